// K34  Analytic edge antialiasing behind K31 (after nvdiffrast, Laine et al. 2020), its two
// transposes -- in the image and in the vertex positions -- and a smoothness term for vertex
// displacements.  K31's picture is piecewise constant in the positions; here two 4-neighbour pixels
// whose ids differ are blended by how far the silhouette edge between their centres reaches, and
// that amount is a smooth function of the edge's two vertices.
//
// No reference counterpart.  The decisions are integers (K31b's edge functions in int64), every
// float operation is one rounded f32 operation in a fixed order (this file is compiled with
// -ffp-contract=off; / is the IEEE division), there are no float atomics and no LDS: the same
// inputs give the same bits on every call, and a numpy restatement gives the same bits.  The
// contract, operation by operation, is in include/ffn_hip.h.
//
//   aa_pair() the pair decision of pixels p and q = p + 1 (axis 0) or p + width (axis 1), ONE
//        function, so every kernel and both pixels of a pair see the same bits: inactive when the ids
//        agree; near = the smaller z-buffer key; attempt(near -> far), else attempt(far -> near) when
//        far is covered.  attempt(a -> b): the triangle f of a must cover a's centre, some E_i must
//        be negative at b; alpha_i = (float)E_i(a) / (float)(E_i(a) - E_i(b)), the smallest one is
//        the exit edge i*; the edge is a silhouette when it has no single neighbour (opposite < 0) or
//        the neighbour's third vertex, projected and snapped as K31a does, lies on f's own side.
//   K34a forward, one thread per pixel: out = in, then for the pairs left, right, up, down that are
//        active with this pixel as the target, out = out + m * (in[source] - in[p]) on r, g, b, a.
//   K34b backward, one thread per pixel: the transpose of K34a in the image, and for the two slots
//        (p, 0), (p, 1) the thread owns the two vertex entries of the pair: the edge's two vertices
//        and d loss / d (their snapped screen position / 256).  Every entry is written on every call.
//   K34c vertex sums, one thread per vertex: the run of the vertex in the stably sorted entries by two
//        binary searches (K33c's), the sum in that order, then through the projection's Jacobian.
//   K34d the gradient of 1/2 sum_edges |x_i - x_j|^2 over a CSR of neighbours, one thread per vertex.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   mesh_aa_forward_kernel      64 VGPRs, 76 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8 waves per SIMD
//   mesh_aa_backward_kernel     72 VGPRs, 88 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 7
//   mesh_aa_vertex_grad_kernel  14 VGPRs, 26 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8
//   mesh_laplacian_kernel       15 VGPRs, 22 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8
// The kernels of mesh_raster.hip, mesh_raster_grad.hip and mesh_texture.hip are not touched: their
// gfx950 disassemblies before and after this file was added are the same.
//
// Not done: a work split for a vertex on a long silhouette (K34c's loop is linear in the run, as
// K33c's), several cameras per launch.  The interior gradients (colour through the barycentric
// weights) are K35's, in mesh_interp_grad.hip.
#include "common.h"
#include "mesh_raster_terms.h"

namespace ffn {

constexpr int64_t kAaMaxPixels = (int64_t)1 << 28;          // 4 P entries index in an int32

struct AaMatrix {
    float p[12];
};

struct AaPair {
    bool active;
    int f, edge;            // the triangle and its exit edge i*
    int a, b;               // the attempt's pixels: f is drawn at a and ends before b
    int target, source;
    float alpha, s, m;
    int64_t d;              // D = E(a) - E(b) > 0
    int sign;               // sign(A)
};

// E_i of K31b at Q = (qx, qy), all three, with sgn(A) applied.  -> A
__device__ __forceinline__ int64_t aa_edges(int4 r0, int4 r1, int64_t qx, int64_t qy, int64_t e[3]) {
    const int64_t x0 = r0.x, y0 = r0.y, x1 = r0.z, y1 = r0.w, x2 = r1.x, y2 = r1.y;
    const int64_t area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    e[0] = (x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1);
    e[1] = (x0 - x2) * (qy - y2) - (y0 - y2) * (qx - x2);
    e[2] = (x1 - x0) * (qy - y0) - (y1 - y0) * (qx - x0);
    if (area < 0) e[0] = -e[0], e[1] = -e[1], e[2] = -e[2];
    return area;
}

__device__ __forceinline__ void aa_corner(int4 r0, int4 r1, int i, int& x, int& y) {
    x = i == 0 ? r0.x : (i == 1 ? r0.z : r1.x);
    y = i == 0 ? r0.y : (i == 1 ? r0.w : r1.y);
}

// attempt(a -> b); on success out holds f, edge, alpha, d, sign, a, b
__device__ __forceinline__ bool aa_attempt(int a, int b, int width, const int4* __restrict__ record,
                                           const int* __restrict__ ids,
                                           const int* __restrict__ opposite,
                                           const float* __restrict__ vertices, int num_vertices,
                                           int num_triangles, const AaMatrix& m, AaPair& out) {
    const int f = ids[a];
    if ((unsigned)f >= (unsigned)num_triangles) return false;
    const int4 r0 = record[4 * (int64_t)f + 0], r1 = record[4 * (int64_t)f + 1];
    int64_t ea[3], eb[3];
    const int64_t area = aa_edges(r0, r1, 256 * (int64_t)(a % width), 256 * (int64_t)(a / width), ea);
    aa_edges(r0, r1, 256 * (int64_t)(b % width), 256 * (int64_t)(b / width), eb);
    if (area == 0 || ea[0] < 0 || ea[1] < 0 || ea[2] < 0) return false;
    int best = -1;
    float best_alpha = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (eb[i] >= 0) continue;
        const float alpha = (float)ea[i] / (float)(ea[i] - eb[i]);
        if (best < 0 || alpha < best_alpha) best = i, best_alpha = alpha;
    }
    if (best < 0) return false;
    const int sign = area < 0 ? -1 : 1;
    const int o = opposite[3 * (int64_t)f + best];
    if (o >= 0) {
        const int id = min(o, num_vertices - 1);
        const float px = vertices[3 * (int64_t)id + 0], py = vertices[3 * (int64_t)id + 1];
        const float pz = vertices[3 * (int64_t)id + 2];
        const float x = ((m.p[0] * px + m.p[1] * py) + m.p[2] * pz) + m.p[3];
        const float y = ((m.p[4] * px + m.p[5] * py) + m.p[6] * pz) + m.p[7];
        const float w = ((m.p[8] * px + m.p[9] * py) + m.p[10] * pz) + m.p[11];
        const float sx = x / w, sy = y / w;
        if (!(w > 0.0f) || !(fabsf(sx) <= kRasterGuard) || !(fabsf(sy) <= kRasterGuard)) return false;
        const int64_t ox = (int)rintf(sx * 256.0f), oy = (int)rintf(sy * 256.0f);
        int xj, yj, xk, yk;
        aa_corner(r0, r1, (best + 1) % 3, xj, yj);
        aa_corner(r0, r1, (best + 2) % 3, xk, yk);
        int64_t side = (int64_t)(xk - xj) * (oy - yj) - (int64_t)(yk - yj) * (ox - xj);
        if (sign < 0) side = -side;
        if (side < 0) return false;         // an interior edge: the surface goes on
    }
    out.f = f, out.edge = best, out.alpha = best_alpha, out.d = ea[best] - eb[best];
    out.sign = sign, out.a = a, out.b = b;
    return true;
}

// the decision of the pair (p, q), q = p + 1 or p + width inside the image
__device__ __forceinline__ AaPair aa_pair(int p, int q, int width,
                                          const unsigned long long* __restrict__ zbuf,
                                          const int4* __restrict__ record,
                                          const int* __restrict__ ids,
                                          const int* __restrict__ opposite,
                                          const float* __restrict__ vertices, int num_vertices,
                                          int num_triangles, const AaMatrix& m) {
    AaPair pair;
    pair.active = false;
    if (ids[p] == ids[q]) return pair;
    const bool q_near = zbuf[q] < zbuf[p];
    const int near = q_near ? q : p, far = q_near ? p : q;
    bool found = aa_attempt(near, far, width, record, ids, opposite, vertices, num_vertices,
                            num_triangles, m, pair);
    if (!found && ids[far] >= 0)
        found = aa_attempt(far, near, width, record, ids, opposite, vertices, num_vertices,
                           num_triangles, m, pair);
    if (!found) return pair;
    pair.active = true;
    pair.s = pair.alpha - 0.5f;
    pair.target = pair.s >= 0.0f ? pair.b : pair.a;
    pair.source = pair.s >= 0.0f ? pair.a : pair.b;
    pair.m = fabsf(pair.s);
    return pair;
}

// the four pairs of pixel p in the order left, right, up, down: (first pixel, second pixel) of
// pair n, or false when it does not exist
__device__ __forceinline__ bool aa_neighbor(int p, int n, int width, int height, int& first,
                                            int& second) {
    const int px = p % width, py = p / width;
    if (n == 0) { first = p - 1, second = p; return px > 0; }
    if (n == 1) { first = p, second = p + 1; return px + 1 < width; }
    if (n == 2) { first = p - width, second = p; return py > 0; }
    first = p, second = p + width;
    return py + 1 < height;
}

__device__ __forceinline__ float aa_channel(const float* __restrict__ color,
                                            const float* __restrict__ alpha, int pixel, int c) {
    return c < 3 ? color[3 * (int64_t)pixel + c] : alpha[pixel];
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_aa_forward_kernel(const int4* __restrict__ record, const unsigned long long* __restrict__ zbuf,
                       const int* __restrict__ ids, const int* __restrict__ opposite,
                       const float* __restrict__ vertices, int num_vertices, int num_triangles,
                       AaMatrix m, const float* __restrict__ color, const float* __restrict__ alpha,
                       int width, int height, float* __restrict__ out_color,
                       float* __restrict__ out_alpha) {
    const int p = blockIdx.x * kRasterThreads + threadIdx.x;         // W H <= 2^28
    if (p >= width * height) return;
    float own[4], out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = own[c] = aa_channel(color, alpha, p, c);
    for (int n = 0; n < 4; ++n) {
        int first, second;
        if (!aa_neighbor(p, n, width, height, first, second)) continue;
        const AaPair pair = aa_pair(first, second, width, zbuf, record, ids, opposite, vertices,
                                    num_vertices, num_triangles, m);
        if (!pair.active || pair.target != p) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            out[c] = out[c] + pair.m * (aa_channel(color, alpha, pair.source, c) - own[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out_color[3 * (int64_t)p + c] = out[c];
    out_alpha[p] = out[3];
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_aa_backward_kernel(const int4* __restrict__ record, const unsigned long long* __restrict__ zbuf,
                        const int* __restrict__ ids, const int* __restrict__ opposite,
                        const float* __restrict__ vertices, int num_vertices,
                        const int* __restrict__ triangles, int num_triangles, AaMatrix m,
                        const float* __restrict__ color, const float* __restrict__ alpha,
                        const float* __restrict__ g_color, const float* __restrict__ g_alpha,
                        int width, int height, float* __restrict__ d_color,
                        float* __restrict__ d_alpha, int* __restrict__ entry_vertex,
                        float2* __restrict__ entry_grad) {
    const int p = blockIdx.x * kRasterThreads + threadIdx.x;         // W H <= 2^28
    if (p >= width * height) return;
    float own[4], d[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) d[c] = own[c] = aa_channel(g_color, g_alpha, p, c);
    for (int n = 0; n < 4; ++n) {
        int first, second;
        const bool exists = aa_neighbor(p, n, width, height, first, second);
        AaPair pair;
        pair.active = false;
        if (exists)
            pair = aa_pair(first, second, width, zbuf, record, ids, opposite, vertices,
                           num_vertices, num_triangles, m);
        if (pair.active) {
            if (pair.target == p) {
#pragma unroll
                for (int c = 0; c < 4; ++c) d[c] = d[c] - pair.m * own[c];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    d[c] = d[c] + pair.m * aa_channel(g_color, g_alpha, pair.target, c);
            }
        }
        if (n != 1 && n != 3) continue;
        // the slots (p, 0) and (p, 1) are this thread's: two entries each
        const int e = 4 * p + (n == 1 ? 0 : 2);
        int v0 = num_vertices, v1 = num_vertices;
        float2 grad0 = make_float2(0.0f, 0.0f), grad1 = make_float2(0.0f, 0.0f);
        if (pair.active) {
            float delta[4], g[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                delta[c] = aa_channel(color, alpha, pair.source, c)
                           - aa_channel(color, alpha, pair.target, c);
                g[c] = aa_channel(g_color, g_alpha, pair.target, c);
            }
            const float total = ((g[0] * delta[0] + g[1] * delta[1]) + g[2] * delta[2])
                                + g[3] * delta[3];
            const float d_alpha_pair = pair.s >= 0.0f ? total : -total;
            const int4 r0 = record[4 * (int64_t)pair.f + 0], r1 = record[4 * (int64_t)pair.f + 1];
            const int j = (pair.edge + 1) % 3, k = (pair.edge + 2) % 3;
            int xj, yj, xk, yk;
            aa_corner(r0, r1, j, xj, yj);
            aa_corner(r0, r1, k, xk, yk);
            const int ax = pair.a % width, ay = pair.a / width;
            const int bx = pair.b % width, by = pair.b / width;
            const float cx = (float)(256 * ax) + pair.alpha * (float)(256 * (bx - ax));
            const float cy = (float)(256 * ay) + pair.alpha * (float)(256 * (by - ay));
            const float cjx = cx - (float)xj, cjy = cy - (float)yj;
            const float ckx = cx - (float)xk, cky = cy - (float)yk;
            const float signed_grad = pair.sign < 0 ? -d_alpha_pair : d_alpha_pair;
            const float r256 = 256.0f * (signed_grad / (float)pair.d);
            const int last_vertex = num_vertices - 1;
            v0 = min(max(triangles[3 * (int64_t)pair.f + k], 0), last_vertex);
            v1 = min(max(triangles[3 * (int64_t)pair.f + j], 0), last_vertex);
            grad0 = make_float2(r256 * cjy, -(r256 * cjx));
            grad1 = make_float2(-(r256 * cky), r256 * ckx);
        }
        entry_vertex[e + 0] = v0;
        entry_vertex[e + 1] = v1;
        entry_grad[e + 0] = grad0;
        entry_grad[e + 1] = grad1;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d_color[3 * (int64_t)p + c] = d[c];
    d_alpha[p] = d[3];
}

// the first position in the ascending sorted[0 .. n) that holds key or more (K33c's search)
__device__ __forceinline__ int aa_lower_bound(const int* __restrict__ sorted, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_aa_vertex_grad_kernel(const int* __restrict__ sorted_vertex, const int* __restrict__ order,
                           const float2* __restrict__ entry_grad, int num_entries,
                           const float* __restrict__ vertices, int num_vertices, AaMatrix m,
                           int accumulate, float* __restrict__ grad) {
    const int v = blockIdx.x * kRasterThreads + threadIdx.x;         // V <= (2^31 - 1) / 3
    if (v >= num_vertices) return;
    // both ends lie in 0 .. N whatever sorted_vertex holds
    const int begin = aa_lower_bound(sorted_vertex, num_entries, v);
    const int end = aa_lower_bound(sorted_vertex, num_entries, v + 1);
    float gx = 0.0f, gy = 0.0f;
    for (int at = begin; at < end; ++at) {
        const int e = order[at];
        if ((unsigned)e >= (unsigned)num_entries) continue;
        const float2 g = entry_grad[e];
        gx = gx + g.x;
        gy = gy + g.y;
    }
    const float px = vertices[3 * (int64_t)v + 0], py = vertices[3 * (int64_t)v + 1];
    const float pz = vertices[3 * (int64_t)v + 2];
    const float x = ((m.p[0] * px + m.p[1] * py) + m.p[2] * pz) + m.p[3];
    const float y = ((m.p[4] * px + m.p[5] * py) + m.p[6] * pz) + m.p[7];
    const float w = ((m.p[8] * px + m.p[9] * py) + m.p[10] * pz) + m.p[11];
    const float sx = x / w, sy = y / w;
    float value[3] = {0.0f, 0.0f, 0.0f};
    if (w > 0.0f) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            value[c] = ((gx * (m.p[c] - sx * m.p[8 + c])) + (gy * (m.p[4 + c] - sy * m.p[8 + c]))) / w;
    }
    float* out = grad + 3 * (int64_t)v;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = accumulate ? out[c] + value[c] : value[c];
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_laplacian_kernel(const float* __restrict__ values, const int* __restrict__ neighbor_starts,
                      const int* __restrict__ neighbors, int num_vertices, int num_neighbors,
                      float scale, int accumulate, float* __restrict__ out) {
    const int v = blockIdx.x * kRasterThreads + threadIdx.x;
    if (v >= num_vertices) return;
    // rows that are not a CSR of neighbors must not read outside it
    const int begin = max(neighbor_starts[v], 0), end = min(neighbor_starts[v + 1], num_neighbors);
    const float x0 = values[3 * (int64_t)v + 0], x1 = values[3 * (int64_t)v + 1];
    const float x2 = values[3 * (int64_t)v + 2];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int at = begin; at < end; ++at) {
        const int n = neighbors[at];
        if ((unsigned)n >= (unsigned)num_vertices) continue;
        a0 = a0 + (x0 - values[3 * (int64_t)n + 0]);
        a1 = a1 + (x1 - values[3 * (int64_t)n + 1]);
        a2 = a2 + (x2 - values[3 * (int64_t)n + 2]);
    }
    float* row = out + 3 * (int64_t)v;
    if (accumulate) {
        row[0] = row[0] + scale * a0;
        row[1] = row[1] + scale * a1;
        row[2] = row[2] + scale * a2;
    } else {
        row[0] = scale * a0;
        row[1] = scale * a1;
        row[2] = scale * a2;
    }
}

static inline bool aa_bad_pixels(int width, int height) {
    return raster_bad_image(width, height) || (int64_t)width * height > kAaMaxPixels;
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_aa_forward(const int32_t* record, const uint64_t* zbuf, const int32_t* ids,
                                   const int32_t* opposite, const float* vertices,
                                   int64_t num_vertices, int64_t num_triangles, const float* proj,
                                   const float* color, const float* alpha, int width, int height,
                                   float* out_color, float* out_alpha, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_aa_forward: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (aa_bad_pixels(width, height))
        return fail_arg("ffn_mesh_aa_forward: image (1 <= width, height <= 16384, at most 2^28 "
                        "pixels)");
    if (!record || !zbuf || !ids || !opposite || !vertices || !proj || !color || !alpha ||
        !out_color || !out_alpha)
        return fail_arg("ffn_mesh_aa_forward: null argument");
    if (((uintptr_t)record & 15) != 0 || ((uintptr_t)zbuf & 7) != 0)
        return fail_arg("ffn_mesh_aa_forward: record must be 16-byte, zbuf 8-byte aligned");
    AaMatrix m;
    for (int i = 0; i < 12; ++i) m.p[i] = proj[i];
    const unsigned blocks = (unsigned)(((int64_t)width * height + kRasterThreads - 1) /
                                       kRasterThreads);
    hipLaunchKernelGGL(mesh_aa_forward_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)record, (const unsigned long long*)zbuf,
                       ids, opposite, vertices, (int)num_vertices, (int)num_triangles, m, color,
                       alpha, width, height, out_color, out_alpha);
    return check_launch("ffn_mesh_aa_forward");
}

extern "C" int ffn_mesh_aa_backward(const int32_t* record, const uint64_t* zbuf, const int32_t* ids,
                                    const int32_t* opposite, const float* vertices,
                                    int64_t num_vertices, const int32_t* triangles,
                                    int64_t num_triangles, const float* proj, const float* color,
                                    const float* alpha, const float* g_color, const float* g_alpha,
                                    int width, int height, float* d_color, float* d_alpha,
                                    int32_t* entry_vertex, float* entry_grad, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_aa_backward: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (aa_bad_pixels(width, height))
        return fail_arg("ffn_mesh_aa_backward: image (1 <= width, height <= 16384, at most 2^28 "
                        "pixels)");
    if (!record || !zbuf || !ids || !opposite || !vertices || !triangles || !proj || !color ||
        !alpha || !g_color || !g_alpha || !d_color || !d_alpha || !entry_vertex || !entry_grad)
        return fail_arg("ffn_mesh_aa_backward: null argument");
    if (((uintptr_t)record & 15) != 0 || ((uintptr_t)zbuf & 7) != 0 ||
        ((uintptr_t)entry_grad & 7) != 0)
        return fail_arg("ffn_mesh_aa_backward: record must be 16-byte, zbuf and entry_grad 8-byte "
                        "aligned");
    AaMatrix m;
    for (int i = 0; i < 12; ++i) m.p[i] = proj[i];
    const unsigned blocks = (unsigned)(((int64_t)width * height + kRasterThreads - 1) /
                                       kRasterThreads);
    hipLaunchKernelGGL(mesh_aa_backward_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)record, (const unsigned long long*)zbuf,
                       ids, opposite, vertices, (int)num_vertices, triangles, (int)num_triangles, m,
                       color, alpha, g_color, g_alpha, width, height, d_color, d_alpha,
                       entry_vertex, (float2*)entry_grad);
    return check_launch("ffn_mesh_aa_backward");
}

extern "C" int ffn_mesh_aa_vertex_grad(const int32_t* sorted_vertex, const int32_t* order,
                                       const float* entry_grad, int64_t num_pixels,
                                       const float* vertices, int64_t num_vertices,
                                       const float* proj, float* grad, int accumulate,
                                       void* stream) {
    if (num_pixels < 1 || num_pixels > kAaMaxPixels)
        return fail_arg("ffn_mesh_aa_vertex_grad: shape (1 <= num_pixels <= 2^28)");
    if (num_vertices < 1 || num_vertices > 0x7fffffff / 3)
        return fail_arg("ffn_mesh_aa_vertex_grad: shape (1 <= num_vertices <= (2^31 - 1) / 3)");
    if (!sorted_vertex || !order || !entry_grad || !vertices || !proj || !grad)
        return fail_arg("ffn_mesh_aa_vertex_grad: null argument");
    if (((uintptr_t)entry_grad & 7) != 0)
        return fail_arg("ffn_mesh_aa_vertex_grad: entry_grad must be 8-byte aligned");
    AaMatrix m;
    for (int i = 0; i < 12; ++i) m.p[i] = proj[i];
    const unsigned blocks = (unsigned)((num_vertices + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_aa_vertex_grad_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, sorted_vertex, order, (const float2*)entry_grad,
                       (int)(4 * num_pixels), vertices, (int)num_vertices, m, accumulate, grad);
    return check_launch("ffn_mesh_aa_vertex_grad");
}

extern "C" int ffn_mesh_laplacian(const float* values, const int32_t* neighbor_starts,
                                  const int32_t* neighbors, int64_t num_vertices,
                                  int64_t num_neighbors, float scale, float* out, int accumulate,
                                  void* stream) {
    if (num_vertices < 1 || num_vertices > 0x7fffffff / 3)
        return fail_arg("ffn_mesh_laplacian: shape (1 <= num_vertices <= (2^31 - 1) / 3)");
    if (num_neighbors < 0 || num_neighbors > 0x7fffffff)
        return fail_arg("ffn_mesh_laplacian: shape (0 <= num_neighbors < 2^31)");
    if (!values || !neighbor_starts || !out || (num_neighbors > 0 && !neighbors))
        return fail_arg("ffn_mesh_laplacian: null argument");
    const unsigned blocks = (unsigned)((num_vertices + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_laplacian_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, values, neighbor_starts, neighbors, (int)num_vertices,
                       (int)num_neighbors, scale, accumulate, out);
    return check_launch("ffn_mesh_laplacian");
}
