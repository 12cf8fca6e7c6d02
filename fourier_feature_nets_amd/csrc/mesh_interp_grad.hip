// K35  The interior half of the geometry gradient behind K31 (after nvdiffrast, Laine et al. 2020):
// colour through the barycentric weights.  K34 (mesh_aa.hip) moves the vertices a camera sees on an
// outline; here every pixel a triangle wins pulls the triangle's three corners by how K31c's colour
// (c_v0 b0 + c_v1 b1) + c_v2 b2 changes when the sample point slides over the triangle.  Which
// triangle wins a pixel is held fixed, and the snap to 1/256 pixel is passed straight through.
//
// No reference counterpart.  The edge functions are int64 (K31b's), every float operation is one
// rounded f32 operation in a fixed order (this file is compiled with -ffp-contract=off; / is the
// IEEE division), there are no float atomics and no LDS: the same inputs give the same bits on every
// call, and a numpy restatement gives the same bits.  The contract, operation by operation, is in
// include/ffn_hip.h.
//
//   K35a face gradients, K32a's organisation: one wavefront of 64 lanes per triangle f (grid-stride
//        over triangles, at most 2^16 blocks).  The box of record[f]; a box that is empty, not
//        inside the image or of more than 2^28 pixels contributes nothing, so a bad record never
//        indexes outside the image.  Box pixel k is selected iff ids[pixel] == f; a pixel that is not
//        selected is skipped: its d_color is not read.  Per triangle (the same in all lanes) the
//        three corner colours, vertex ids clamped into [0, V), and n_i = (256 d E_i / d Q) / |A|, the
//        gradient of lambda_i per pixel.  Per selected pixel lambda_i = (float)E_i / (float)|A|,
//        q_i, depth_w, b_i (the bits of K31c), C, a_i = g . (c_i - C), r_i = (a_i depth_w) / w_i,
//        G = (r_0 n_0 + r_1 n_1) + r_2 n_2 and the nine terms t[3j] = -(lambda_j G_x),
//        t[3j+1] = -(lambda_j G_y), t[3j+2] = -(r_j q_j).  Segments, butterfly and the order of the
//        sums are K32a's.  face_grads[f] = the nine sums; every row is written.
//   K35b vertex sums, one thread per vertex v over K32b's CSR (corner_order, vertex_starts) with its
//        guards: (gx, gy, gw) from 0.0f in CSR order, then K34c's projection Jacobian and the w
//        term: value[c] = ((gx (P[c] - sx P[8+c])) + (gy (P[4+c] - sy P[8+c]))) / w + gw P[8+c],
//        zero unless w > 0; grad[v] = value or grad[v] + value with accumulate.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   mesh_interp_face_grads_kernel   55 VGPRs, 78 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of
//                                   LDS, occupancy 8 waves per SIMD.  K32a has 50 VGPRs and 64
//                                   SGPRs: the pixel body keeps lambda_i, q_i and r_i live at once,
//                                   and the nine corner colours and the six n_i are the same in all
//                                   lanes and sit in SGPRs (the record, the vertex ids and the
//                                   colours come through scalar loads).  The
//                                   butterfly is 54 ds_bpermute_b32 per segment (9 values, 6 steps)
//                                   against K32a's 72; a selected pixel has ten IEEE divisions
//                                   against K32a's seven.  No contraction: the v_fma_f32 in the
//                                   listing are the division's own expansion.
//   mesh_interp_vertex_grad_kernel  17 VGPRs, 26 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of
//                                   LDS, occupancy 8
// mesh_raster_terms.h is not changed (raster_terms() returns no lambda_i: interp_edges() below
// recomputes K31b's three edge functions), and neither are the kernels of mesh_raster.hip,
// mesh_raster_grad.hip, mesh_texture.hip and mesh_aa.hip (of the last only the header comment):
// their gfx950 disassemblies before and after this file was added differ in the compilation-unit
// id alone.
//
// Not done: the textured path (the derivative of K31c's bilinear lookup in the UVs), a joint colour
// and geometry step, a work split for a screen-filling triangle (one wave's loop over
// ceil(n / 64) segments, as K32a's), a vertex of huge valence (K35b's loop is linear in it).
#include "common.h"
#include "mesh_raster_terms.h"

namespace ffn {

constexpr int kInterpWave = 64;
constexpr int kInterpWavesPerBlock = kRasterThreads / kInterpWave;
constexpr int kInterpMaxBlocks = 1 << 16;
constexpr int64_t kInterpMaxBox = (int64_t)1 << 28;

struct InterpMatrix {
    float p[12];
};

__device__ __forceinline__ float interp_fold(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, kInterpWave);
    return x;
}

// E_0 .. E_2 of K31b at the centre of pixel (px, py) with sgn(A) applied
__device__ __forceinline__ void interp_edges(int4 r0, int4 r1, int px, int py, int64_t e[3]) {
    const int64_t x0 = r0.x, y0 = r0.y, x1 = r0.z, y1 = r0.w, x2 = r1.x, y2 = r1.y;
    const int64_t area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    const int64_t qx = 256 * (int64_t)px, qy = 256 * (int64_t)py;
    e[0] = (x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1);
    e[1] = (x0 - x2) * (qy - y2) - (y0 - y2) * (qx - x2);
    e[2] = (x1 - x0) * (qy - y0) - (y1 - y0) * (qx - x0);
    if (area < 0) e[0] = -e[0], e[1] = -e[1], e[2] = -e[2];
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_interp_face_grads_kernel(const int4* __restrict__ record, const int* __restrict__ ids,
                              const float* __restrict__ d_color, const float* __restrict__ colors,
                              const int* __restrict__ triangles, int num_triangles,
                              int num_vertices, int width, int height,
                              float* __restrict__ face_grads) {
    const int lane = threadIdx.x & (kInterpWave - 1);
    // (the wave's number is the same in all of its lanes: say so, the loops below are uniform)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kInterpWave);
    const int stride = gridDim.x * kInterpWavesPerBlock;
    for (int f = blockIdx.x * kInterpWavesPerBlock + wave; f < num_triangles; f += stride) {
        const int4 r0 = record[4 * (int64_t)f + 0], r1 = record[4 * (int64_t)f + 1];
        const int4 r2 = record[4 * (int64_t)f + 2], r3 = record[4 * (int64_t)f + 3];
        const int x0 = r2.y, y0 = r2.z, x1 = r2.w, y1 = r3.x;
        int box_width = 1;
        int64_t n = 0;
        // a record that does not belong to the image must not index outside it
        if (x0 >= 0 && y0 >= 0 && x1 < width && y1 < height && x1 >= x0 && y1 >= y0) {
            box_width = x1 - x0 + 1;
            n = (int64_t)box_width * (y1 - y0 + 1);
        }
        if (n > kInterpMaxBox) n = 0;
        const int count = (int)n;

        float acc[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) acc[c] = 0.0f;
        if (count > 0) {
            // what every pixel of the triangle shares
            const int64_t cx[3] = {r0.x, r0.z, r1.x}, cy[3] = {r0.y, r0.w, r1.y};
            const int64_t area = (cx[1] - cx[0]) * (cy[2] - cy[0]) - (cy[1] - cy[0]) * (cx[2] - cx[0]);
            const float denominator = (float)(area < 0 ? -area : area);
            const float w[3] = {__int_as_float(r1.z), __int_as_float(r1.w), __int_as_float(r2.x)};
            float nx[3], ny[3], corner[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int j = (i + 1) % 3, k = (i + 2) % 3;
                int64_t dx = -(cy[k] - cy[j]), dy = cx[k] - cx[j];
                if (area < 0) dx = -dx, dy = -dy;
                nx[i] = (256.0f * (float)dx) / denominator;
                ny[i] = (256.0f * (float)dy) / denominator;
                const int v = min(max(triangles[3 * (int64_t)f + i], 0), num_vertices - 1);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) corner[i][ch] = colors[3 * (int64_t)v + ch];
            }
            for (int first = 0; first < count; first += kInterpWave) {
                float t[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) t[c] = 0.0f;
                const int k = first + lane;
                if (k < count) {
                    const int px = x0 + k % box_width, py = y0 + k / box_width;
                    const int pixel = py * width + px;               // inside the image: < 2^28
                    if (ids[pixel] == f) {
                        int64_t e[3];
                        interp_edges(r0, r1, px, py, e);
                        float lambda[3], q[3], b[3], g[3], mixed[3], r[3];
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            lambda[i] = (float)e[i] / denominator;
                            q[i] = lambda[i] / w[i];
                        }
                        const float inv_w = (q[0] + q[1]) + q[2];
                        const float depth_w = 1.0f / inv_w;
#pragma unroll
                        for (int i = 0; i < 3; ++i) b[i] = q[i] * depth_w;
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            g[ch] = d_color[3 * (int64_t)pixel + ch];
                            mixed[ch] = (corner[0][ch] * b[0] + corner[1][ch] * b[1])
                                        + corner[2][ch] * b[2];
                        }
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const float a = (g[0] * (corner[i][0] - mixed[0])
                                             + g[1] * (corner[i][1] - mixed[1]))
                                            + g[2] * (corner[i][2] - mixed[2]);
                            r[i] = (a * depth_w) / w[i];
                        }
                        const float gx = (r[0] * nx[0] + r[1] * nx[1]) + r[2] * nx[2];
                        const float gy = (r[0] * ny[0] + r[1] * ny[1]) + r[2] * ny[2];
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            t[3 * j + 0] = -(lambda[j] * gx);
                            t[3 * j + 1] = -(lambda[j] * gy);
                            t[3 * j + 2] = -(r[j] * q[j]);
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 9; ++c) acc[c] = acc[c] + interp_fold(t[c]);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) face_grads[9 * (int64_t)f + c] = acc[c];
        }
    }
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_interp_vertex_grad_kernel(const float* __restrict__ face_grads,
                               const int* __restrict__ corner_order,
                               const int* __restrict__ vertex_starts, int num_corners,
                               const float* __restrict__ vertices, int num_vertices, InterpMatrix m,
                               int accumulate, float* __restrict__ grad) {
    const int v = blockIdx.x * kRasterThreads + threadIdx.x;         // V <= (2^31 - 1) / 3
    if (v >= num_vertices) return;
    // rows that are not a CSR of corner_order must not read outside it
    const int begin = max(vertex_starts[v], 0), end = min(vertex_starts[v + 1], num_corners);
    float gx = 0.0f, gy = 0.0f, gw = 0.0f;
    for (int at = begin; at < end; ++at) {
        const int corner = corner_order[at];
        if ((unsigned)corner >= (unsigned)num_corners) continue;
        const float* row = face_grads + 3 * (int64_t)corner;          // 9 f + 3 i
        gx = gx + row[0];
        gy = gy + row[1];
        gw = gw + row[2];
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
            value[c] = ((gx * (m.p[c] - sx * m.p[8 + c])) + (gy * (m.p[4 + c] - sy * m.p[8 + c]))) / w
                       + gw * m.p[8 + c];
    }
    float* out = grad + 3 * (int64_t)v;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = accumulate ? out[c] + value[c] : value[c];
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_interp_face_grads(const int32_t* record, const int32_t* ids,
                                          const float* d_color, const float* colors,
                                          int64_t num_vertices, const int32_t* triangles,
                                          int64_t num_triangles, int width, int height,
                                          float* face_grads, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_interp_face_grads: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (raster_bad_image(width, height))
        return fail_arg("ffn_mesh_interp_face_grads: image (1 <= width, height <= 16384)");
    if (!record || !ids || !d_color || !colors || !triangles || !face_grads)
        return fail_arg("ffn_mesh_interp_face_grads: null argument");
    if (((uintptr_t)record & 15) != 0)
        return fail_arg("ffn_mesh_interp_face_grads: record must be 16-byte aligned");
    const int64_t wanted = (num_triangles + kInterpWavesPerBlock - 1) / kInterpWavesPerBlock;
    const unsigned blocks = (unsigned)(wanted < kInterpMaxBlocks ? wanted : kInterpMaxBlocks);
    hipLaunchKernelGGL(mesh_interp_face_grads_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)record, ids, d_color, colors, triangles,
                       (int)num_triangles, (int)num_vertices, width, height, face_grads);
    return check_launch("ffn_mesh_interp_face_grads");
}

extern "C" int ffn_mesh_interp_vertex_grad(const float* face_grads, const int32_t* corner_order,
                                           const int32_t* vertex_starts, int64_t num_triangles,
                                           const float* vertices, int64_t num_vertices,
                                           const float* proj, float* grad, int accumulate,
                                           void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_interp_vertex_grad: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (!face_grads || !corner_order || !vertex_starts || !vertices || !proj || !grad)
        return fail_arg("ffn_mesh_interp_vertex_grad: null argument");
    InterpMatrix m;
    for (int i = 0; i < 12; ++i) m.p[i] = proj[i];
    const unsigned blocks = (unsigned)((num_vertices + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_interp_vertex_grad_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, face_grads, corner_order, vertex_starts,
                       (int)(3 * num_triangles), vertices, (int)num_vertices, m, accumulate, grad);
    return check_launch("ffn_mesh_interp_vertex_grad");
}
