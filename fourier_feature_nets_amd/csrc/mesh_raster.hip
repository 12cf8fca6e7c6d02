// K31  A z-buffer rasteriser for coloured or textured triangle meshes: the picture of a mesh from a
// pinhole camera, as RenderResult(color, alpha, depth) and the id of the triangle in every pixel.
//
// No reference counterpart (the reference looks at meshes with an external viewer).  Coverage is
// decided on integers, and every float operation is one rounded f32 operation in a fixed order
// (this file is compiled with -ffp-contract=off; / and sqrtf are the IEEE operations), so the
// same inputs give the same image on every call and for any chunk size, and a numpy-f32
// restatement gives the same bits.  Pixel (px, py) is the ray through the integer coordinates
// (px, py), as everywhere in the project.
//
//   K31a set-up, one thread per triangle.  Vertex ids clamped into [0, V-1] (K22).  Per vertex
//        K23's projection, x = ((P00 px + P01 py) + P02 pz) + P03, likewise y and w; sx = x / w,
//        sy = y / w; X = (int)rintf(sx * 256.0f), Y likewise: 24.8 fixed point.  Status byte:
//          1 behind      all three w <= 0
//          2 clipped     some !(w > 0), or some !(fabsf(s) <= 16384.0f) (guard band; NaN, inf)
//          3 degenerate  A == 0, A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) in int64
//          4 off-image   the clamped box is empty
//          0 drawn       everything else
//        box x0 = max(0, ceil(minX / 256)), x1 = min(W-1, floor(maxX / 256)), likewise y, in
//        integers with floor division.  counts[f] = (x1-x0+1)(y1-y0+1) for a drawn triangle, 0 for
//        every other.  record[f] = 16 words: X0 Y0 X1 Y1 | X2 Y2 w0 w1 | w2 x0 y0 x1 | y1 0 0 0
//        (X, Y zero when behind or clipped; the box 0 0 -1 -1 unless drawn).  There is no
//        near-plane clipping: a clipped triangle is not drawn, its status says so.
//   K31b raster, one thread per box pixel s of a chunk [first, first + count).  f by binary search
//        in the exclusive int64 scan of counts (K22's search), k = s - offsets[f],
//        (px, py) = (x0 + k % bw, y0 + k / bw).  raster_terms() (mesh_raster_terms.h, shared
//        with K32, mesh_raster_grad.hip): Q = (256 px, 256 py),
//        E_i = sgn(A) [(X_k - X_j)(Q_y - Y_j) - (Y_k - Y_j)(Q_x - X_j)], (j, k) = (i+1, i+2) mod 3,
//        int64; covered iff all E_i >= 0 (inclusive, two-sided: a shared edge belongs to both
//        triangles, the z-buffer decides).  l_i = (float)E_i / (float)|A|, q_i = l_i / w_i,
//        inv_w = (q0 + q1) + q2, depth_w = 1.0f / inv_w; skipped unless depth_w is finite and > 0.
//        key = bits(depth_w) << 32 | f; unsigned 64-bit atomicMin on zbuf[py W + px] (all ones =
//        empty).  Positive f32 bits are monotone, so the minimum is exact and independent of the
//        order; ties go to the lower id.  A plain load first skips the atomic where the pixel
//        already holds less (K21a).  One integer atomic per covered pixel at most, spread over the
//        image; no float atomics, no LDS.
//   K31c resolve, one thread per pixel.  Empty key: background, alpha 0, depth 0, id -1.  Else the
//        triangle of the low word, raster_terms() again (the same bits), b_i = q_i * depth_w;
//        colour (c0 b0 + c1 b1) + c2 b2 per channel, or the UV interpolated the same way and put
//        through K22's lookup (mesh_terms.h); p = (v0 b0 + v1 b1) + v2 b2 per component,
//        d = p - eye, depth = sqrtf((dx dx + dy dy) + dz dz): the t of OcTree.render.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   mesh_raster_setup_kernel    34 VGPRs, 28 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8 waves per SIMD
//   mesh_raster_draw_kernel     36 VGPRs, 15 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8; the atomic is one global_atomic_umin_x2 without a
//                               return value, no compare-and-swap loop
//   mesh_raster_resolve_kernel  51 VGPRs, 30 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8
// mesh_sample_kernel (mesh.hip) compiles to the instructions it had before its texture lookup moved
// into mesh_terms.h (the disassemblies differ in the compilation-unit id alone).
#include "common.h"
#include "mesh_terms.h"
#include "mesh_raster_terms.h"

namespace ffn {

enum : uint8_t { kRasterDrawn = 0, kRasterBehind = 1, kRasterClipped = 2, kRasterDegenerate = 3,
                 kRasterOffImage = 4 };

struct RasterMatrix {
    float p[12];
};
struct RasterVec3 {
    float v[3];
};

__device__ __forceinline__ int raster_floor256(int a) { return a >> 8; }
__device__ __forceinline__ int raster_ceil256(int a) { return -((-a) >> 8); }

__global__ void __launch_bounds__(kRasterThreads)
mesh_raster_setup_kernel(const float* __restrict__ vertices, int num_vertices,
                         const int* __restrict__ triangles, int num_triangles, RasterMatrix m,
                         int width, int height, int4* __restrict__ record,
                         uint8_t* __restrict__ status, int64_t* __restrict__ counts) {
    const int f = blockIdx.x * kRasterThreads + threadIdx.x;
    if (f >= num_triangles) return;
    const int last_vertex = num_vertices - 1;
    float w[3], sx[3], sy[3];
    int behind = 0;
    bool clipped = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int id = min(max(triangles[3 * (int64_t)f + i], 0), last_vertex);
        const float px = vertices[3 * (int64_t)id + 0], py = vertices[3 * (int64_t)id + 1];
        const float pz = vertices[3 * (int64_t)id + 2];
        const float x = ((m.p[0] * px + m.p[1] * py) + m.p[2] * pz) + m.p[3];
        const float y = ((m.p[4] * px + m.p[5] * py) + m.p[6] * pz) + m.p[7];
        w[i] = ((m.p[8] * px + m.p[9] * py) + m.p[10] * pz) + m.p[11];
        sx[i] = x / w[i];
        sy[i] = y / w[i];
        behind += w[i] <= 0.0f;
        clipped |= !(w[i] > 0.0f) || !(fabsf(sx[i]) <= kRasterGuard) ||
                   !(fabsf(sy[i]) <= kRasterGuard);
    }
    int fx[3] = {0, 0, 0}, fy[3] = {0, 0, 0};
    int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
    uint8_t state = kRasterDrawn;
    if (behind == 3) {
        state = kRasterBehind;
    } else if (clipped) {
        state = kRasterClipped;
    } else {
        // |s| <= 2^14, so |X| <= 2^22: the conversion is defined and the products fit an int64
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            fx[i] = (int)rintf(sx[i] * 256.0f);
            fy[i] = (int)rintf(sy[i] * 256.0f);
        }
        const int64_t area = (int64_t)(fx[1] - fx[0]) * (fy[2] - fy[0]) -
                             (int64_t)(fy[1] - fy[0]) * (fx[2] - fx[0]);
        const int cx0 = max(0, raster_ceil256(min(fx[0], min(fx[1], fx[2]))));
        const int cx1 = min(width - 1, raster_floor256(max(fx[0], max(fx[1], fx[2]))));
        const int cy0 = max(0, raster_ceil256(min(fy[0], min(fy[1], fy[2]))));
        const int cy1 = min(height - 1, raster_floor256(max(fy[0], max(fy[1], fy[2]))));
        if (area == 0) {
            state = kRasterDegenerate;
        } else if (cx1 < cx0 || cy1 < cy0) {
            state = kRasterOffImage;
        } else {
            bx0 = cx0, by0 = cy0, bx1 = cx1, by1 = cy1;
        }
    }
    record[4 * (int64_t)f + 0] = make_int4(fx[0], fy[0], fx[1], fy[1]);
    record[4 * (int64_t)f + 1] = make_int4(fx[2], fy[2], __float_as_int(w[0]), __float_as_int(w[1]));
    record[4 * (int64_t)f + 2] = make_int4(__float_as_int(w[2]), bx0, by0, bx1);
    record[4 * (int64_t)f + 3] = make_int4(by1, 0, 0, 0);
    status[f] = state;
    counts[f] = (int64_t)(bx1 - bx0 + 1) * (by1 - by0 + 1);
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_raster_draw_kernel(const int4* __restrict__ record, const int64_t* __restrict__ offsets,
                        int num_triangles, int64_t first, int64_t count, int width, int height,
                        unsigned long long* __restrict__ zbuf) {
    const int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    if (i >= count) return;
    const int64_t s = first + i;

    // offsets[lo] <= s < offsets[hi] throughout (offsets[0] = 0, offsets[num_triangles] > s)
    int lo = 0, hi = num_triangles;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= s) lo = mid; else hi = mid;
    }
    const int4 r0 = record[4 * (int64_t)lo + 0], r1 = record[4 * (int64_t)lo + 1];
    const int4 r2 = record[4 * (int64_t)lo + 2];
    const int box_width = r2.w - r2.y + 1;
    const int64_t k = s - offsets[lo];
    // a record that does not belong to the offsets must not index outside the image
    if (box_width < 1 || k < 0 || k >= ((int64_t)1 << 28)) return;
    const int px = r2.y + (int)k % box_width, py = r2.z + (int)k / box_width;
    if ((unsigned)px >= (unsigned)width || (unsigned)py >= (unsigned)height) return;

    const RasterTerms t = raster_terms(r0, r1, r2.x, px, py);
    if (!t.covered) return;
    // finite and > 0: the bits of such an f32 order as the values do
    if (!(t.depth_w > 0.0f && t.depth_w < __builtin_inff())) return;
    const unsigned long long key =
        ((unsigned long long)(unsigned)__float_as_int(t.depth_w) << 32) | (unsigned)lo;
    unsigned long long* cell = zbuf + ((int64_t)py * width + px);
    // (a stale value is only ever larger than the current one: the atomic then runs and decides)
    if (*cell <= key) return;
    atomicMin(cell, key);
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_raster_resolve_kernel(const unsigned long long* __restrict__ zbuf,
                           const int4* __restrict__ record, const float* __restrict__ vertices,
                           int num_vertices, const int* __restrict__ triangles, int num_triangles,
                           const float* __restrict__ vertex_colors, const float* __restrict__ uvs,
                           const uint8_t* __restrict__ texture, int tex_height, int tex_width,
                           int tex_channels, RasterVec3 eye, RasterVec3 background, int width,
                           int height, float* __restrict__ color, float* __restrict__ alpha,
                           float* __restrict__ depth, int* __restrict__ ids) {
    const int pixel = blockIdx.x * kRasterThreads + threadIdx.x;     // W H <= 2^28
    if (pixel >= width * height) return;
    const unsigned long long key = zbuf[pixel];
    const unsigned f = (unsigned)key;
    if (key == kRasterEmpty || f >= (unsigned)num_triangles) {
#pragma unroll
        for (int j = 0; j < 3; ++j) color[3 * (int64_t)pixel + j] = background.v[j];
        alpha[pixel] = 0.0f;
        depth[pixel] = 0.0f;
        ids[pixel] = -1;
        return;
    }
    const int px = pixel % width, py = pixel / width;
    const int4 r0 = record[4 * (int64_t)f + 0], r1 = record[4 * (int64_t)f + 1];
    const int4 r2 = record[4 * (int64_t)f + 2];
    const RasterTerms t = raster_terms(r0, r1, r2.x, px, py);
    const float b0 = t.q0 * t.depth_w, b1 = t.q1 * t.depth_w, b2 = t.q2 * t.depth_w;

    const int last_vertex = num_vertices - 1;
    const int64_t v0 = min(max(triangles[3 * (int64_t)f + 0], 0), last_vertex);
    const int64_t v1 = min(max(triangles[3 * (int64_t)f + 1], 0), last_vertex);
    const int64_t v2 = min(max(triangles[3 * (int64_t)f + 2], 0), last_vertex);
    float d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float p = (vertices[3 * v0 + j] * b0 + vertices[3 * v1 + j] * b1)
                        + vertices[3 * v2 + j] * b2;
        d[j] = p - eye.v[j];
    }
    depth[pixel] = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    alpha[pixel] = 1.0f;
    ids[pixel] = (int)f;
    if (vertex_colors) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            color[3 * (int64_t)pixel + j] =
                (vertex_colors[3 * v0 + j] * b0 + vertex_colors[3 * v1 + j] * b1)
                + vertex_colors[3 * v2 + j] * b2;
    } else {
        const float u = (uvs[2 * v0 + 0] * b0 + uvs[2 * v1 + 0] * b1) + uvs[2 * v2 + 0] * b2;
        const float v = (uvs[2 * v0 + 1] * b0 + uvs[2 * v1 + 1] * b1) + uvs[2 * v2 + 1] * b2;
        mesh_texture_lookup(u, v, texture, tex_height, tex_width, tex_channels,
                            color + 3 * (int64_t)pixel);
    }
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_raster_setup(const float* vertices, int64_t num_vertices,
                                     const int32_t* triangles, int64_t num_triangles,
                                     const float* proj, int width, int height, int32_t* record,
                                     uint8_t* status, int64_t* counts, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_raster_setup: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (raster_bad_image(width, height))
        return fail_arg("ffn_mesh_raster_setup: image (1 <= width, height <= 16384)");
    if (!vertices || !triangles || !proj || !record || !status || !counts)
        return fail_arg("ffn_mesh_raster_setup: null argument");
    if (((uintptr_t)record & 15) != 0)
        return fail_arg("ffn_mesh_raster_setup: record must be 16-byte aligned");
    RasterMatrix m;
    for (int i = 0; i < 12; ++i) m.p[i] = proj[i];
    const unsigned blocks = (unsigned)((num_triangles + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_raster_setup_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, vertices, (int)num_vertices, triangles,
                       (int)num_triangles, m, width, height, (int4*)record, status, counts);
    return check_launch("ffn_mesh_raster_setup");
}

extern "C" int ffn_mesh_raster_draw(const int32_t* record, const int64_t* offsets,
                                    int64_t num_triangles, int64_t first, int64_t count, int width,
                                    int height, uint64_t* zbuf, void* stream) {
    if (num_triangles < 1 || num_triangles > 0x7fffffff / 3)
        return fail_arg("ffn_mesh_raster_draw: shape (1 <= num_triangles <= (2^31 - 1) / 3)");
    if (count < 1 || count > ffn_octree_max_points() || first < 0)
        return fail_arg("ffn_mesh_raster_draw: chunk (first >= 0, 1 <= count < 2^31)");
    if (raster_bad_image(width, height))
        return fail_arg("ffn_mesh_raster_draw: image (1 <= width, height <= 16384)");
    if (!record || !offsets || !zbuf)
        return fail_arg("ffn_mesh_raster_draw: null argument");
    if (((uintptr_t)record & 15) != 0 || ((uintptr_t)zbuf & 7) != 0)
        return fail_arg("ffn_mesh_raster_draw: record must be 16-byte, zbuf 8-byte aligned");
    const unsigned blocks = (unsigned)((count + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_raster_draw_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)record, offsets, (int)num_triangles,
                       first, count, width, height, (unsigned long long*)zbuf);
    return check_launch("ffn_mesh_raster_draw");
}

extern "C" int ffn_mesh_raster_resolve(const uint64_t* zbuf, const int32_t* record,
                                       const float* vertices, int64_t num_vertices,
                                       const int32_t* triangles, int64_t num_triangles,
                                       const float* vertex_colors, const float* uvs,
                                       const uint8_t* texture, int tex_height, int tex_width,
                                       int tex_channels, const float* eye, const float* background,
                                       int width, int height, float* color, float* alpha,
                                       float* depth, int32_t* ids, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_raster_resolve: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (raster_bad_image(width, height))
        return fail_arg("ffn_mesh_raster_resolve: image (1 <= width, height <= 16384)");
    if (!zbuf || !record || !vertices || !triangles || !eye || !background || !color || !alpha ||
        !depth || !ids)
        return fail_arg("ffn_mesh_raster_resolve: null argument");
    if ((vertex_colors != nullptr) == (uvs != nullptr || texture != nullptr) ||
        (uvs != nullptr) != (texture != nullptr))
        return fail_arg("ffn_mesh_raster_resolve: either vertex_colors, or uvs and texture");
    if (texture && (tex_height < 1 || tex_width < 1 || tex_channels < 3 ||
                    tex_height > (1 << 24) || tex_width > (1 << 24) ||
                    (int64_t)tex_height * tex_width > 0x7fffffff / tex_channels))
        return fail_arg("ffn_mesh_raster_resolve: texture (1 <= height, width <= 2^24, "
                        "channels >= 3, fewer than 2^31 bytes)");
    if (((uintptr_t)record & 15) != 0 || ((uintptr_t)zbuf & 7) != 0)
        return fail_arg("ffn_mesh_raster_resolve: record must be 16-byte, zbuf 8-byte aligned");
    RasterVec3 e, b;
    for (int i = 0; i < 3; ++i) e.v[i] = eye[i], b.v[i] = background[i];
    const unsigned blocks = (unsigned)(((int64_t)width * height + kRasterThreads - 1) /
                                       kRasterThreads);
    hipLaunchKernelGGL(mesh_raster_resolve_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const unsigned long long*)zbuf, (const int4*)record,
                       vertices, (int)num_vertices, triangles, (int)num_triangles, vertex_colors,
                       uvs, texture, tex_height, tex_width, tex_channels, e, b, width, height,
                       color, alpha, depth, ids);
    return check_launch("ffn_mesh_raster_resolve");
}
