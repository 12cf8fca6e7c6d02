// K32  The adjoint of K31's colour interpolation: per-vertex sums of b_i * g[p] over the pixels
// every triangle wins, and of b_i alone.  With g the gradient of a loss it is the gradient of the
// vertex colours (fit_mesh_colors); with g an image it is, divided by the sum of b_i, the mean
// colour of the cameras that see a vertex (color_mesh_from_images).  Geometry gets no gradient and
// the textured path of K31 no backward.
//
// No reference counterpart.  K31 decides coverage on integers and its colour is
// (c_v0 b0 + c_v1 b1) + c_v2 b2 with b_i from the geometry alone, so the image is a linear map of
// the vertex colours and this is its transpose.  No float atomics, no LDS: every sum has one fixed
// order, the same bits on every call, and a numpy-f32 restatement gives the same bits (this file is
// compiled with -ffp-contract=off).
//
//   K32a face sums, one wavefront of 64 lanes per triangle f (grid-stride over triangles).  The box
//        x0 y0 x1 y1 of record[f] (K31a), bw = x1 - x0 + 1, n = bw (y1 - y0 + 1); a box that is
//        empty, not inside the image or of more than 2^28 pixels contributes nothing, so a bad
//        record never indexes outside the image.  Box pixel k is (x0 + k % bw, y0 + k / bw); it is
//        selected iff ids[py W + px] == f (ids is compared, never an index).  A pixel that is not
//        selected is skipped: its d_color is not read.  A selected pixel has raster_terms() (the
//        bits of K31c), b_i = q_i * depth_w and the twelve terms t[3i+j] = b_i * d_color[p][j],
//        t[9+i] = b_i.  Segment s holds k = 64 s + lane; lanes not selected or past n hold +0.0f;
//        the 64 values are folded by x += __shfl_xor(x, off), off = 32 .. 1 (an IEEE add commutes
//        bit for bit: the fold of halves), and acc = acc + segment in the order of s from 0.0f.
//        face_sums[f] = the twelve acc; every row is written.
//   K32b vertex gather, one thread per vertex v.  corner_order (3F,) holds the corners 3f + i
//        stably sorted by vertex, vertex_starts (V+1,) their CSR rows.  From 0.0f and in that order
//        g[j] = g[j] + face_sums[f][3i+j], w = w + face_sums[f][9+i]; a corner outside [0, 3F) is
//        skipped.  grad[v] = g, weight[v] = w, or out = out + value with accumulate.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   mesh_raster_face_sums_kernel  50 VGPRs, 64 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of
//                                 LDS, occupancy 8 waves per SIMD; the butterfly is 72
//                                 ds_bpermute_b32 per segment (12 values, 6 steps), the adds are
//                                 v_add_f32 / v_pk_add_f32, no fma
//   mesh_vertex_gather_kernel     20 VGPRs, 24 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of
//                                 LDS, occupancy 8
// The three K31 kernels compile to the instructions they had before raster_terms() and the
// constants moved into mesh_raster_terms.h: the gfx950 disassemblies of mesh_raster.hip before
// and after differ in the compilation-unit id alone.
//
// Not done: a work split for a screen-filling triangle (it is a loop over ceil(n / 64) segments in
// one wave; a split would have to keep these bits), and a vertex of huge valence (K32b's loop is
// linear in the valence, which is fine for the meshes of OcTree.extract_mesh).  "No LDS" is
// true of the allocation, not of the data path: the butterfly's ds_bpermute_b32 goes through the
// LDS crossbar.  DPP or v_permlane forms of the same adds would keep the bits; they are not
// written, and would matter only where a screen-filling triangle does.
#include "common.h"
#include "mesh_raster_terms.h"

namespace ffn {

constexpr int kGradWave = 64;
constexpr int kGradWavesPerBlock = kRasterThreads / kGradWave;
constexpr int kGradMaxBlocks = 1 << 16;
constexpr int64_t kGradMaxBox = (int64_t)1 << 28;

__device__ __forceinline__ float wave_fold(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, kGradWave);
    return x;
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_raster_face_sums_kernel(const int4* __restrict__ record, const int* __restrict__ ids,
                             const float* __restrict__ d_color, int num_triangles, int width,
                             int height, float* __restrict__ face_sums) {
    const int lane = threadIdx.x & (kGradWave - 1);
    // (the wave's number is the same in all of its lanes: say so, the loops below are uniform)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kGradWave);
    const int stride = gridDim.x * kGradWavesPerBlock;
    for (int f = blockIdx.x * kGradWavesPerBlock + wave; f < num_triangles; f += stride) {
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
        if (n > kGradMaxBox) n = 0;
        const int count = (int)n;

        float acc[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[c] = 0.0f;
        for (int first = 0; first < count; first += kGradWave) {
            float t[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) t[c] = 0.0f;
            const int k = first + lane;
            if (k < count) {
                const int px = x0 + k % box_width, py = y0 + k / box_width;
                const int pixel = py * width + px;                   // inside the image: < 2^28
                if (ids[pixel] == f) {
                    const RasterTerms terms = raster_terms(r0, r1, r2.x, px, py);
                    const float b[3] = {terms.q0 * terms.depth_w, terms.q1 * terms.depth_w,
                                        terms.q2 * terms.depth_w};
                    float g[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) g[j] = d_color[3 * (int64_t)pixel + j];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) t[3 * i + j] = b[i] * g[j];
                        t[9 + i] = b[i];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 12; ++c) acc[c] = acc[c] + wave_fold(t[c]);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 12; ++c) face_sums[12 * (int64_t)f + c] = acc[c];
        }
    }
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_vertex_gather_kernel(const float* __restrict__ face_sums, const int* __restrict__ corner_order,
                          const int* __restrict__ vertex_starts, int num_corners, int num_vertices,
                          int accumulate, float* __restrict__ grad, float* __restrict__ weight) {
    const int v = blockIdx.x * kRasterThreads + threadIdx.x;
    if (v >= num_vertices) return;
    // rows that are not a CSR of corner_order must not read outside it
    const int begin = max(vertex_starts[v], 0), end = min(vertex_starts[v + 1], num_corners);
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, w = 0.0f;
    for (int at = begin; at < end; ++at) {
        const int corner = corner_order[at];
        if ((unsigned)corner >= (unsigned)num_corners) continue;
        const int f = corner / 3, i = corner - 3 * f;
        const float* row = face_sums + 12 * (int64_t)f;
        g0 = g0 + row[3 * i + 0];
        g1 = g1 + row[3 * i + 1];
        g2 = g2 + row[3 * i + 2];
        w = w + row[9 + i];
    }
    float* out = grad + 3 * (int64_t)v;
    if (accumulate) {
        out[0] = out[0] + g0;
        out[1] = out[1] + g1;
        out[2] = out[2] + g2;
        weight[v] = weight[v] + w;
    } else {
        out[0] = g0;
        out[1] = g1;
        out[2] = g2;
        weight[v] = w;
    }
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_raster_face_sums(const int32_t* record, const int32_t* ids,
                                         const float* d_color, int64_t num_triangles, int width,
                                         int height, float* face_sums, void* stream) {
    if (num_triangles < 1 || num_triangles > 0x7fffffff / 3)
        return fail_arg("ffn_mesh_raster_face_sums: shape (1 <= num_triangles <= (2^31 - 1) / 3)");
    if (raster_bad_image(width, height))
        return fail_arg("ffn_mesh_raster_face_sums: image (1 <= width, height <= 16384)");
    if (!record || !ids || !d_color || !face_sums)
        return fail_arg("ffn_mesh_raster_face_sums: null argument");
    if (((uintptr_t)record & 15) != 0)
        return fail_arg("ffn_mesh_raster_face_sums: record must be 16-byte aligned");
    const int64_t wanted = (num_triangles + kGradWavesPerBlock - 1) / kGradWavesPerBlock;
    const unsigned blocks = (unsigned)(wanted < kGradMaxBlocks ? wanted : kGradMaxBlocks);
    hipLaunchKernelGGL(mesh_raster_face_sums_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)record, ids, d_color, (int)num_triangles,
                       width, height, face_sums);
    return check_launch("ffn_mesh_raster_face_sums");
}

extern "C" int ffn_mesh_vertex_gather(const float* face_sums, const int32_t* corner_order,
                                      const int32_t* vertex_starts, int64_t num_triangles,
                                      int64_t num_vertices, float* grad, float* weight,
                                      int accumulate, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_vertex_gather: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (!face_sums || !corner_order || !vertex_starts || !grad || !weight)
        return fail_arg("ffn_mesh_vertex_gather: null argument");
    const unsigned blocks = (unsigned)((num_vertices + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_vertex_gather_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, face_sums, corner_order, vertex_starts,
                       (int)(3 * num_triangles), (int)num_vertices, accumulate, grad, weight);
    return check_launch("ffn_mesh_vertex_gather");
}
