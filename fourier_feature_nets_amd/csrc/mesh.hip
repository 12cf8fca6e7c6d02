// K22  Surface samples of a textured triangle mesh: the point cloud an octree is built from.
//
// Replaces the host-side (numba / numpy) sampler of the reference: octree.py:42-99 (Basu-Owen
// low-discrepancy points in the triangle from a base-4 van der Corput sequence), octree.py:102-136
// (barycentric interpolation of positions and UVs) and utils.py:197-241 (bilinear texture lookup),
// followed by the / 255 of octree.py:849.
//
// One thread per sample, nothing shared between threads: no atomics, no LDS, and the result of a
// sample depends on its number alone, not on the launch shape.  Every operation below is a single
// rounded f32 operation in a fixed order (this file is compiled with -ffp-contract=off, and the two
// divisions are IEEE divisions), so a numpy-f32 restatement gives the same bits.
//
//   triangle   f with offsets[f] <= s < offsets[f + 1] (binary search; empty triangles have
//              offsets[f] == offsets[f + 1] and are never found), k = s - offsets[f], n = k + 1
//   point      16 rounds of the Basu-Owen subdivision on the corners A = (1,0), B = (0,1),
//              C = (0,0), round i steered by the base-4 digit (n >> 2 i) & 3; all coordinates stay
//              multiples of 2^-16, so the rounds are exact.  p = ((A + B) + C) / 3,
//              (b0, b1, b2) = (p.x, p.y, 1 - (p.x + p.y))
//   interpolate  per component (x0 b0 + x1 b1) + x2 b2, every product and sum rounded
//   colour     col = u W, row = v H; j0 = floor(col), i0 = floor(row); dj = col - j0,
//              di = row - i0 BEFORE the indices are clamped to the image; four weights
//              (1 - di)(1 - dj), (1 - di) dj, di (1 - dj), di dj, each times its texel as f32;
//              ((v00 + v01) + v10) + v11, then / 255.  Channels 0..2.  (mesh_texture_lookup in
//              mesh_terms.h, which K31c shares)
#include "common.h"
#include "mesh_terms.h"

namespace ffn {

constexpr int kMeshThreads = 256;
constexpr int kMeshRounds = 16;

struct MeshPoint {
    float x, y;
};

__device__ __forceinline__ MeshPoint mesh_mid(MeshPoint a, MeshPoint b) {
    return {(a.x + b.x) * 0.5f, (a.y + b.y) * 0.5f};
}

__device__ __forceinline__ MeshPoint mesh_pick(int d, MeshPoint v0, MeshPoint v1, MeshPoint v2,
                                               MeshPoint v3) {
    const MeshPoint lo = d & 1 ? v1 : v0, hi = d & 1 ? v3 : v2;
    return d & 2 ? hi : lo;
}

__global__ void __launch_bounds__(kMeshThreads)
mesh_sample_kernel(const float* __restrict__ vertices, int num_vertices,
                   const int* __restrict__ triangles, int num_triangles,
                   const float* __restrict__ uvs, const int* __restrict__ offsets, int64_t n,
                   const uint8_t* __restrict__ texture, int height, int width, int channels,
                   float* __restrict__ positions, float* __restrict__ colors,
                   float* __restrict__ sample_uvs) {
    const int64_t s = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (s >= n) return;

    // offsets[lo] <= s < offsets[hi] throughout (offsets[0] = 0, offsets[num_triangles] = n)
    int lo = 0, hi = num_triangles;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)offsets[mid] <= s) lo = mid; else hi = mid;
    }
    const unsigned number = (unsigned)((int)s - offsets[lo]) + 1u;

    MeshPoint a = {1.0f, 0.0f}, b = {0.0f, 1.0f}, c = {0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < kMeshRounds; ++i) {
        const int d = (number >> (2 * i)) & 3;
        const MeshPoint ab = mesh_mid(a, b), ac = mesh_mid(a, c), bc = mesh_mid(b, c);
        const MeshPoint na = mesh_pick(d, bc, a, ab, ac);
        const MeshPoint nb = mesh_pick(d, ac, ab, b, bc);
        const MeshPoint nc = mesh_pick(d, ab, ac, bc, c);
        a = na, b = nb, c = nc;
    }
    const float b0 = ((a.x + b.x) + c.x) / 3.0f;
    const float b1 = ((a.y + b.y) + c.y) / 3.0f;
    const float b2 = 1.0f - (b0 + b1);

    // the ids are the caller's check; clamped here so that a bad one reads a wrong vertex and
    // never memory outside the arrays
    const int last_vertex = num_vertices - 1;
    const int v0 = min(max(triangles[3 * (int64_t)lo + 0], 0), last_vertex);
    const int v1 = min(max(triangles[3 * (int64_t)lo + 1], 0), last_vertex);
    const int v2 = min(max(triangles[3 * (int64_t)lo + 2], 0), last_vertex);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        positions[3 * s + j] = (vertices[3 * (int64_t)v0 + j] * b0 + vertices[3 * (int64_t)v1 + j] * b1)
                               + vertices[3 * (int64_t)v2 + j] * b2;
    const float u = (uvs[2 * (int64_t)v0 + 0] * b0 + uvs[2 * (int64_t)v1 + 0] * b1)
                    + uvs[2 * (int64_t)v2 + 0] * b2;
    const float v = (uvs[2 * (int64_t)v0 + 1] * b0 + uvs[2 * (int64_t)v1 + 1] * b1)
                    + uvs[2 * (int64_t)v2 + 1] * b2;
    if (sample_uvs) {
        sample_uvs[2 * s + 0] = u;
        sample_uvs[2 * s + 1] = v;
    }

    mesh_texture_lookup(u, v, texture, height, width, channels, colors + 3 * s);
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_sample(const float* vertices, int64_t num_vertices, const int32_t* triangles,
                               int64_t num_triangles, const float* uvs, const int32_t* offsets,
                               int64_t n, const uint8_t* texture, int height, int width,
                               int channels, float* positions, float* colors, float* sample_uvs,
                               void* stream) {
    const int64_t int_max = 0x7fffffff;
    if (n < 1 || n > ffn_octree_max_points() || num_vertices < 1 || num_vertices > int_max / 3 ||
        num_triangles < 1 || num_triangles > int_max / 3)
        return fail_arg("ffn_mesh_sample: shape (1 <= n < 2^31, 1 <= num_vertices, "
                        "1 <= num_triangles)");
    if (height < 1 || width < 1 || channels < 3 || height > (1 << 24) || width > (1 << 24) ||
        (int64_t)height * width > int_max / channels)
        return fail_arg("ffn_mesh_sample: texture (1 <= height, width <= 2^24, channels >= 3, "
                        "fewer than 2^31 bytes)");
    if (!vertices || !triangles || !uvs || !offsets || !texture || !positions || !colors)
        return fail_arg("ffn_mesh_sample: null argument");
    const unsigned blocks = (unsigned)((n + kMeshThreads - 1) / kMeshThreads);
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(blocks), dim3(kMeshThreads), 0, (hipStream_t)stream,
                       vertices, (int)num_vertices, triangles, (int)num_triangles, uvs, offsets, n,
                       texture, height, width, channels, positions, colors, sample_uvs);
    return check_launch("ffn_mesh_sample");
}
