// K33  K31c's textured colour as a sparse matrix, and both of its products: the picture of a
// textured mesh is a linear map of the texture, with four entries per covered pixel that depend on
// the geometry, the camera and the UVs alone.  K33a makes the entries (the taps), K33b applies the
// matrix to a float texture (the forward of a fit) and K33c its transpose to an image (the gradient
// of the texels, or with an image for input the weighted sum of the pixels that see a texel).
//
// No reference counterpart.  No float atomics, no LDS: every sum has one fixed order, the same bits
// on every call, and a numpy-f32 restatement gives the same bits (this file is compiled with
// -ffp-contract=off).  Every index read from an input array is held against its range before it is
// used (K20's rule): foreign ids, taps or orders give wrong numbers, never an access outside the
// buffers.
//
//   K33a taps, one thread per pixel p.  f = ids[p] (K31c); outside 0 .. F-1 the pixel is uncovered:
//        tap_texel[p] = -1 -1 -1 -1, tap_weight[p] = +0 four times.  Else raster_terms() of
//        record[f] (the bits of K31c), b_i = q_i * depth_w, the vertex ids clamped into 0 .. V-1,
//        u = (u0 b0 + u1 b1) + u2 b2 and v likewise, then mesh_texture_taps() of mesh_terms.h: the
//        index and weight arithmetic of mesh_texture_lookup.  tap_texel[p][k] = i width + j and
//        tap_weight[p][k] in the order 00, 01, 10, 11.
//   K33b forward gather, one thread per pixel.  tap_texel[p][0] < 0: background, alpha 0.  Else
//        term_k = tap_weight[p][k] * texture[tap_texel[p][k]][ch], or +0.0f by selection for a texel
//        outside 0 .. T-1; color[p][ch] = ((term_0 + term_1) + term_2) + term_3, alpha 1.
//   K33c transposed gather, one thread per texel t.  sorted_texels (N) and tap_order (N) are the
//        N = 4 P tap slots 4 p + k stably sorted by tap_texel (made by the caller).  The row of t is
//        [lower_bound(t), lower_bound(t + 1)) of sorted_texels.  From 0.0f and in that order, for
//        s = tap_order[at], w = tap_weight[s]: skipped by selection when s is outside 0 .. N-1 or
//        !(w > 0.0f) (a NaN weight, or a zero weight over a non-finite d_color, reaches no texel);
//        else g[ch] = g[ch] + w * d_color[s / 4][ch], wsum = wsum + w.  grad[t] = g,
//        weight[t] = wsum, or out = out + value with accumulate (K32b's convention).
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   mesh_texture_taps_kernel    41 VGPRs, 24 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8 waves per SIMD
//   mesh_texture_gather_kernel  21 VGPRs, 19 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8
//   mesh_texture_grad_kernel    17 VGPRs, 26 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
//                               occupancy 8
//
// Not done: a split of long texel rows.  K33c's loop is linear in the row length: fine for an
// atlas, where every texel gets a few taps, slow for a heavily minified texture, where one texel
// gets the whole image.  A split would have to keep these bits.
#include "common.h"
#include "mesh_terms.h"
#include "mesh_raster_terms.h"

namespace ffn {

constexpr int64_t kTextureMaxTexels = 0x7fffffff / 3;        // 3 T floats index in an int
constexpr int64_t kTextureMaxPixels = (int64_t)1 << 28;      // 4 P tap slots index in an int

struct TextureVec3 {
    float v[3];
};

__global__ void __launch_bounds__(kRasterThreads)
mesh_texture_taps_kernel(const int4* __restrict__ record, const int* __restrict__ ids,
                         const int* __restrict__ triangles, int num_triangles,
                         const float* __restrict__ uvs, int num_vertices, int tex_height,
                         int tex_width, int width, int height, int4* __restrict__ tap_texel,
                         float4* __restrict__ tap_weight) {
    const int pixel = blockIdx.x * kRasterThreads + threadIdx.x;     // W H <= 2^28
    if (pixel >= width * height) return;
    const int f = ids[pixel];
    if ((unsigned)f >= (unsigned)num_triangles) {
        tap_texel[pixel] = make_int4(-1, -1, -1, -1);
        tap_weight[pixel] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
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
    const float u = (uvs[2 * v0 + 0] * b0 + uvs[2 * v1 + 0] * b1) + uvs[2 * v2 + 0] * b2;
    const float v = (uvs[2 * v0 + 1] * b0 + uvs[2 * v1 + 1] * b1) + uvs[2 * v2 + 1] * b2;
    const MeshTextureTaps taps = mesh_texture_taps(u, v, tex_height, tex_width);
    tap_texel[pixel] = make_int4(taps.texel[0], taps.texel[1], taps.texel[2], taps.texel[3]);
    tap_weight[pixel] = make_float4(taps.weight[0], taps.weight[1], taps.weight[2],
                                    taps.weight[3]);
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_texture_gather_kernel(const int4* __restrict__ tap_texel,
                           const float4* __restrict__ tap_weight,
                           const float* __restrict__ texture, int num_texels,
                           TextureVec3 background, int num_pixels, float* __restrict__ color,
                           float* __restrict__ alpha) {
    const int pixel = blockIdx.x * kRasterThreads + threadIdx.x;
    if (pixel >= num_pixels) return;
    const int4 texel = tap_texel[pixel];
    float* out = color + 3 * (int64_t)pixel;
    if (texel.x < 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = background.v[ch];
        alpha[pixel] = 0.0f;
        return;
    }
    const float4 w = tap_weight[pixel];
    const int at[4] = {texel.x, texel.y, texel.z, texel.w};
    const float weight[4] = {w.x, w.y, w.z, w.w};
    float term[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // a texel that does not belong to the texture is not read
        const bool inside = (unsigned)at[k] < (unsigned)num_texels;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            term[k][ch] = inside ? weight[k] * texture[3 * (int64_t)at[k] + ch] : 0.0f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        out[ch] = ((term[0][ch] + term[1][ch]) + term[2][ch]) + term[3][ch];
    alpha[pixel] = 1.0f;
}

// the first position in the ascending texels[0 .. n) that holds key or more (K30's search)
__device__ __forceinline__ int texture_lower_bound(const int* __restrict__ texels, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (texels[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_texture_grad_kernel(const int* __restrict__ sorted_texels, const int* __restrict__ tap_order,
                         const float* __restrict__ tap_weight, const float* __restrict__ d_color,
                         int num_slots, int num_texels, int accumulate, float* __restrict__ grad,
                         float* __restrict__ weight) {
    const int t = blockIdx.x * kRasterThreads + threadIdx.x;        // T <= (2^31 - 1) / 3
    if (t >= num_texels) return;
    // both ends lie in 0 .. N whatever sorted_texels holds
    const int begin = texture_lower_bound(sorted_texels, num_slots, t);
    const int end = texture_lower_bound(sorted_texels, num_slots, t + 1);
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, wsum = 0.0f;
    for (int at = begin; at < end; ++at) {
        const int s = tap_order[at];
        if ((unsigned)s >= (unsigned)num_slots) continue;
        const float w = tap_weight[s];
        if (!(w > 0.0f)) continue;
        const float* g = d_color + 3 * (int64_t)(s >> 2);
        g0 = g0 + w * g[0];
        g1 = g1 + w * g[1];
        g2 = g2 + w * g[2];
        wsum = wsum + w;
    }
    float* out = grad + 3 * (int64_t)t;
    if (accumulate) {
        out[0] = out[0] + g0;
        out[1] = out[1] + g1;
        out[2] = out[2] + g2;
        weight[t] = weight[t] + wsum;
    } else {
        out[0] = g0;
        out[1] = g1;
        out[2] = g2;
        weight[t] = wsum;
    }
}

static inline bool texture_bad_size(int tex_height, int tex_width) {
    return tex_height < 1 || tex_width < 1 || tex_height > (1 << 24) || tex_width > (1 << 24) ||
           (int64_t)tex_height * tex_width > kTextureMaxTexels;
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_texture_taps(const int32_t* record, const int32_t* ids,
                                     const int32_t* triangles, int64_t num_triangles,
                                     const float* uvs, int64_t num_vertices, int tex_height,
                                     int tex_width, int width, int height, int32_t* tap_texel,
                                     float* tap_weight, void* stream) {
    if (raster_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_texture_taps: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (raster_bad_image(width, height))
        return fail_arg("ffn_mesh_texture_taps: image (1 <= width, height <= 16384)");
    if (texture_bad_size(tex_height, tex_width))
        return fail_arg("ffn_mesh_texture_taps: texture (1 <= height, width <= 2^24, at most "
                        "(2^31 - 1) / 3 texels)");
    if (!record || !ids || !triangles || !uvs || !tap_texel || !tap_weight)
        return fail_arg("ffn_mesh_texture_taps: null argument");
    if ((((uintptr_t)record | (uintptr_t)tap_texel | (uintptr_t)tap_weight) & 15) != 0)
        return fail_arg("ffn_mesh_texture_taps: record, tap_texel and tap_weight must be 16-byte "
                        "aligned");
    const unsigned blocks = (unsigned)(((int64_t)width * height + kRasterThreads - 1) /
                                       kRasterThreads);
    hipLaunchKernelGGL(mesh_texture_taps_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)record, ids, triangles,
                       (int)num_triangles, uvs, (int)num_vertices, tex_height, tex_width, width,
                       height, (int4*)tap_texel, (float4*)tap_weight);
    return check_launch("ffn_mesh_texture_taps");
}

extern "C" int ffn_mesh_texture_gather(const int32_t* tap_texel, const float* tap_weight,
                                       const float* texture, int64_t num_texels,
                                       const float* background, int64_t num_pixels, float* color,
                                       float* alpha, void* stream) {
    if (num_pixels < 1 || num_pixels > kTextureMaxPixels)
        return fail_arg("ffn_mesh_texture_gather: shape (1 <= num_pixels <= 2^28)");
    if (num_texels < 1 || num_texels > kTextureMaxTexels)
        return fail_arg("ffn_mesh_texture_gather: texture (1 <= num_texels <= (2^31 - 1) / 3)");
    if (!tap_texel || !tap_weight || !texture || !background || !color || !alpha)
        return fail_arg("ffn_mesh_texture_gather: null argument");
    if ((((uintptr_t)tap_texel | (uintptr_t)tap_weight) & 15) != 0)
        return fail_arg("ffn_mesh_texture_gather: tap_texel and tap_weight must be 16-byte "
                        "aligned");
    TextureVec3 b;
    for (int i = 0; i < 3; ++i) b.v[i] = background[i];
    const unsigned blocks = (unsigned)((num_pixels + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_texture_gather_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, (const int4*)tap_texel, (const float4*)tap_weight,
                       texture, (int)num_texels, b, (int)num_pixels, color, alpha);
    return check_launch("ffn_mesh_texture_gather");
}

extern "C" int ffn_mesh_texture_grad(const int32_t* sorted_texels, const int32_t* tap_order,
                                     const float* tap_weight, const float* d_color,
                                     int64_t num_pixels, int64_t num_texels, float* grad,
                                     float* weight, int accumulate, void* stream) {
    if (num_pixels < 1 || num_pixels > kTextureMaxPixels)
        return fail_arg("ffn_mesh_texture_grad: shape (1 <= num_pixels <= 2^28)");
    if (num_texels < 1 || num_texels > kTextureMaxTexels)
        return fail_arg("ffn_mesh_texture_grad: texture (1 <= num_texels <= (2^31 - 1) / 3)");
    if (!sorted_texels || !tap_order || !tap_weight || !d_color || !grad || !weight)
        return fail_arg("ffn_mesh_texture_grad: null argument");
    const unsigned blocks = (unsigned)((num_texels + kRasterThreads - 1) / kRasterThreads);
    hipLaunchKernelGGL(mesh_texture_grad_kernel, dim3(blocks), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, sorted_texels, tap_order, tap_weight, d_color,
                       (int)(4 * num_pixels), (int)num_texels, accumulate, grad, weight);
    return check_launch("ffn_mesh_texture_grad");
}
