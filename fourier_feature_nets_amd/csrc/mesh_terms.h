// The bilinear texture lookup of K22 (mesh.hip), shared with K31c (mesh_raster.hip): the
// reference's interpolate_bilinear (utils.py:197-241) followed by the / 255 of octree.py:849.
// Every operation is one rounded f32 operation in the order written; every including file is
// compiled with -ffp-contract=off.  mesh_texture_taps() is the same lookup without the texture, for
// K33a (mesh_texture.hip).
#pragma once
#include "common.h"

namespace ffn {

// float index of a texel row or column, clamped to [0, last]; NaN clamps to 0.  Clamping the
// float keeps the conversion defined for any finite or infinite coordinate; below 2^24 it is the
// integer clamp of the reference.
__device__ __forceinline__ int mesh_clamp_index(float index, float last) {
    return (int)fminf(fmaxf(index, 0.0f), last);
}

// rgb[0..2] = the texture at (u, v), row index growing with v, channels 0..2, in [0, 1].
// col = u W, row = v H; j0 = floor(col), i0 = floor(row); dj = col - j0, di = row - i0 BEFORE the
// indices are clamped to the image; ((w00 t00 + w01 t01) + w10 t10) + w11 t11, then / 255.
__device__ __forceinline__ void mesh_texture_lookup(float u, float v,
                                                    const uint8_t* __restrict__ texture,
                                                    int height, int width, int channels,
                                                    float* __restrict__ rgb) {
    const float col = u * (float)width, row = v * (float)height;
    const float fj = floorf(col), fi = floorf(row);
    const float dj = col - fj, di = row - fi;
    const float last_col = (float)(width - 1), last_row = (float)(height - 1);
    const int j0 = mesh_clamp_index(fj, last_col), j1 = mesh_clamp_index(fj + 1.0f, last_col);
    const int i0 = mesh_clamp_index(fi, last_row), i1 = mesh_clamp_index(fi + 1.0f, last_row);
    const float w00 = (1.0f - di) * (1.0f - dj), w01 = (1.0f - di) * dj;
    const float w10 = di * (1.0f - dj), w11 = di * dj;
    const uint8_t* t00 = texture + ((int64_t)i0 * width + j0) * channels;
    const uint8_t* t01 = texture + ((int64_t)i0 * width + j1) * channels;
    const uint8_t* t10 = texture + ((int64_t)i1 * width + j0) * channels;
    const uint8_t* t11 = texture + ((int64_t)i1 * width + j1) * channels;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float sum = ((w00 * (float)t00[ch] + w01 * (float)t01[ch]) + w10 * (float)t10[ch])
                          + w11 * (float)t11[ch];
        rgb[ch] = sum / 255.0f;
    }
}

// The four texels and weights mesh_texture_lookup blends at (u, v), without the texture: the same
// operations in the same order, so the same bits (K33a, mesh_texture.hip).  texel[k] = i width + j
// and weight[k] in the order 00, 01, 10, 11; height width < 2^31.
struct MeshTextureTaps {
    int texel[4];
    float weight[4];
};

__device__ __forceinline__ MeshTextureTaps mesh_texture_taps(float u, float v, int height,
                                                             int width) {
    const float col = u * (float)width, row = v * (float)height;
    const float fj = floorf(col), fi = floorf(row);
    const float dj = col - fj, di = row - fi;
    const float last_col = (float)(width - 1), last_row = (float)(height - 1);
    const int j0 = mesh_clamp_index(fj, last_col), j1 = mesh_clamp_index(fj + 1.0f, last_col);
    const int i0 = mesh_clamp_index(fi, last_row), i1 = mesh_clamp_index(fi + 1.0f, last_row);
    MeshTextureTaps t;
    t.weight[0] = (1.0f - di) * (1.0f - dj), t.weight[1] = (1.0f - di) * dj;
    t.weight[2] = di * (1.0f - dj), t.weight[3] = di * dj;
    t.texel[0] = i0 * width + j0, t.texel[1] = i0 * width + j1;
    t.texel[2] = i1 * width + j0, t.texel[3] = i1 * width + j1;
    return t;
}

}  // namespace ffn
