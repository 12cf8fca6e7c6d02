// What csrc/octree_walk.hip (K17a and K19a, the gradient walks) offers csrc/octree_grad.hip (K17b,
// K19b).
#pragma once
#include "common.h"

namespace ffn {

// phase 0: ray_slots[r] = taken leaves of ray r, ray_color / ray_trans its C and T_{n+1}.
// phase 1: ray_slots holds the n + 1 exclusive offsets; entry k of ray r goes to
//          entry_values / entry_leaves[ray_slots[r] + k].
int octree_grad_walk(const char* who, const float* starts, const float* directions, int64_t n,
                     float scale, int depth, const int64_t* node_index, int64_t num_nodes,
                     const int64_t* leaf_index, int64_t num_leaves, float t_min,
                     const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
                     float min_transmittance, const float* d_color, const float* d_alpha,
                     int32_t* ray_slots, float* ray_color, float* ray_trans, float4* entry_values,
                     int32_t* entry_leaves, int phase, hipStream_t stream);

// K19a: as octree_grad_walk on the SH rows of K18a (leaf_rows, row_stride floats per row, degree 1 or
// 2).  An entry's float4 is (e_r, e_g, e_b, d sigma) and phase 1 also writes its ray's number to
// entry_rays[ray_slots[r] + k].
int octree_grad_sh_walk(const char* who, const float* starts, const float* directions, int64_t n,
                        float scale, int depth, const int64_t* node_index, int64_t num_nodes,
                        const int64_t* leaf_index, int64_t num_leaves, float t_min,
                        const float* leaf_rows, int row_stride, int degree, float bg_r, float bg_g,
                        float bg_b, float min_transmittance, const float* d_color,
                        const float* d_alpha, int32_t* ray_slots, float* ray_color,
                        float* ray_trans, float4* entry_values, int32_t* entry_leaves,
                        int32_t* entry_rays, int phase, hipStream_t stream);

int octree_check_walk_args(const char* who, const float* starts, const float* directions,
                           int64_t n, int depth, const int64_t* node_index, int64_t num_nodes,
                           const int64_t* leaf_index, int64_t num_leaves);

}  // namespace ffn
