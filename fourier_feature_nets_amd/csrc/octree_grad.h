// What csrc/octree_walk.hip (K13 .. K19a, the walks) and csrc/octree_grad.hip (K17b, K19b) share on
// the host.
#pragma once
#include "common.h"

namespace ffn {

// what every mode of the walk takes (t_min: 0 for the path form, which has none)
struct Walk {
    const float* starts;
    const float* directions;
    int64_t n;
    float scale;
    int depth;
    const int64_t* node_index;
    int64_t num_nodes;
    const int64_t* leaf_index;
    int64_t num_leaves;
    float t_min;
    hipStream_t stream;
};

// what a volume render and its backward composite: rows of `stride` floats, K15's (degree 0,
// [r, g, b, sigma, ...]) or the device layout of K18a (degree 1 or 2)
struct VolumeLeaves {
    const float* data;
    int stride;
    int degree;
    float bg_r, bg_g, bg_b;
    float min_transmittance;
};

// K17a / K19a: a volume walk, the upstream gradients and the buffers of the two phases.
// phase 0: ray_slots[r] = taken leaves of ray r, ray_color / ray_trans its C and T_{n+1}.
// phase 1: ray_slots holds the n + 1 exclusive offsets; entry k of ray r goes to
//          entry_values / entry_leaves[ray_slots[r] + k], a float4 (d rgb, d sigma) or, on SH rows,
//          (e_r, e_g, e_b, d sigma) with its ray's number in entry_rays (null at degree 0).
struct GradWalk {
    Walk walk;
    VolumeLeaves leaves;
    const float* d_color;
    const float* d_alpha;
    int32_t* ray_slots;
    float* ray_color;
    float* ray_trans;
    float4* entry_values;
    int32_t* entry_leaves;
    int32_t* entry_rays;
    // K29b (dist: the walk is one of the three modes with the distortion term): phase 0 also writes
    // ray_dist[3 r ..] = (W_tot, M_tot, D) and, where it is not null, ray_distortion[r] = D; phase 1
    // adds dist_scale * dD/dsigma_k to every entry's d sigma
    bool dist;
    float dist_scale;
    float* ray_dist;
    float* ray_distortion;
};

// launched by the backward entry points (csrc/octree_grad.hip), which have checked the arguments
int octree_grad_walk(const char* who, const GradWalk& grad, int phase);

inline int fail_who(const char* who, const char* what) {
    char text[200];
    snprintf(text, sizeof text, "%s: %s", who, what);
    return fail_arg(text);
}

inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

int check_walk_args(const char* who, const Walk& walk);

// what the volume renders and their backwards refuse alike, in this order: a NaN t_min,
// min_transmittance, null leaf data or `any_null` (the caller's other pointers), the walk arguments
int check_volume_args(const char* who, const Walk& walk, const VolumeLeaves& leaves, bool any_null);

}  // namespace ffn
