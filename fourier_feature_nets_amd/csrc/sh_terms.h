// The real SH basis of K18 / K19 at a ray's unit direction, shared by the walk (K18a, K19a:
// csrc/octree_walk.hip) and the wide reduce (K19b: csrc/octree_grad.hip) so that every user gets the
// same bits.  Both files are compiled with -ffp-contract=off: every product and sum below rounds on
// its own.
#pragma once
#include "common.h"

namespace ffn {

// the real SH basis of bands 0 .. kDegree at the unit vector (x, y, z), in the order and with the
// signs of include/ffn_hip.h
template <int kDegree>
__device__ __forceinline__ void sh_terms(float x, float y, float z,
                                         float (&basis)[(kDegree + 1) * (kDegree + 1)]) {
    basis[0] = 0.28209479177387814f;
    basis[1] = -0.4886025119029199f * y;
    basis[2] = 0.4886025119029199f * z;
    basis[3] = -0.4886025119029199f * x;
    if constexpr (kDegree >= 2) {
        basis[4] = 1.0925484305920792f * (x * y);
        basis[5] = -1.0925484305920792f * (y * z);
        basis[6] = 0.31539156525252005f * (2.0f * (z * z) - x * x - y * y);
        basis[7] = -1.0925484305920792f * (x * z);
        basis[8] = 0.5462742152960396f * (x * x - y * y);
    }
}

// world length per unit of t: the walk's own expression
__device__ __forceinline__ float ray_norm(float dx, float dy, float dz) {
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

// the basis at u = d / norm.  A direction without a length (zero, NaN) is a miss and takes no leaf;
// its basis is never read, and is kept finite anyway
template <int kDegree>
__device__ __forceinline__ void sh_ray_basis(float dx, float dy, float dz, float norm,
                                             float (&basis)[(kDegree + 1) * (kDegree + 1)]) {
    const float inv = norm > 0.0f && norm < __builtin_inff() ? 1.0f / norm : 0.0f;
    sh_terms<kDegree>(dx * inv, dy * inv, dz * inv, basis);
}

}  // namespace ffn
