// K36  Rays against a triangle mesh: a tree over the triangles, the nearest or the farthest hit of
// every ray, and the shading of the hits.  What K13/K14 are for octrees; no reference counterpart.
//
// A ray caster has no camera plane: a mesh can be seen from inside or from next to it (K31 refuses
// every triangle that reaches w <= 0), and any batch of rays can be asked, not only a pinhole's.
// Every float operation is one rounded f32 operation in the order written (this file is compiled
// with -ffp-contract=off; / is the IEEE division), so a numpy-f32 restatement gives the same bits;
// the contract is in include/ffn_hip.h (K36), restated in tests/mesh_cast_reference.py.
//
//   K36a boxes, one thread per triangle.  Vertex ids clamped into [0, V-1] (K22).  lo = min(a, b,
//        c) - pad, hi = max(a, b, c) + pad per axis; a triangle with a non-finite vertex gets the
//        EMPTY box lo = +inf, hi = -inf.  key: the 30-bit Morton code of the box centre on the
//        1024^3 grid the host gives (grid_lo, grid_scale); 2^30 for an empty box.
//        (the sort of key << 32 | f is torch's: plumbing, as in K12 and K30)
//   K36b tree, one thread per node of a level, one launch per level from the leaves up.  The tree
//        is the complete binary tree of `levels` levels, level l holding 2^l nodes from row
//        2^l - 1 (level-major): no pointers.  Leaf j is the min / max of the boxes of the triangles
//        order[j leaf_size .. (j+1) leaf_size - 1] that exist, a node above it of its two children;
//        a leaf past the last triangle is the empty box.
//   K36c cast, one lane per ray, templated on nearest / farthest.  Stackless: the walk is depth
//        first, left child first, on (level, index) alone; after a node is done, index + 1 with
//        its trailing zero bits stripped (one level up per bit) is the next node, and index + 1 ==
//        2^level ends the walk.  Every node is visited at most once and the loop is bounded by the
//        number of nodes.  A box is entered iff it is not empty, tn <= tf, tf > t_min and it can
//        still hold a better hit (tn <= t_best, or tf >= t_best in farthest mode; ties are let in,
//        they may go to a lower id).  A triangle is tested against its own padded box first and
//        then by Moeller-Trumbore; a hit has tn <= t <= tf for that box, which is what makes the
//        culling exact: the slab test is monotone operation by operation, so a box built by min /
//        max alone over other boxes has a [tn, tf] that contains theirs bit for bit.  The best hit
//        is the minimum of (t, f) (the maximum t, then the lower f), whatever the order visited.
//        No scratch, no LDS, no atomics.
//   K36d shade, one thread per ray.  b0 = (1 - u) - v, b1 = u, b2 = v; colour (c0 b0 + c1 b1) + c2
//        b2, or the UV interpolated the same way and put through K22's lookup (mesh_terms.h);
//        alpha 1, depth t.  A miss: the background, 0, 0 (as K31c).
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   mesh_cast_boxes_kernel        23 VGPRs, 20 SGPRs, occupancy 8 waves per SIMD
//   mesh_cast_tree_kernel         22 VGPRs, 18 SGPRs, occupancy 8
//   mesh_cast_kernel<nearest>     56 VGPRs, 54 SGPRs, occupancy 8
//   mesh_cast_kernel<farthest>    56 VGPRs, 54 SGPRs, occupancy 8
//   mesh_cast_shade_kernel        32 VGPRs, 25 SGPRs, occupancy 8
// all five: 0 bytes of scratch, 0 spills, 0 bytes of LDS; no atomic instruction in the file.
//
// Not done: gradients through the cast, a refit after the vertices move (build again), any-hit or
// counting queries, a surface-area or LBVH build, a near-child-first walk (the order is fixed).
#include "common.h"
#include "mesh_terms.h"

namespace ffn {

constexpr int kCastThreads = 256;
constexpr int kCastMaxLeaf = 64;
constexpr int kCastMaxLevels = 31;
constexpr int kCastEmptyKey = 1 << 30;

__device__ __forceinline__ unsigned cast_spread10(unsigned x) {
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ void __launch_bounds__(kCastThreads)
mesh_cast_boxes_kernel(const float* __restrict__ vertices, int num_vertices,
                       const int* __restrict__ triangles, int num_triangles, float pad,
                       float grid_x, float grid_y, float grid_z, float grid_scale,
                       float* __restrict__ boxes, int* __restrict__ keys) {
    const int f = blockIdx.x * kCastThreads + threadIdx.x;
    if (f >= num_triangles) return;
    const int last_vertex = num_vertices - 1;
    float lo[3], hi[3];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int64_t id = min(max(triangles[3 * (int64_t)f + i], 0), last_vertex);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float p = vertices[3 * id + j];
            finite &= fabsf(p) < __builtin_inff();
            lo[j] = i == 0 ? p : fminf(lo[j], p);
            hi[j] = i == 0 ? p : fmaxf(hi[j], p);
        }
    }
    const float grid[3] = {grid_x, grid_y, grid_z};
    unsigned q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        lo[j] = finite ? lo[j] - pad : __builtin_inff();
        hi[j] = finite ? hi[j] + pad : -__builtin_inff();
        const float centre = (lo[j] + hi[j]) * 0.5f;
        const float cell = (centre - grid[j]) * grid_scale;
        q[j] = (unsigned)(int)fminf(fmaxf(cell, 0.0f), 1023.0f);
        boxes[6 * (int64_t)f + j] = lo[j];
        boxes[6 * (int64_t)f + 3 + j] = hi[j];
    }
    const unsigned key = cast_spread10(q[0]) | (cast_spread10(q[1]) << 1) |
                         (cast_spread10(q[2]) << 2);
    keys[f] = finite ? (int)key : kCastEmptyKey;
}

// level < levels - 1: node j of the level from its children 2 j, 2 j + 1 of the next one;
// the last level: leaf j from the boxes of its triangles.  j < 2^level <= 2^30.
__global__ void __launch_bounds__(kCastThreads)
mesh_cast_tree_kernel(const float* __restrict__ boxes, const int* __restrict__ order,
                      int num_triangles, int leaf_size, int levels, int level,
                      float* __restrict__ nodes) {
    const unsigned j = blockIdx.x * kCastThreads + threadIdx.x;
    if (j >= (1u << level)) return;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    if (level == levels - 1) {
        const int64_t first = (int64_t)j * leaf_size;
        const int64_t end = min(first + leaf_size, (int64_t)num_triangles);
        for (int64_t p = first; p < end; ++p) {
            const int64_t f = min(max(order[p], 0), num_triangles - 1);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], boxes[6 * f + a]);
                hi[a] = fmaxf(hi[a], boxes[6 * f + 3 + a]);
            }
        }
    } else {
        const int64_t child = ((int64_t)2 << level) - 1 + 2 * (int64_t)j;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(nodes[6 * child + a], nodes[6 * (child + 1) + a]);
            hi[a] = fmaxf(nodes[6 * child + 3 + a], nodes[6 * (child + 1) + 3 + a]);
        }
    }
    const int64_t node = ((int64_t)1 << level) - 1 + j;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nodes[6 * node + a] = lo[a];
        nodes[6 * node + 3 + a] = hi[a];
    }
}

struct CastRay {
    float o[3], d[3], inv[3];
};

// The slab test of the contract -> is the box not empty and tn <= tf; tn and tf by reference.
// box: 6 floats, 8-byte aligned (rows of 24 bytes in an 8-byte aligned array).
__device__ __forceinline__ bool cast_slab(const float* __restrict__ box, const CastRay& ray,
                                          float& tn, float& tf) {
    const float2 b0 = ((const float2*)box)[0], b1 = ((const float2*)box)[1];
    const float2 b2 = ((const float2*)box)[2];
    const float lo[3] = {b0.x, b0.y, b1.x}, hi[3] = {b1.y, b2.x, b2.y};
    float near[3], far[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t0 = (lo[a] - ray.o[a]) * ray.inv[a];
        const float t1 = (hi[a] - ray.o[a]) * ray.inv[a];
        near[a] = fminf(t0, t1);
        far[a] = fmaxf(t0, t1);
    }
    tn = fmaxf(fmaxf(near[0], near[1]), near[2]);
    tf = fminf(fminf(far[0], far[1]), far[2]);
    return lo[0] <= hi[0] && tn <= tf;
}

template <bool kFarthest>
__global__ void __launch_bounds__(kCastThreads)
mesh_cast_kernel(const float* __restrict__ nodes, const float* __restrict__ boxes,
                 const int* __restrict__ order, const float* __restrict__ vertices,
                 int num_vertices, const int* __restrict__ triangles, int num_triangles,
                 int leaf_size, int levels, const float* __restrict__ starts,
                 const float* __restrict__ directions, int64_t num_rays, float t_min,
                 int* __restrict__ hit, float* __restrict__ t_out, float* __restrict__ u_out,
                 float* __restrict__ v_out) {
    const int64_t r = (int64_t)blockIdx.x * kCastThreads + threadIdx.x;
    if (r >= num_rays) return;
    CastRay ray;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ray.o[a] = starts[3 * r + a];
        ray.d[a] = directions[3 * r + a];
        ray.inv[a] = 1.0f / ray.d[a];
    }
    float best_t = kFarthest ? -__builtin_inff() : __builtin_inff();
    float best_u = 0.0f, best_v = 0.0f;
    int best_f = -1;
    const int last_vertex = num_vertices - 1;
    const unsigned leaf_level = (unsigned)(levels - 1);
    const unsigned num_nodes = (unsigned)(((int64_t)1 << levels) - 1);
    unsigned level = 0, index = 0;
    for (unsigned trip = 0; trip < num_nodes; ++trip) {
        const int64_t node = (int64_t)((1u << level) - 1u) + index;
        float tn, tf;
        bool enter = cast_slab(nodes + 6 * node, ray, tn, tf);
        enter = enter && tf > t_min && (kFarthest ? tf >= best_t : tn <= best_t);
        if (enter && level < leaf_level) {
            level += 1;
            index <<= 1;
            continue;
        }
        if (enter) {
            const int64_t first = (int64_t)index * leaf_size;
            const int64_t end = min(first + leaf_size, (int64_t)num_triangles);
            for (int64_t p = first; p < end; ++p) {
                const int f = min(max(order[p], 0), num_triangles - 1);
                float bn, bf;
                if (!cast_slab(boxes + 6 * (int64_t)f, ray, bn, bf)) continue;
                const int64_t ia = min(max(triangles[3 * (int64_t)f + 0], 0), last_vertex);
                const int64_t ib = min(max(triangles[3 * (int64_t)f + 1], 0), last_vertex);
                const int64_t ic = min(max(triangles[3 * (int64_t)f + 2], 0), last_vertex);
                float e1[3], e2[3], s[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float va = vertices[3 * ia + a];
                    e1[a] = vertices[3 * ib + a] - va;
                    e2[a] = vertices[3 * ic + a] - va;
                    s[a] = ray.o[a] - va;
                }
                const float px = ray.d[1] * e2[2] - ray.d[2] * e2[1];
                const float py = ray.d[2] * e2[0] - ray.d[0] * e2[2];
                const float pz = ray.d[0] * e2[1] - ray.d[1] * e2[0];
                const float det = (px * e1[0] + py * e1[1]) + pz * e1[2];
                const float k = 1.0f / det;
                const float u = ((px * s[0] + py * s[1]) + pz * s[2]) * k;
                const float qx = s[1] * e1[2] - s[2] * e1[1];
                const float qy = s[2] * e1[0] - s[0] * e1[2];
                const float qz = s[0] * e1[1] - s[1] * e1[0];
                const float v = ((ray.d[0] * qx + ray.d[1] * qy) + ray.d[2] * qz) * k;
                const float t = ((qx * e2[0] + qy * e2[1]) + qz * e2[2]) * k;
                // (NaN fails every comparison: a NaN u, v or t is no hit)
                const bool inside = det != 0.0f && u >= 0.0f && v >= 0.0f && u + v <= 1.0f &&
                                    fabsf(t) < __builtin_inff() && t > t_min && bn <= t && t <= bf;
                const bool better = kFarthest ? t > best_t : t < best_t;
                if (inside && (better || (t == best_t && f < best_f))) {
                    best_t = t, best_u = u, best_v = v, best_f = f;
                }
            }
        }
        index += 1;
        if (index == (1u << level)) break;
        const unsigned up = (unsigned)__builtin_ctz(index);
        level -= up;
        index >>= up;
    }
    const bool found = best_f >= 0;
    hit[r] = best_f;
    t_out[r] = found ? best_t : 0.0f;
    u_out[r] = best_u;
    v_out[r] = best_v;
}

struct CastColor {
    float v[3];
};

__global__ void __launch_bounds__(kCastThreads)
mesh_cast_shade_kernel(const int* __restrict__ hit, const float* __restrict__ t,
                       const float* __restrict__ u, const float* __restrict__ v, int64_t num_rays,
                       const int* __restrict__ triangles, int num_triangles,
                       const float* __restrict__ vertex_colors, const float* __restrict__ uvs,
                       int num_vertices, const uint8_t* __restrict__ texture, int tex_height,
                       int tex_width, int tex_channels, CastColor background,
                       float* __restrict__ color, float* __restrict__ alpha,
                       float* __restrict__ depth) {
    const int64_t r = (int64_t)blockIdx.x * kCastThreads + threadIdx.x;
    if (r >= num_rays) return;
    const int f = hit[r];
    if ((unsigned)f >= (unsigned)num_triangles) {
#pragma unroll
        for (int j = 0; j < 3; ++j) color[3 * r + j] = background.v[j];
        alpha[r] = 0.0f;
        depth[r] = 0.0f;
        return;
    }
    const float b1 = u[r], b2 = v[r];
    const float b0 = (1.0f - b1) - b2;
    const int last_vertex = num_vertices - 1;
    const int64_t v0 = min(max(triangles[3 * (int64_t)f + 0], 0), last_vertex);
    const int64_t v1 = min(max(triangles[3 * (int64_t)f + 1], 0), last_vertex);
    const int64_t v2 = min(max(triangles[3 * (int64_t)f + 2], 0), last_vertex);
    alpha[r] = 1.0f;
    depth[r] = t[r];
    if (vertex_colors) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            color[3 * r + j] = (vertex_colors[3 * v0 + j] * b0 + vertex_colors[3 * v1 + j] * b1)
                               + vertex_colors[3 * v2 + j] * b2;
    } else {
        const float tu = (uvs[2 * v0 + 0] * b0 + uvs[2 * v1 + 0] * b1) + uvs[2 * v2 + 0] * b2;
        const float tv = (uvs[2 * v0 + 1] * b0 + uvs[2 * v1 + 1] * b1) + uvs[2 * v2 + 1] * b2;
        mesh_texture_lookup(tu, tv, texture, tex_height, tex_width, tex_channels, color + 3 * r);
    }
}

static bool cast_bad_mesh(int64_t num_vertices, int64_t num_triangles) {
    return num_vertices < 1 || num_triangles < 1 || num_vertices > 0x7fffffff / 3 ||
           num_triangles > 0x7fffffff / 3;
}

// the smallest number of levels whose 2^(levels - 1) leaves of leaf_size hold every triangle
static int cast_levels(int64_t num_triangles, int leaf_size) {
    int levels = 1;
    while (((int64_t)leaf_size << (levels - 1)) < num_triangles) ++levels;
    return levels;
}

static bool cast_bad_tree(int64_t num_triangles, int leaf_size, int levels) {
    return leaf_size < 1 || leaf_size > kCastMaxLeaf || levels < 1 || levels > kCastMaxLevels ||
           levels != cast_levels(num_triangles, leaf_size);
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_mesh_cast_boxes(const float* vertices, int64_t num_vertices,
                                   const int32_t* triangles, int64_t num_triangles, float pad,
                                   float grid_x, float grid_y, float grid_z, float grid_scale,
                                   float* boxes, int32_t* keys, void* stream) {
    if (cast_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_cast_boxes: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (!(pad >= 0.0f) || !(pad < __builtin_inff()))
        return fail_arg("ffn_mesh_cast_boxes: pad (finite and >= 0)");
    if (!(fabsf(grid_x) < __builtin_inff()) || !(fabsf(grid_y) < __builtin_inff()) ||
        !(fabsf(grid_z) < __builtin_inff()) || !(grid_scale >= 0.0f) ||
        !(grid_scale < __builtin_inff()))
        return fail_arg("ffn_mesh_cast_boxes: grid (a finite corner, a finite scale >= 0)");
    if (!vertices || !triangles || !boxes || !keys)
        return fail_arg("ffn_mesh_cast_boxes: null argument");
    const unsigned blocks = (unsigned)((num_triangles + kCastThreads - 1) / kCastThreads);
    hipLaunchKernelGGL(mesh_cast_boxes_kernel, dim3(blocks), dim3(kCastThreads), 0,
                       (hipStream_t)stream, vertices, (int)num_vertices, triangles,
                       (int)num_triangles, pad, grid_x, grid_y, grid_z, grid_scale, boxes, keys);
    return check_launch("ffn_mesh_cast_boxes");
}

extern "C" int ffn_mesh_cast_tree(const float* boxes, const int32_t* order, int64_t num_triangles,
                                  int leaf_size, int levels, float* nodes, void* stream) {
    if (num_triangles < 1 || num_triangles > 0x7fffffff / 3)
        return fail_arg("ffn_mesh_cast_tree: shape (1 <= num_triangles <= (2^31 - 1) / 3)");
    if (cast_bad_tree(num_triangles, leaf_size, levels))
        return fail_arg("ffn_mesh_cast_tree: tree (1 <= leaf_size <= 64, levels the smallest with "
                        "leaf_size 2^(levels - 1) >= num_triangles, at most 31)");
    if (!boxes || !order || !nodes)
        return fail_arg("ffn_mesh_cast_tree: null argument");
    for (int level = levels - 1; level >= 0; --level) {
        const unsigned blocks = (unsigned)((((int64_t)1 << level) + kCastThreads - 1) /
                                           kCastThreads);
        hipLaunchKernelGGL(mesh_cast_tree_kernel, dim3(blocks), dim3(kCastThreads), 0,
                           (hipStream_t)stream, boxes, order, (int)num_triangles, leaf_size,
                           levels, level, nodes);
        const int status = check_launch("ffn_mesh_cast_tree");
        if (status != 0) return status;
    }
    return 0;
}

extern "C" int ffn_mesh_cast(const float* nodes, const float* boxes, const int32_t* order,
                             const float* vertices, int64_t num_vertices,
                             const int32_t* triangles, int64_t num_triangles, int leaf_size,
                             int levels, const float* starts, const float* directions,
                             int64_t num_rays, float t_min, int farthest, int32_t* hit, float* t,
                             float* u, float* v, void* stream) {
    if (cast_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_cast: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (cast_bad_tree(num_triangles, leaf_size, levels))
        return fail_arg("ffn_mesh_cast: tree (1 <= leaf_size <= 64, levels the smallest with "
                        "leaf_size 2^(levels - 1) >= num_triangles, at most 31)");
    if (num_rays < 1 || num_rays > 0x7fffffff)
        return fail_arg("ffn_mesh_cast: rays (1 <= num_rays < 2^31)");
    if (t_min != t_min)
        return fail_arg("ffn_mesh_cast: t_min (not NaN)");
    if (farthest != 0 && farthest != 1)
        return fail_arg("ffn_mesh_cast: farthest (0 or 1)");
    if (!nodes || !boxes || !order || !vertices || !triangles || !starts || !directions || !hit ||
        !t || !u || !v)
        return fail_arg("ffn_mesh_cast: null argument");
    if (((uintptr_t)nodes & 7) != 0 || ((uintptr_t)boxes & 7) != 0)
        return fail_arg("ffn_mesh_cast: nodes and boxes must be 8-byte aligned");
    const unsigned blocks = (unsigned)((num_rays + kCastThreads - 1) / kCastThreads);
    if (farthest)
        hipLaunchKernelGGL(mesh_cast_kernel<true>, dim3(blocks), dim3(kCastThreads), 0,
                           (hipStream_t)stream, nodes, boxes, order, vertices, (int)num_vertices,
                           triangles, (int)num_triangles, leaf_size, levels, starts, directions,
                           num_rays, t_min, hit, t, u, v);
    else
        hipLaunchKernelGGL(mesh_cast_kernel<false>, dim3(blocks), dim3(kCastThreads), 0,
                           (hipStream_t)stream, nodes, boxes, order, vertices, (int)num_vertices,
                           triangles, (int)num_triangles, leaf_size, levels, starts, directions,
                           num_rays, t_min, hit, t, u, v);
    return check_launch("ffn_mesh_cast");
}

extern "C" int ffn_mesh_cast_shade(const int32_t* hit, const float* t, const float* u,
                                   const float* v, int64_t num_rays, const int32_t* triangles,
                                   int64_t num_triangles, const float* vertex_colors,
                                   const float* uvs, int64_t num_vertices, const uint8_t* texture,
                                   int tex_height, int tex_width, int tex_channels,
                                   float background_r, float background_g, float background_b,
                                   float* color, float* alpha, float* depth, void* stream) {
    if (cast_bad_mesh(num_vertices, num_triangles))
        return fail_arg("ffn_mesh_cast_shade: shape (1 <= num_vertices, num_triangles <= "
                        "(2^31 - 1) / 3)");
    if (num_rays < 1 || num_rays > 0x7fffffff)
        return fail_arg("ffn_mesh_cast_shade: rays (1 <= num_rays < 2^31)");
    if (!hit || !t || !u || !v || !triangles || !color || !alpha || !depth)
        return fail_arg("ffn_mesh_cast_shade: null argument");
    if ((vertex_colors != nullptr) == (uvs != nullptr || texture != nullptr) ||
        (uvs != nullptr) != (texture != nullptr))
        return fail_arg("ffn_mesh_cast_shade: either vertex_colors, or uvs and texture");
    if (texture && (tex_height < 1 || tex_width < 1 || tex_channels < 3 ||
                    tex_height > (1 << 24) || tex_width > (1 << 24) ||
                    (int64_t)tex_height * tex_width > 0x7fffffff / tex_channels))
        return fail_arg("ffn_mesh_cast_shade: texture (1 <= height, width <= 2^24, "
                        "channels >= 3, fewer than 2^31 bytes)");
    CastColor b;
    b.v[0] = background_r, b.v[1] = background_g, b.v[2] = background_b;
    const unsigned blocks = (unsigned)((num_rays + kCastThreads - 1) / kCastThreads);
    hipLaunchKernelGGL(mesh_cast_shade_kernel, dim3(blocks), dim3(kCastThreads), 0,
                       (hipStream_t)stream, hit, t, u, v, num_rays, triangles, (int)num_triangles,
                       vertex_colors, uvs, (int)num_vertices, texture, tex_height, tex_width,
                       tex_channels, b, color, alpha, depth);
    return check_launch("ffn_mesh_cast_shade");
}
