// K30  A coloured triangle mesh from a sparse octree: the way out of the tree.
//
// The surface is the boundary between solid and empty finest cells, made of unit quads on the lattice
// of cell corners c = (i, j, k), 0 <= i, j, k <= n, n = 2^(depth-1) finest cells per axis.  A corner's
// eight samples are the cells c - 1 + (dx, dy, dz), bit b = 4 dx + 2 dy + dz (the child digit); its
// mask has bit b set when that cell is solid; it is a vertex when the mask is neither 0 nor 255; its
// key is (i (n+1) + j)(n+1) + k.  Cells outside the cube are empty.
//
//   K30a mesh_solid        per leaf the opacity a = -expm1f(-(sigma * side)) over one FINEST side (0 for
//                          a negative or NaN sigma; 1 without a density; 1 / 0 from a caller's mask) and
//                          the flag a > threshold
//   K30b mesh_candidates   one thread per (solid leaf, corner on its closed surface): the leaf by a
//                          binary search of the exclusive int64 scan of (k+1)^3 - (k-1)^3 = 6 k^2 + 2
//                          corners per solid leaf of k cells a side, the corner by a closed form; eight
//                          cell lookups from the root down with the binary searches of K20a; kept when
//                          the mask is active and the first solid sample in bit order lies in this
//                          thread's leaf, which names every vertex exactly once
//        mesh_scatter      the K12b/c scan of the flags, then a stable scatter of key, mask and the
//                          eight leaf numbers
//   K30c mesh_vertices     per vertex (keys sorted by the caller) the position, colour and normal
//   K30d mesh_face_flags   per (vertex, axis) whether the vertex owns the quad across that axis
//        mesh_faces        per owned quad its three other corners by a binary search of their keys,
//                          two triangles wound so that the normal points from solid to empty
//
// Integers wherever the contract is integer, f32 sums in a fixed order, no float atomics: the same
// input gives the same bits.  Every index read from an input array is held against its range before
// it is used, as in K20: arrays of another tree give a wrong mesh, never an access outside the
// buffers.
#include <math.h>

#include "common.h"
#include "composite_terms.h"
#include "octree_cells.h"

namespace ffn {

constexpr int kMeshThreads = 256;
constexpr int kMeshMaxDepth = 21;       // 3 * 20 bits of path below the root; (n + 1)^3 < 2^63
constexpr float kShY0 = 0.28209479177387814f;

static inline unsigned mesh_blocks(int64_t n) {
    return (unsigned)((n + kMeshThreads - 1) / kMeshThreads);
}

__device__ __forceinline__ int64_t mesh_lower_bound(const int64_t* __restrict__ ids, int64_t n,
                                                    int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------- K30a
__global__ void __launch_bounds__(kMeshThreads)
mesh_solid_kernel(const float* __restrict__ rows, int stride, int sigma_offset,
                  const uint8_t* __restrict__ solid_in, int64_t num_leaves, float side,
                  float threshold, uint8_t* __restrict__ solid, float* __restrict__ alpha) {
    const int64_t l = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (l >= num_leaves) return;
    float a = 1.0f;
    if (solid_in != nullptr) {
        a = solid_in[l] ? 1.0f : 0.0f;
    } else if (rows != nullptr) {
        const float sigma = rows[l * stride + sigma_offset];
        a = sigma >= 0.0f ? -expm1f(-(sigma * side)) : 0.0f;      // NaN fails the comparison
    }
    alpha[l] = a;
    solid[l] = a > threshold;
}

// ---------------------------------------------------------------------------------- K30b
// the leaf number of the finest cell (x, y, z), -1 for empty space and outside the cube: from the
// root down, a leaf met on the way covers the cell, an id in neither index is empty
__device__ __forceinline__ int32_t mesh_cell_leaf(const int64_t* __restrict__ node_index,
                                                  int64_t num_nodes,
                                                  const int64_t* __restrict__ leaf_index,
                                                  int64_t num_leaves, int depth, int64_t x,
                                                  int64_t y, int64_t z) {
    const int64_t n = (int64_t)1 << (depth - 1);
    if (x < 0 || y < 0 || z < 0 || x >= n || y >= n || z >= n) return -1;
    int64_t walk = 0;
    for (int level = 0; level < depth; ++level) {
        int64_t j = mesh_lower_bound(leaf_index, num_leaves, walk);
        if (j < num_leaves && leaf_index[j] == walk) return (int32_t)j;
        if (level == depth - 1) break;
        j = mesh_lower_bound(node_index, num_nodes, walk);
        if (j == num_nodes || node_index[j] != walk) break;          // empty space
        const int bit = depth - 2 - level;
        const int child = (int)(4 * ((x >> bit) & 1) + 2 * ((y >> bit) & 1) + ((z >> bit) & 1));
        walk = 8 * walk + 1 + child;
    }
    return -1;
}

// surface corner number s of a block of k cells a side -> its local corner in [0, k]^3: the plane
// a = 0, the plane a = k, then per a = 1 .. k - 1 the ring of 4 k corners (row b = 0, row b = k, then
// per b = 1 .. k - 1 the two ends c = 0 and c = k)
__device__ __forceinline__ void mesh_surface_corner(int64_t s, int64_t k, int64_t* a, int64_t* b,
                                                    int64_t* c) {
    const int64_t row = k + 1, plane = row * row;
    if (s < 2 * plane) {
        *a = s < plane ? 0 : k;
        if (s >= plane) s -= plane;
        *b = s / row;
        *c = s - *b * row;
        return;
    }
    s -= 2 * plane;
    const int64_t ring = 4 * k;
    *a = 1 + s / ring;
    int64_t r = s - (*a - 1) * ring;
    if (r < 2 * row) {
        *b = r < row ? 0 : k;
        *c = r < row ? r : r - row;
        return;
    }
    r -= 2 * row;
    *b = 1 + (r >> 1);
    *c = (r & 1) ? k : 0;
}

__global__ void __launch_bounds__(kMeshThreads)
mesh_candidates_kernel(const int64_t* __restrict__ node_index, int64_t num_nodes,
                       const int64_t* __restrict__ leaf_index, int64_t num_leaves,
                       const uint8_t* __restrict__ solid, const int64_t* __restrict__ cand_offsets,
                       int64_t first, int64_t count, int depth, uint8_t* __restrict__ flags,
                       int64_t* __restrict__ keys, uint8_t* __restrict__ masks,
                       int32_t* __restrict__ samples) {
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= count) return;
    flags[t] = 0;
    const int64_t g = first + t;
    // the last leaf whose offset is <= g: leaves without candidates share their successor's offset
    int64_t lo = 0, hi = num_leaves + 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cand_offsets[mid] <= g) lo = mid + 1; else hi = mid;
    }
    const int64_t leaf = lo - 1;
    if (leaf < 0 || leaf >= num_leaves || g >= cand_offsets[leaf + 1] || !solid[leaf]) return;
    const int64_t s = g - cand_offsets[leaf];
    // the leaf's level and cell, as K20a reads them off its id
    int64_t id = leaf_index[leaf];
    int64_t cell[3] = {0, 0, 0};
    int d = 0;
    while (id > 0 && d < depth - 1) {
        const int child = (int)((id - 1) & 7);
        cell[0] |= (int64_t)((child >> 2) & 1) << d;
        cell[1] |= (int64_t)((child >> 1) & 1) << d;
        cell[2] |= (int64_t)(child & 1) << d;
        id = (id - 1) >> 3;
        ++d;
    }
    if (id != 0) return;                          // a leaf below the finest level, or a negative id
    const int64_t k = (int64_t)1 << (depth - 1 - d);
    if (s >= 6 * k * k + 2) return;               // offsets made for another depth
    int64_t corner[3];
    mesh_surface_corner(s, k, &corner[0], &corner[1], &corner[2]);
    int64_t base[3];
    for (int a = 0; a < 3; ++a) {
        base[a] = cell[a] * k;
        corner[a] += base[a];
    }
    int mask = 0, owner = -1;
    int32_t sample[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int64_t x = corner[0] - 1 + ((b >> 2) & 1), y = corner[1] - 1 + ((b >> 1) & 1),
                      z = corner[2] - 1 + (b & 1);
        int32_t j;
        if (x >= base[0] && x < base[0] + k && y >= base[1] && y < base[1] + k && z >= base[2] &&
            z < base[2] + k)
            j = (int32_t)leaf;                    // inside this thread's own leaf: no search
        else
            j = mesh_cell_leaf(node_index, num_nodes, leaf_index, num_leaves, depth, x, y, z);
        sample[b] = j;
        if (j >= 0 && solid[j]) {
            mask |= 1 << b;
            if (owner < 0) owner = j;
        }
    }
    if (mask == 0 || mask == 255 || owner != (int32_t)leaf) return;
    const int64_t n1 = ((int64_t)1 << (depth - 1)) + 1;
    flags[t] = 1;
    keys[t] = (corner[0] * n1 + corner[1]) * n1 + corner[2];
    masks[t] = (uint8_t)mask;
#pragma unroll
    for (int b = 0; b < 8; ++b) samples[t * 8 + b] = sample[b];
}

__global__ void __launch_bounds__(kMeshThreads)
mesh_scatter_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                    const int64_t* __restrict__ keys, const uint8_t* __restrict__ masks,
                    const int32_t* __restrict__ samples, int64_t count,
                    int64_t* __restrict__ keys_out, uint8_t* __restrict__ masks_out,
                    int32_t* __restrict__ samples_out) {
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= count || !flags[t]) return;
    const int64_t o = offsets[t];     // < number of set flags <= count: inside the (count, .) outputs
    keys_out[o] = keys[t];
    masks_out[o] = masks[t];
#pragma unroll
    for (int b = 0; b < 8; ++b) samples_out[o * 8 + b] = samples[t * 8 + b];
}

// ---------------------------------------------------------------------------------- K30c
struct MeshColor { int offset, step, sh; };      // channel c of a row at offset + c * step

__global__ void __launch_bounds__(kMeshThreads)
mesh_vertices_kernel(const int64_t* __restrict__ keys, const uint8_t* __restrict__ masks,
                     const int32_t* __restrict__ samples, int64_t num_vertices,
                     const float* __restrict__ alpha, const float* __restrict__ rows,
                     int64_t num_leaves, int stride, MeshColor color, int depth, float side, float cx,
                     float cy, float cz, float threshold, int surface_nets,
                     float* __restrict__ vertices, float* __restrict__ colors,
                     float* __restrict__ normals, int32_t* __restrict__ corners) {
    const int64_t v = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (v >= num_vertices) return;
    const int64_t n = (int64_t)1 << (depth - 1), n1 = n + 1;
    int64_t key = keys[v];
    if (key < 0 || key >= n1 * n1 * n1) key = 0;
    const int64_t ci = key / (n1 * n1), cj = key / n1 - ci * n1, ck = key - (key / n1) * n1;
    const int mask = masks[v];
    float a[8];
    int32_t leaf[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int32_t j = samples[v * 8 + b];
        leaf[b] = j >= 0 && j < num_leaves ? j : -1;
        a[b] = leaf[b] >= 0 ? alpha[leaf[b]] : 0.0f;
    }
    // the offset: the mean of the crossings of the 12 sample pairs, x pairs first, then y, then z,
    // within an axis by ascending lower bit
    float off[3] = {0.0f, 0.0f, 0.0f};
    if (surface_nets) {
        int crossings = 0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const int step = 4 >> ax;
#pragma unroll
            for (int b0 = 0; b0 < 8; ++b0) {
                if (b0 & step) continue;
                const int b1 = b0 | step;
                if (((mask >> b0) & 1) == ((mask >> b1) & 1)) continue;
                const float t = (threshold - a[b0]) / (a[b1] - a[b0]);
                float p[3] = {(float)((b0 >> 2) & 1) - 0.5f, (float)((b0 >> 1) & 1) - 0.5f,
                              (float)(b0 & 1) - 0.5f};
                p[ax] = p[ax] + t;
                off[0] += p[0];
                off[1] += p[1];
                off[2] += p[2];
                ++crossings;
            }
        }
        if (crossings > 0) {
            const float count = (float)crossings;
            off[0] /= count;
            off[1] /= count;
            off[2] /= count;
        }
    }
    const float mid = (float)n * 0.5f;            // n / 2: 0.5 for the one-cell tree of depth 1
    vertices[v * 3 + 0] = cx + (((float)ci - mid) + off[0]) * side;
    vertices[v * 3 + 1] = cy + (((float)cj - mid) + off[1]) * side;
    vertices[v * 3 + 2] = cz + (((float)ck - mid) + off[2]) * side;
    corners[v * 3 + 0] = (int32_t)ci;
    corners[v * 3 + 1] = (int32_t)cj;
    corners[v * 3 + 2] = (int32_t)ck;
    // the normal: minus the gradient of the opacity over the eight samples, g = sum_b a_b * 2 p_b
    float g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        g[0] += (b & 4) ? a[b] : -a[b];
        g[1] += (b & 2) ? a[b] : -a[b];
        g[2] += (b & 1) ? a[b] : -a[b];
    }
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[v * 3 + c] = len > 0.0f ? -g[c] / len : 0.0f;
    // the colour: the mean over the solid samples in bit order, each of them counted once
    if (colors != nullptr) {
        float sum[3] = {0.0f, 0.0f, 0.0f};
        int solid = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (!((mask >> b) & 1) || leaf[b] < 0) continue;
            const float* row = rows + (int64_t)leaf[b] * stride + color.offset;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float value = row[c * color.step];
                sum[c] += color.sh ? sigmoid_f(value * kShY0) : value;
            }
            ++solid;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) colors[v * 3 + c] = solid > 0 ? sum[c] / (float)solid : 0.0f;
    }
}

// ---------------------------------------------------------------------------------- K30d
// slot 3 v + ax: vertex v owns the quad across axis ax when cell c (bit 7) and cell c - e_ax differ
__global__ void __launch_bounds__(kMeshThreads)
mesh_face_flags_kernel(const uint8_t* __restrict__ masks, int64_t slots,
                       uint8_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= slots) return;
    const int64_t v = t / 3;
    const int ax = (int)(t - v * 3);
    const int mask = masks[v];
    flags[t] = ((mask >> 7) & 1) != ((mask >> (7 ^ (4 >> ax))) & 1);
}

__global__ void __launch_bounds__(kMeshThreads)
mesh_faces_kernel(const int64_t* __restrict__ keys, const uint8_t* __restrict__ masks,
                  const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                  int64_t num_vertices, int depth, int64_t num_quads,
                  int32_t* __restrict__ triangles, int32_t* __restrict__ missing) {
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= num_vertices * 3 || !flags[t]) return;
    const int64_t o = offsets[t];
    if (o < 0 || o >= num_quads) { *missing = 1; return; }
    const int64_t v = t / 3;
    const int ax = (int)(t - v * 3);
    const int64_t n1 = ((int64_t)1 << (depth - 1)) + 1;
    const int64_t stride[3] = {n1 * n1, n1, 1};
    const int64_t key = keys[v];
    const int64_t eu = stride[(ax + 1) % 3], ev = stride[(ax + 2) % 3];
    // a corner at n along u or v has no cell c inside the cube and owns no quad: key + eu would be
    // another row's corner
    int64_t coord[3] = {key / (n1 * n1), key / n1 % n1, key % n1};
    if (key < 0 || coord[0] >= n1 || coord[(ax + 1) % 3] + 1 >= n1 ||
        coord[(ax + 2) % 3] + 1 >= n1) {
        *missing = 1;
        return;
    }
    const int64_t want[3] = {key + eu, key + eu + ev, key + ev};
    int32_t q[4] = {(int32_t)v, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int64_t j = mesh_lower_bound(keys, num_vertices, want[i]);
        if (j >= num_vertices || keys[j] != want[i]) { *missing = 1; return; }
        q[i + 1] = (int32_t)j;
    }
    // as written the quad's normal is +ax: right when the cell below (c - e_ax) is the solid one
    if ((masks[v] >> 7) & 1) {
        const int32_t swap = q[1];
        q[1] = q[3];
        q[3] = swap;
    }
    int32_t* out = triangles + o * 6;
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    out[3] = q[0]; out[4] = q[2]; out[5] = q[3];
}

static inline bool mesh_depth_ok(int depth) { return depth >= 1 && depth <= kMeshMaxDepth; }

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_octree_mesh_max_depth(void) { return kMeshMaxDepth; }

extern "C" int ffn_octree_mesh_solid(const float* leaf_rows, int stride, int sigma_offset,
                                     const uint8_t* solid_in, int64_t num_leaves, float side,
                                     float threshold, uint8_t* solid, float* alpha, void* stream) {
    if (num_leaves < 1 || num_leaves >= ((int64_t)1 << 31))
        return fail_arg("ffn_octree_mesh_solid: shape (1 <= num_leaves < 2^31)");
    if (!solid || !alpha) return fail_arg("ffn_octree_mesh_solid: null argument");
    if (!(threshold > 0.0f) || !(threshold < 1.0f))
        return fail_arg("ffn_octree_mesh_solid: threshold must lie in (0, 1)");
    if (!(side > 0.0f) || !(side < 3.0e38f))
        return fail_arg("ffn_octree_mesh_solid: side must be finite and positive");
    if (leaf_rows && (stride < 1 || sigma_offset < 0 || sigma_offset >= stride))
        return fail_arg("ffn_octree_mesh_solid: stride >= 1 and 0 <= sigma_offset < stride");
    hipLaunchKernelGGL(mesh_solid_kernel, dim3(mesh_blocks(num_leaves)), dim3(kMeshThreads), 0,
                       (hipStream_t)stream, leaf_rows, stride, sigma_offset, solid_in, num_leaves,
                       side, threshold, solid, alpha);
    return check_launch("ffn_octree_mesh_solid");
}

extern "C" int ffn_octree_mesh_candidates(const int64_t* node_index, int64_t num_nodes,
                                          const int64_t* leaf_index, int64_t num_leaves,
                                          const uint8_t* solid, const int64_t* cand_offsets,
                                          int64_t first, int64_t count, int depth, uint8_t* flags,
                                          int* offsets, int* tile_sums, int64_t* keys_scratch,
                                          uint8_t* masks_scratch, int32_t* samples_scratch,
                                          int64_t* keys, uint8_t* masks, int32_t* samples,
                                          int* total, void* stream) {
    if (num_leaves < 1 || num_leaves >= ((int64_t)1 << 31) || num_nodes < 0)
        return fail_arg("ffn_octree_mesh_candidates: shape (1 <= num_leaves < 2^31, num_nodes >= "
                        "0)");
    if (!mesh_depth_ok(depth))
        return fail_arg("ffn_octree_mesh_candidates: depth outside 1 .. 21");
    if (first < 0 || count < 1 || count > ffn_octree_max_points())
        return fail_arg("ffn_octree_mesh_candidates: first >= 0 and 1 <= count <= "
                        "ffn_octree_max_points()");
    if (!leaf_index || !solid || !cand_offsets || !flags || !offsets || !tile_sums ||
        !keys_scratch || !masks_scratch || !samples_scratch || !keys || !masks || !samples ||
        !total || (num_nodes > 0 && !node_index))
        return fail_arg("ffn_octree_mesh_candidates: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_candidates_kernel, dim3(mesh_blocks(count)), dim3(kMeshThreads), 0, st,
                       node_index, num_nodes, leaf_index, num_leaves, solid, cand_offsets, first,
                       count, depth, flags, keys_scratch, masks_scratch, samples_scratch);
    if (int err = octree_scan_flags(flags, count, tile_sums, offsets, total, st)) return err;
    hipLaunchKernelGGL(mesh_scatter_kernel, dim3(mesh_blocks(count)), dim3(kMeshThreads), 0, st,
                       flags, offsets, keys_scratch, masks_scratch, samples_scratch, count, keys,
                       masks, samples);
    return check_launch("ffn_octree_mesh_candidates");
}

extern "C" int ffn_octree_mesh_vertices(const int64_t* keys, const uint8_t* masks,
                                        const int32_t* samples, int64_t num_vertices,
                                        const float* alpha, const float* leaf_rows,
                                        int64_t num_leaves, int stride, int color_offset,
                                        int color_step, int color_sh, int depth, float scale,
                                        float center_x, float center_y, float center_z,
                                        float threshold, int surface_nets, float* vertices,
                                        float* colors, float* normals, int32_t* corners,
                                        void* stream) {
    if (num_vertices < 1 || num_vertices >= ((int64_t)1 << 31) || num_leaves < 1 ||
        num_leaves >= ((int64_t)1 << 31))
        return fail_arg("ffn_octree_mesh_vertices: shape (1 <= num_vertices, num_leaves < 2^31)");
    if (!mesh_depth_ok(depth)) return fail_arg("ffn_octree_mesh_vertices: depth outside 1 .. 21");
    if (!keys || !masks || !samples || !alpha || !vertices || !normals || !corners)
        return fail_arg("ffn_octree_mesh_vertices: null argument");
    if ((leaf_rows == nullptr) != (colors == nullptr))
        return fail_arg("ffn_octree_mesh_vertices: leaf_rows and colors go together");
    if (leaf_rows && (stride < 1 || color_step < 1 || color_offset < 0 ||
                      (int64_t)color_offset + 2 * (int64_t)color_step >= stride))
        return fail_arg("ffn_octree_mesh_vertices: the three colour columns color_offset + c "
                        "color_step must lie inside the row");
    if (!(threshold > 0.0f) || !(threshold < 1.0f))
        return fail_arg("ffn_octree_mesh_vertices: threshold must lie in (0, 1)");
    if (!(scale > 0.0f) || !(scale < 3.0e38f))
        return fail_arg("ffn_octree_mesh_vertices: scale must be finite and positive");
    if (center_x != center_x || center_y != center_y || center_z != center_z)
        return fail_arg("ffn_octree_mesh_vertices: the centre is NaN");
    const float side = 2.0f * scale / (float)((int64_t)1 << (depth - 1));
    MeshColor color = {color_offset, color_step, color_sh != 0};
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3(mesh_blocks(num_vertices)), dim3(kMeshThreads), 0,
                       (hipStream_t)stream, keys, masks, samples, num_vertices, alpha, leaf_rows,
                       num_leaves, stride, color, depth, side, center_x, center_y, center_z,
                       threshold, surface_nets != 0, vertices, colors, normals, corners);
    return check_launch("ffn_octree_mesh_vertices");
}

extern "C" int ffn_octree_mesh_face_flags(const uint8_t* masks, int64_t num_vertices,
                                          uint8_t* flags, int* offsets, int* tile_sums, int* total,
                                          void* stream) {
    if (num_vertices < 1 || 3 * num_vertices > ffn_octree_max_points())
        return fail_arg("ffn_octree_mesh_face_flags: shape (1 <= 3 num_vertices <= "
                        "ffn_octree_max_points())");
    if (!masks || !flags || !offsets || !tile_sums || !total)
        return fail_arg("ffn_octree_mesh_face_flags: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_face_flags_kernel, dim3(mesh_blocks(3 * num_vertices)),
                       dim3(kMeshThreads), 0, st, masks, 3 * num_vertices, flags);
    if (int err = octree_scan_flags(flags, 3 * num_vertices, tile_sums, offsets, total, st))
        return err;
    return check_launch("ffn_octree_mesh_face_flags");
}

extern "C" int ffn_octree_mesh_faces(const int64_t* keys, const uint8_t* masks,
                                     const uint8_t* flags, const int* offsets,
                                     int64_t num_vertices, int depth, int64_t num_quads,
                                     int32_t* triangles, int32_t* missing, void* stream) {
    if (num_vertices < 1 || 3 * num_vertices > ffn_octree_max_points() || num_quads < 1 ||
        num_quads > 3 * num_vertices)
        return fail_arg("ffn_octree_mesh_faces: shape (1 <= 3 num_vertices <= "
                        "ffn_octree_max_points(), 1 <= num_quads <= 3 num_vertices)");
    if (!mesh_depth_ok(depth)) return fail_arg("ffn_octree_mesh_faces: depth outside 1 .. 21");
    if (!keys || !masks || !flags || !offsets || !triangles || !missing)
        return fail_arg("ffn_octree_mesh_faces: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(missing, 0, sizeof(int32_t), st) != hipSuccess)
        return check_launch("ffn_octree_mesh_faces");
    hipLaunchKernelGGL(mesh_faces_kernel, dim3(mesh_blocks(3 * num_vertices)), dim3(kMeshThreads),
                       0, st, keys, masks, flags, offsets, num_vertices, depth, num_quads, triangles,
                       missing);
    if (int err = check_launch("ffn_octree_mesh_faces")) return err;
    int32_t host = 0;
    hipError_t err = hipMemcpyAsync(&host, missing, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) {
        set_error("ffn_octree_mesh_faces: reading the status back", err);
        return (int)err;
    }
    if (host != 0)
        return fail_arg("ffn_octree_mesh_faces: a quad's corner is not among the vertices (keys "
                        "unsorted, or masks of another tree); its triangles were not written");
    return 0;
}
