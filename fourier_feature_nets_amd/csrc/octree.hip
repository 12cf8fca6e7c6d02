// K12  Sparse octree from a point cloud, and the surface points that feed it.
//
// Replaces the host-side (Python / Numba, one point at a time) octree of the reference:
// voxelize_model.py:71-77 (surface points of a render batch), octree.py:274-286 (child index of
// a point), octree.py:733-806 (build_from_samples), octree.py:513-541 (point query) and the
// node-by-node walk behind leaf_centers / leaf_depths (octree.py:564-582, 605-613).
//
// Node ids are the reference's: root 0, children of i are 8 i + 1 .. 8 i + 8, child index
// 4 [x >= cx] + 2 [y >= cy] + [z >= cz].  A node centre is reached from the root by adding
// +-scale / 2^k level by level, every add rounded to f32 (the reference's Node arithmetic on an
// np.float32 scale); the kernels replay exactly that chain, so a point on or next to a splitting
// plane takes the reference's side.
//
// The build counts by SORTING: a point's path code is its D-1 child indices, 3 bits each, root
// first.  With the codes sorted (a stable key sort done by the caller), the points of any node
// are one contiguous range and the ranges of its children nest inside it, so "how many points
// does this node hold" is two binary searches inside the parent's range -- integer work only,
// no atomics, no per-level histogram whose size grows as 8^D.
//
//   K12a surface_flags / K12d surface_scatter   alpha > threshold, stable compaction
//   K12b/c scan_*            exclusive scan of u8 flags (tile counts, one-workgroup scan, offsets)
//   K12e path_codes          per point: shift by the cube centre, descend D-1 levels
//   K12f assign              per sorted point: walk down the nested ranges, stop at the first
//                            node with < min_leaf_size points; leaf id or -1
//   K12g leaf_heads / leaf_gather    first point of every leaf -> (id, start, count), code order
//   K12h ancestor_flags / ancestor_gather   interior nodes = proper ancestors of the leaves
//   K12i leaf_means          one wave per leaf, lanes stride the leaf's points in sorted order,
//                            fixed butterfly: the same input gives the same bits
//   K12j query               containment, descent, binary search in the sorted id arrays
//   K12k leaf_geometry       centre and depth of a leaf from its id alone
#include "common.h"
#include "octree_cells.h"

namespace ffn {

constexpr int kOctThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kOctThreads * kScanItems;
constexpr int kOctMaxDepth = 11;      // 3 (D - 1) code bits in an int32
constexpr int kOctMaxLevels = 21;     // 8^21 < 2^63: the deepest id an int64 holds

static inline int oct_blocks(int64_t n) { return (int)((n + kOctThreads - 1) / kOctThreads); }
static inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

// inclusive scan of one int per thread over the workgroup; *total = sum over the workgroup
__device__ __forceinline__ int block_inclusive_scan(int v, int* wave_sums, int* total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int up = __shfl_up(v, off, kWave);
        if (lane >= off) v += up;
    }
    __syncthreads();   // wave_sums may still be read from the previous call
    if (lane == kWave - 1) wave_sums[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kOctThreads / kWave; ++w) {
        const int s = wave_sums[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return v + before;
}

// ------------------------------------------------------------------------------- K12b/c
__global__ void __launch_bounds__(kOctThreads)
scan_tile_counts_kernel(const uint8_t* __restrict__ flags, int64_t n, int* __restrict__ tile_sums) {
    __shared__ int wave_sums[kOctThreads / kWave];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int c = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < n) c += flags[base + j] != 0;
    int total;
    block_inclusive_scan(c, wave_sums, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums -> exclusive prefix in place, *total = sum
__global__ void __launch_bounds__(kOctThreads)
scan_tile_sums_kernel(int* __restrict__ tile_sums, int64_t tiles, int* __restrict__ total_out) {
    __shared__ int wave_sums[kOctThreads / kWave];
    int carry = 0;
    for (int64_t base = 0; base < tiles; base += kOctThreads) {
        const int64_t i = base + threadIdx.x;
        const int v = i < tiles ? tile_sums[i] : 0;
        int total;
        const int incl = block_inclusive_scan(v, wave_sums, &total);
        if (i < tiles) tile_sums[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(kOctThreads)
scan_offsets_kernel(const uint8_t* __restrict__ flags, int64_t n, const int* __restrict__ tile_sums,
                    int* __restrict__ offsets) {
    __shared__ int wave_sums[kOctThreads / kWave];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    bool f[kScanItems];
    int c = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        f[j] = base + j < n && flags[base + j] != 0;
        c += f[j];
    }
    int total;
    int rank = tile_sums[blockIdx.x] + block_inclusive_scan(c, wave_sums, &total) - c;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (base + j < n) offsets[base + j] = rank;
        rank += f[j];
    }
}

// flags (n) -> offsets (n) exclusive, *total; tile_sums holds scan_tiles(n) ints
static int scan_flags(const uint8_t* flags, int64_t n, int* tile_sums, int* offsets, int* total,
                      hipStream_t s) {
    const int64_t tiles = scan_tiles(n);
    hipLaunchKernelGGL(scan_tile_counts_kernel, dim3((unsigned)tiles), dim3(kOctThreads), 0, s,
                       flags, n, tile_sums);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(1), dim3(kOctThreads), 0, s, tile_sums, tiles,
                       total);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3((unsigned)tiles), dim3(kOctThreads), 0, s, flags,
                       n, tile_sums, offsets);
    return check_launch("ffn_octree: flag scan");
}

// ------------------------------------------------------------------------------- K12a/d
__global__ void __launch_bounds__(kOctThreads)
surface_flags_kernel(const float* __restrict__ alpha, int64_t n, float threshold,
                     uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i < n) flags[i] = alpha[i] > threshold;
}

__global__ void __launch_bounds__(kOctThreads)
surface_scatter_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                       const float* __restrict__ starts, const float* __restrict__ directions,
                       const float* __restrict__ depth, const float* __restrict__ color,
                       int64_t n, int channels, float* __restrict__ out_positions,
                       float* __restrict__ out_colors) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int64_t o = offsets[i];   // < number of set flags <= n: inside the (n, .) outputs
    const float d = depth[i];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out_positions[o * 3 + a] = mul_add_rn(directions[i * 3 + a], d, starts[i * 3 + a]);
    for (int c = 0; c < channels; ++c) out_colors[o * channels + c] = color[i * channels + c];
}

// ------------------------------------------------------------------------------- K12e
// child index of p in the node centred at c (octree.py:274-286), and the child's centre
__device__ __forceinline__ int descend(float x, float y, float z, float& cx, float& cy, float& cz,
                                       float half) {
#pragma clang fp contract(off)
    const bool px = x >= cx, py = y >= cy, pz = z >= cz;
    cx = px ? cx + half : cx - half;
    cy = py ? cy + half : cy - half;
    cz = pz ? cz + half : cz - half;
    return (px ? 4 : 0) + (py ? 2 : 0) + (pz ? 1 : 0);
}

__global__ void __launch_bounds__(kOctThreads)
path_codes_kernel(const float* __restrict__ positions, int64_t n, float ox, float oy, float oz,
                  float scale, int depth, int* __restrict__ codes) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n) return;
    const float x = sub_rn(positions[i * 3 + 0], ox);
    const float y = sub_rn(positions[i * 3 + 1], oy);
    const float z = sub_rn(positions[i * 3 + 2], oz);
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, half = scale;
    uint32_t code = 0u;
    for (int level = 1; level < depth; ++level) {
        half *= 0.5f;
        code = (code << 3) | (uint32_t)descend(x, y, z, cx, cy, cz, half);
    }
    codes[i] = (int)code;
}

// ------------------------------------------------------------------------------- K12f
// first index in [lo, hi) whose code is >= key
__device__ __forceinline__ int64_t lower_bound_code(const int* __restrict__ codes, int64_t lo,
                                                    int64_t hi, uint32_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)codes[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kOctThreads)
assign_kernel(const int* __restrict__ codes, const int64_t* __restrict__ perm, int64_t n, int depth,
              int64_t min_leaf, int64_t* __restrict__ leaf_sorted, int* __restrict__ count_sorted,
              int64_t* __restrict__ leaf_of_point) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t code = (uint32_t)codes[i];
    int64_t lo = 0, hi = n, id = 0, leaf = -1;
    bool done = false;
    if (depth == 1) {
        leaf = n >= min_leaf ? 0 : -1;
        done = true;
    }
    for (int level = 1; level < depth && !done; ++level) {
        const int shift = 3 * (depth - 1 - level);
        const uint32_t prefix = code >> shift;
        const int64_t clo = lower_bound_code(codes, lo, hi, prefix << shift);
        const int64_t chi = lower_bound_code(codes, clo, hi, (prefix + 1u) << shift);
        if (chi - clo < min_leaf) {
            // this child is not visited: its parent is a leaf iff no sibling is visited either,
            // otherwise the point is dropped (octree.py:780-797)
            const uint32_t first = prefix & ~7u;
            bool any = false;
            int64_t b = lo;
            for (uint32_t j = 1; j <= 8u; ++j) {
                const int64_t e = j == 8u ? hi : lower_bound_code(codes, b, hi, (first + j) << shift);
                any = any || e - b >= min_leaf;
                b = e;
            }
            if (!any) leaf = id;
            done = true;
        } else {
            id = 8 * id + 1 + (prefix & 7u);
            lo = clo;
            hi = chi;
        }
    }
    if (!done) leaf = id;   // visited at depth D-1 with >= min_leaf points
    leaf_sorted[i] = leaf;
    count_sorted[i] = (int)(hi - lo);
    leaf_of_point[perm[i]] = leaf;   // perm is a permutation of [0, n)
}

// ------------------------------------------------------------------------------- K12g
__global__ void __launch_bounds__(kOctThreads)
leaf_heads_kernel(const int64_t* __restrict__ leaf_sorted, int64_t n, uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t leaf = leaf_sorted[i];
    flags[i] = leaf >= 0 && (i == 0 || leaf_sorted[i - 1] != leaf);
}

__global__ void __launch_bounds__(kOctThreads)
leaf_gather_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                   const int64_t* __restrict__ leaf_sorted, const int* __restrict__ count_sorted,
                   int64_t n, int64_t* __restrict__ leaf_ids, int64_t* __restrict__ leaf_start,
                   int* __restrict__ leaf_count) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int o = offsets[i];
    leaf_ids[o] = leaf_sorted[i];
    leaf_start[o] = i;
    leaf_count[o] = count_sorted[i];
}

// ------------------------------------------------------------------------------- K12h
__device__ __forceinline__ int id_depth(int64_t id) {
    int d = 0;
    while (id > 0) { id = (id - 1) >> 3; ++d; }
    return d;
}
__device__ __forceinline__ int64_t ancestor_at(int64_t id, int from_depth, int level) {
    for (int d = from_depth; d > level; --d) id = (id - 1) >> 3;
    return id;
}

// leaves in code (depth-first) order: the leaves below one node are consecutive, so ancestor
// (leaf j, level L) is new iff leaf j-1 does not have the same one.  flags (num_leaves, levels).
__global__ void __launch_bounds__(kOctThreads)
ancestor_flags_kernel(const int64_t* __restrict__ leaf_ids, int64_t num_leaves, int levels,
                      uint8_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (t >= num_leaves * levels) return;
    const int64_t j = t / levels;
    const int level = (int)(t % levels);
    const int64_t id = leaf_ids[j];
    const int d = id_depth(id);
    bool flag = false;
    if (level < d) {
        flag = true;
        if (j > 0) {
            const int64_t prev = leaf_ids[j - 1];
            const int pd = id_depth(prev);
            if (level < pd && ancestor_at(prev, pd, level) == ancestor_at(id, d, level)) flag = false;
        }
    }
    flags[t] = flag;
}

__global__ void __launch_bounds__(kOctThreads)
ancestor_gather_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                       const int64_t* __restrict__ leaf_ids, int64_t num_leaves, int levels,
                       int64_t* __restrict__ node_ids) {
    const int64_t t = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (t >= num_leaves * levels || !flags[t]) return;
    const int64_t id = leaf_ids[t / levels];
    node_ids[offsets[t]] = ancestor_at(id, id_depth(id), (int)(t % levels));
}

// ------------------------------------------------------------------------------- K12i
__global__ void __launch_bounds__(kOctThreads)
leaf_means_kernel(const float* __restrict__ data, int channels, const int64_t* __restrict__ perm,
                  const int64_t* __restrict__ leaf_start, const int* __restrict__ leaf_count,
                  int64_t num_leaves, float* __restrict__ out) {
    const int64_t leaf = (int64_t)blockIdx.x * (kOctThreads / kWave) + (threadIdx.x >> 6);
    if (leaf >= num_leaves) return;   // whole waves leave together
    const int lane = lane_id();
    const int64_t start = leaf_start[leaf];
    const int count = leaf_count[leaf];
    for (int c = 0; c < channels; ++c) {
        float acc = 0.0f;
        for (int j = lane; j < count; j += kWave) acc += data[perm[start + j] * channels + c];
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, kWave);
        if (lane == 0) out[leaf * channels + c] = acc / (float)count;
    }
}

// ------------------------------------------------------------------------------- K12j
__device__ __forceinline__ int64_t lower_bound_id(const int64_t* __restrict__ ids, int64_t n,
                                                  int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kOctThreads)
query_kernel(const float* __restrict__ positions, int64_t n, float scale,
             const int64_t* __restrict__ node_index, int64_t num_nodes,
             const int64_t* __restrict__ leaf_index, int64_t num_leaves, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n) return;
    const float x = positions[i * 3 + 0], y = positions[i * 3 + 1], z = positions[i * 3 + 2];
    int64_t result = -1;
    // _node_contains (octree.py:262-267): the faces belong to the cube
    const bool outside = fabsf(x) > scale || fabsf(y) > scale || fabsf(z) > scale;
    if (!outside) {
        if (leaf_index[0] == 0) {
            result = 0;   // the root is the only leaf
        } else {
            const int64_t max_id = leaf_index[num_leaves - 1];
            float cx = 0.0f, cy = 0.0f, cz = 0.0f, half = scale;
            int64_t id = 0;
            for (int level = 0; level < kOctMaxLevels && id <= max_id; ++level) {
                half *= 0.5f;
                id = 8 * id + 1 + descend(x, y, z, cx, cy, cz, half);
                int64_t j = lower_bound_id(leaf_index, num_leaves, id);
                if (j < num_leaves && leaf_index[j] == id) { result = j; break; }
                j = lower_bound_id(node_index, num_nodes, id);
                if (j == num_nodes || node_index[j] != id) break;
            }
        }
    }
    out[i] = result;
}

// ------------------------------------------------------------------------------- K12k
__global__ void __launch_bounds__(kOctThreads)
leaf_geometry_kernel(const int64_t* __restrict__ leaf_index, int64_t num_leaves, float scale,
                     float* __restrict__ centers, int* __restrict__ depths) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= num_leaves) return;
    int64_t id = leaf_index[i];
    uint64_t digits = 0u;   // child indices, the leaf's own in the low bits
    int d = 0;
    while (id > 0 && d < kOctMaxLevels) {
        digits |= (uint64_t)((id - 1) & 7) << (3 * d);
        id = (id - 1) >> 3;
        ++d;
    }
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, half = scale;
    for (int k = d - 1; k >= 0; --k) {
        const int child = (int)((digits >> (3 * k)) & 7u);
        half *= 0.5f;
        cx = (child & 4) ? cx + half : cx - half;
        cy = (child & 2) ? cy + half : cy - half;
        cz = (child & 1) ? cz + half : cz - half;
    }
    centers[i * 3 + 0] = cx;
    centers[i * 3 + 1] = cy;
    centers[i * 3 + 2] = cz;
    depths[i] = d;
}

// ------------------------------------------------------------------------------- K16
// Density octree from a trained model: the finest grid is evaluated densely, chunk by chunk, in
// path-code order.  No reference counterpart (voxelize_model.py builds from depth renders only).
//
//   K16a cell_centers     code -> centre of the finest cell, the chain of K12k plus the cube centre
//   K16b density_scatter  stable compaction of the cells octree_density_flags_kernel
//                         (composite.hip, where the activations live) has flagged; K23
//                         (carve.hip) flags its cells itself and shares this tail
//   K16c merge_*          one bottom-up coarsening pass over the code-sorted leaf list
__global__ void __launch_bounds__(kOctThreads)
cell_centers_kernel(int64_t first_code, int64_t count, float ox, float oy, float oz, float scale,
                    int depth, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= count) return;
    float x, y, z;
    oct_cell_center(first_code + i, ox, oy, oz, scale, depth, &x, &y, &z);
    out[i * 3 + 0] = x;
    out[i * 3 + 1] = y;
    out[i * 3 + 2] = z;
}

__global__ void __launch_bounds__(kOctThreads)
density_scatter_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                       const float4* __restrict__ activated, int64_t first_code, int64_t count,
                       int* __restrict__ codes_out, float4* __restrict__ data_out) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= count || !flags[i]) return;
    const int64_t o = offsets[i];   // < number of set flags <= count: inside the (count, .) outputs
    codes_out[o] = (int)(first_code + i);
    data_out[o] = activated[i];
}

// mean of eight siblings: the f32 sum of children 0 .. 7 in that order, times 1/8
__device__ __forceinline__ float4 sibling_mean(const float4* __restrict__ d) {
#pragma clang fp contract(off)
    float4 s = d[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const float4 v = d[k];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    return make_float4(s.x * 0.125f, s.y * 0.125f, s.z * 0.125f, s.w * 0.125f);
}

// merge[i] = entry i heads eight siblings, all leaves of `level`, that lie within the tolerances
// of their mean.  A NaN in the group fails a comparison: no merge.
__global__ void __launch_bounds__(kOctThreads)
merge_heads_kernel(const int* __restrict__ codes, const int* __restrict__ levels,
                   const float4* __restrict__ data, int64_t n, int level, int depth, float rgb_tol,
                   float sigma_tol, uint8_t* __restrict__ merge) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n) return;
    const int shift = 3 * (depth - 1 - level);
    bool ok = false;
    if (i + 7 < n && levels[i] == level && (((uint32_t)codes[i] >> shift) & 7u) == 0u) {
        bool all = true;
#pragma unroll
        for (int k = 1; k < 8; ++k) all = all && levels[i + k] == level;
        if (all && ((uint32_t)codes[i + 7] >> shift) == ((uint32_t)codes[i] >> shift) + 7u) {
            const float4 m = sibling_mean(data + i);
            ok = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 v = data[i + k];
                ok = ok && fabsf(v.x - m.x) <= rgb_tol && fabsf(v.y - m.y) <= rgb_tol &&
                     fabsf(v.z - m.z) <= rgb_tol && fabsf(v.w - m.w) <= sigma_tol;
            }
        }
    }
    merge[i] = ok;
}

// an entry stays unless it is child 1 .. 7 of a merging group; its head is then j entries before
__global__ void __launch_bounds__(kOctThreads)
merge_flags_kernel(const int* __restrict__ codes, const int* __restrict__ levels,
                   const uint8_t* __restrict__ merge, int64_t n, int level, int depth,
                   uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(((uint32_t)codes[i] >> (3 * (depth - 1 - level))) & 7u);
    flags[i] = !(levels[i] == level && j > 0 && i >= j && merge[i - j]);
}

__global__ void __launch_bounds__(kOctThreads)
merge_scatter_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                     const uint8_t* __restrict__ merge, const int* __restrict__ codes,
                     const int* __restrict__ levels, const float4* __restrict__ data, int64_t n,
                     int* __restrict__ codes_out, int* __restrict__ levels_out,
                     float4* __restrict__ data_out) {
    const int64_t i = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int64_t o = offsets[i];   // < number of set flags <= n
    const bool head = merge[i];     // then i + 7 < n
    codes_out[o] = codes[i];        // child 0 of its parent: the parent's left-aligned code
    levels_out[o] = head ? levels[i] - 1 : levels[i];
    data_out[o] = head ? sibling_mean(data + i) : data[i];
}

// ------------------------------------------------------------------------------- K21b
// A fitted tree rebuilt from one decision per leaf: 0 drop, 1 keep, 2 split into its eight children,
// which take the leaf's row.  No reference counterpart (its prune merges the deepest level only).
//
// Leaves come in path-code order, and that order survives: a leaf replaced in place by its children in
// child order 4 bx + 2 by + bz stays sorted.  Leaf i owns the eight SLOTS 8 i .. 8 i + 7; a keep sets
// the flag of slot 8 i, a split all eight, so the K12b/c flag scan over the 8 L slots gives every
// output leaf its place and *total the new leaf count, without an atomic and without a search for the
// source leaf of an output leaf.  An action above 2 sets no flag here; the caller refuses it.
__global__ void __launch_bounds__(kOctThreads)
refine_flags_kernel(const uint8_t* __restrict__ action, int64_t slots, uint8_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (t >= slots) return;
    const uint8_t a = action[t >> 3];
    flags[t] = a == 2 || (a == 1 && (t & 7) == 0);
}

// one thread per (slot, chunk of four row values); a set slot is an output leaf.  Chunk 0 also writes
// the leaf's id and where it came from.  The row is moved as integers, bit for bit: 16 bytes at a time
// when kVector (channels a multiple of 4, both arrays 16-byte aligned), word by word otherwise (the
// file-layout SH rows have 13 and 28 channels, and a sliced array need not be aligned).
template <bool kVector>
__global__ void __launch_bounds__(kOctThreads)
refine_scatter_kernel(const uint8_t* __restrict__ action, const uint8_t* __restrict__ flags,
                      const int* __restrict__ offsets, const int64_t* __restrict__ leaf_ids,
                      const uint32_t* __restrict__ rows, int64_t slots, int channels, int chunks,
                      int64_t out_leaves, int64_t* __restrict__ ids_out,
                      uint32_t* __restrict__ rows_out, int32_t* __restrict__ parent) {
    const int64_t t = (int64_t)blockIdx.x * kOctThreads + threadIdx.x;
    if (t >= slots * chunks) return;
    const int64_t slot = t / chunks;
    const int chunk = (int)(t - slot * chunks);
    if (!flags[slot]) return;
    const int64_t o = offsets[slot];
    if (o >= out_leaves) return;   // the caller sized the outputs by the scan's total: never taken
    const int64_t leaf = slot >> 3;
    if (chunk == 0) {
        const int64_t id = leaf_ids[leaf];
        ids_out[o] = action[leaf] == 2 ? 8 * id + 1 + (slot & 7) : id;
        parent[o] = (int32_t)leaf;
    }
    if (kVector) {
        // chunk < channels / 4 here (chunks == channels / 4 >= 1)
        reinterpret_cast<uint4*>(rows_out)[o * chunks + chunk] =
            reinterpret_cast<const uint4*>(rows)[leaf * chunks + chunk];
    } else {
        const int end = min(4 * chunk + 4, channels);
        for (int c = 4 * chunk; c < end; ++c) rows_out[o * channels + c] = rows[leaf * channels + c];
    }
}

// composite.hip: activations and sigma * side > tau of one chunk
void launch_octree_density_flags(const float* logits, int64_t count, float tau, float side,
                                 float* activated, uint8_t* flags, hipStream_t stream);

// the K12b/c flag scan for the other octree files (octree_cells.h)
int octree_scan_flags(const uint8_t* flags, int64_t n, int* tile_sums, int* offsets, int* total,
                      hipStream_t stream) {
    return scan_flags(flags, n, tile_sums, offsets, total, stream);
}

// the select tail of K16b and K23 (octree_cells.h)
int octree_select_flagged(const uint8_t* flags, const float* rows, int64_t first_code,
                          int64_t count, int* offsets, int* tile_sums, int* codes_out,
                          float* data_out, int* total, hipStream_t stream) {
    if (int err = scan_flags(flags, count, tile_sums, offsets, total, stream)) return err;
    hipLaunchKernelGGL(density_scatter_kernel, dim3(oct_blocks(count)), dim3(kOctThreads), 0,
                       stream, flags, offsets, (const float4*)rows, first_code, count, codes_out,
                       (float4*)data_out);
    return 0;
}

}  // namespace ffn

using namespace ffn;

static const int64_t kOctMaxPoints = ((int64_t)1 << 31) - kScanTile;

extern "C" int64_t ffn_octree_scan_tiles(int64_t n) { return n < 0 ? -1 : scan_tiles(n); }

extern "C" int ffn_octree_max_depth(void) { return kOctMaxDepth; }

extern "C" int64_t ffn_octree_max_points(void) { return kOctMaxPoints; }

extern "C" int ffn_octree_surface_points(const float* alpha, const float* depth, const float* starts,
                                         const float* directions, const float* color, int64_t n,
                                         int channels, float threshold, uint8_t* flags,
                                         int* offsets, int* tile_sums, float* out_positions,
                                         float* out_colors, int* count, void* stream) {
    if (n < 1 || n > kOctMaxPoints || channels < 0)
        return fail_arg("ffn_octree_surface_points: shape (1 <= n < 2^31, channels >= 0)");
    if (!alpha || !depth || !starts || !directions || !flags || !offsets || !tile_sums ||
        !out_positions || !count || (channels > 0 && (!color || !out_colors)))
        return fail_arg("ffn_octree_surface_points: null argument");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(surface_flags_kernel, dim3(oct_blocks(n)), dim3(kOctThreads), 0, s, alpha, n,
                       threshold, flags);
    if (int err = scan_flags(flags, n, tile_sums, offsets, count, s)) return err;
    hipLaunchKernelGGL(surface_scatter_kernel, dim3(oct_blocks(n)), dim3(kOctThreads), 0, s, flags,
                       offsets, starts, directions, depth, color, n, channels, out_positions,
                       out_colors);
    return check_launch("ffn_octree_surface_points");
}

extern "C" int ffn_octree_path_codes(const float* positions, int64_t n, float center_x,
                                     float center_y, float center_z, float scale, int depth,
                                     int* codes, void* stream) {
    if (n < 1 || n > kOctMaxPoints || depth < 1 || depth > kOctMaxDepth)
        return fail_arg("ffn_octree_path_codes: shape (1 <= n < 2^31, 1 <= depth <= 11)");
    if (!positions || !codes) return fail_arg("ffn_octree_path_codes: null argument");
    hipLaunchKernelGGL(path_codes_kernel, dim3(oct_blocks(n)), dim3(kOctThreads), 0,
                       (hipStream_t)stream, positions, n, center_x, center_y, center_z, scale,
                       depth, codes);
    return check_launch("ffn_octree_path_codes");
}

extern "C" int ffn_octree_structure(const int* sorted_codes, const int64_t* perm, int64_t n,
                                    int depth, int64_t min_leaf_size, int64_t* leaf_sorted,
                                    int* count_sorted, int64_t* leaf_of_point, uint8_t* flags,
                                    int* offsets, int* tile_sums, int64_t* leaf_ids,
                                    int64_t* leaf_start, int* leaf_count, int* num_leaves,
                                    void* stream) {
    if (n < 1 || n > kOctMaxPoints || depth < 1 || depth > kOctMaxDepth)
        return fail_arg("ffn_octree_structure: shape (1 <= n < 2^31, 1 <= depth <= 11)");
    if (!sorted_codes || !perm || !leaf_sorted || !count_sorted || !leaf_of_point || !flags ||
        !offsets || !tile_sums || !leaf_ids || !leaf_start || !leaf_count || !num_leaves)
        return fail_arg("ffn_octree_structure: null argument");
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(oct_blocks(n)), block(kOctThreads);
    hipLaunchKernelGGL(assign_kernel, grid, block, 0, s, sorted_codes, perm, n, depth,
                       min_leaf_size, leaf_sorted, count_sorted, leaf_of_point);
    hipLaunchKernelGGL(leaf_heads_kernel, grid, block, 0, s, leaf_sorted, n, flags);
    if (int err = scan_flags(flags, n, tile_sums, offsets, num_leaves, s)) return err;
    hipLaunchKernelGGL(leaf_gather_kernel, grid, block, 0, s, flags, offsets, leaf_sorted,
                       count_sorted, n, leaf_ids, leaf_start, leaf_count);
    return check_launch("ffn_octree_structure");
}

extern "C" int ffn_octree_interior_nodes(const int64_t* leaf_ids, int64_t num_leaves, int depth,
                                         uint8_t* flags, int* offsets, int* tile_sums,
                                         int64_t* node_ids, int* num_nodes, void* stream) {
    const int levels = depth - 1;
    if (num_leaves < 1 || depth < 2 || depth > kOctMaxDepth ||
        num_leaves * levels > kOctMaxPoints)
        return fail_arg("ffn_octree_interior_nodes: shape (num_leaves >= 1, 2 <= depth <= 11)");
    if (!leaf_ids || !flags || !offsets || !tile_sums || !node_ids || !num_nodes)
        return fail_arg("ffn_octree_interior_nodes: null argument");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t m = num_leaves * levels;
    hipLaunchKernelGGL(ancestor_flags_kernel, dim3(oct_blocks(m)), dim3(kOctThreads), 0, s,
                       leaf_ids, num_leaves, levels, flags);
    if (int err = scan_flags(flags, m, tile_sums, offsets, num_nodes, s)) return err;
    hipLaunchKernelGGL(ancestor_gather_kernel, dim3(oct_blocks(m)), dim3(kOctThreads), 0, s, flags,
                       offsets, leaf_ids, num_leaves, levels, node_ids);
    return check_launch("ffn_octree_interior_nodes");
}

extern "C" int ffn_octree_leaf_means(const float* data, int64_t n, int channels, const int64_t* perm,
                                     const int64_t* leaf_start, const int* leaf_count,
                                     int64_t num_leaves, float* leaf_data, void* stream) {
    if (n < 1 || channels < 1 || num_leaves < 1 || num_leaves > kOctMaxPoints)
        return fail_arg("ffn_octree_leaf_means: shape");
    if (!data || !perm || !leaf_start || !leaf_count || !leaf_data)
        return fail_arg("ffn_octree_leaf_means: null argument");
    const int per_block = kOctThreads / kWave;
    hipLaunchKernelGGL(leaf_means_kernel, dim3((unsigned)((num_leaves + per_block - 1) / per_block)),
                       dim3(kOctThreads), 0, (hipStream_t)stream, data, channels, perm, leaf_start,
                       leaf_count, num_leaves, leaf_data);
    return check_launch("ffn_octree_leaf_means");
}

extern "C" int ffn_octree_query(const float* positions, int64_t n, float scale,
                                const int64_t* node_index, int64_t num_nodes,
                                const int64_t* leaf_index, int64_t num_leaves, int64_t* result,
                                void* stream) {
    if (n < 1 || n > kOctMaxPoints || num_leaves < 1 || num_nodes < 0)
        return fail_arg("ffn_octree_query: shape (n >= 1, num_leaves >= 1)");
    if (!positions || !leaf_index || !result || (num_nodes > 0 && !node_index))
        return fail_arg("ffn_octree_query: null argument");
    hipLaunchKernelGGL(query_kernel, dim3(oct_blocks(n)), dim3(kOctThreads), 0, (hipStream_t)stream,
                       positions, n, scale, node_index, num_nodes, leaf_index, num_leaves, result);
    return check_launch("ffn_octree_query");
}

extern "C" int ffn_octree_leaf_geometry(const int64_t* leaf_index, int64_t num_leaves, float scale,
                                        float* centers, int* depths, void* stream) {
    if (num_leaves < 1 || num_leaves > kOctMaxPoints)
        return fail_arg("ffn_octree_leaf_geometry: num_leaves >= 1");
    if (!leaf_index || !centers || !depths) return fail_arg("ffn_octree_leaf_geometry: null argument");
    hipLaunchKernelGGL(leaf_geometry_kernel, dim3(oct_blocks(num_leaves)), dim3(kOctThreads), 0,
                       (hipStream_t)stream, leaf_index, num_leaves, scale, centers, depths);
    return check_launch("ffn_octree_leaf_geometry");
}

static inline bool misaligned16(const void* a, const void* b) {
    return (((uintptr_t)a | (uintptr_t)b) & 15) != 0;
}

extern "C" int ffn_octree_cell_centers(int64_t first_code, int64_t count, float center_x,
                                       float center_y, float center_z, float scale, int depth,
                                       float* out, void* stream) {
    if (depth < 1 || depth > kOctMaxDepth)
        return fail_arg("ffn_octree_cell_centers: shape (1 <= depth <= 11)");
    if (count < 1 || count > kOctMaxPoints || first_code < 0 ||
        first_code + count > ((int64_t)1 << (3 * (depth - 1))))
        return fail_arg("ffn_octree_cell_centers: shape (count >= 1, codes inside "
                        "[0, 8^(depth-1)))");
    if (!out) return fail_arg("ffn_octree_cell_centers: null argument");
    hipLaunchKernelGGL(cell_centers_kernel, dim3(oct_blocks(count)), dim3(kOctThreads), 0,
                       (hipStream_t)stream, first_code, count, center_x, center_y, center_z, scale,
                       depth, out);
    return check_launch("ffn_octree_cell_centers");
}

extern "C" int ffn_octree_density_select(const float* logits, int64_t first_code, int64_t count,
                                         float tau, float side, int depth, uint8_t* flags,
                                         int* offsets, int* tile_sums, float* activated,
                                         int* codes_out, float* data_out, int* total,
                                         void* stream) {
    if (depth < 1 || depth > kOctMaxDepth)
        return fail_arg("ffn_octree_density_select: shape (1 <= depth <= 11)");
    if (count < 1 || count > kOctMaxPoints || first_code < 0 ||
        first_code + count > ((int64_t)1 << (3 * (depth - 1))))
        return fail_arg("ffn_octree_density_select: shape (count >= 1, codes inside "
                        "[0, 8^(depth-1)))");
    if (!logits || !flags || !offsets || !tile_sums || !activated || !codes_out || !data_out ||
        !total)
        return fail_arg("ffn_octree_density_select: null argument");
    if (misaligned16(logits, activated) || misaligned16(data_out, nullptr))
        return fail_arg("ffn_octree_density_select: logits, activated and data_out must be "
                        "16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    launch_octree_density_flags(logits, count, tau, side, activated, flags, s);
    if (int err = octree_select_flagged(flags, activated, first_code, count, offsets, tile_sums,
                                        codes_out, data_out, total, s))
        return err;
    return check_launch("ffn_octree_density_select");
}

extern "C" int ffn_octree_merge_level(const int* codes, const int* levels, const float* data,
                                      int64_t n, int level, int depth, float rgb_tol,
                                      float sigma_tol, uint8_t* merge, uint8_t* flags, int* offsets,
                                      int* tile_sums, int* codes_out, int* levels_out,
                                      float* data_out, int* total, void* stream) {
    if (depth < 2 || depth > kOctMaxDepth || level < 1 || level > depth - 1)
        return fail_arg("ffn_octree_merge_level: shape (2 <= depth <= 11, 1 <= level < depth)");
    if (n < 1 || n > kOctMaxPoints) return fail_arg("ffn_octree_merge_level: shape (1 <= n < 2^31)");
    if (!(rgb_tol >= 0.0f) || !(sigma_tol >= 0.0f))   // NaN fails too
        return fail_arg("ffn_octree_merge_level: tolerances must be >= 0");
    if (!codes || !levels || !data || !merge || !flags || !offsets || !tile_sums || !codes_out ||
        !levels_out || !data_out || !total)
        return fail_arg("ffn_octree_merge_level: null argument");
    if (misaligned16(data, data_out))
        return fail_arg("ffn_octree_merge_level: data and data_out must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(oct_blocks(n)), block(kOctThreads);
    hipLaunchKernelGGL(merge_heads_kernel, grid, block, 0, s, codes, levels, (const float4*)data, n,
                       level, depth, rgb_tol, sigma_tol, merge);
    hipLaunchKernelGGL(merge_flags_kernel, grid, block, 0, s, codes, levels, merge, n, level, depth,
                       flags);
    if (int err = scan_flags(flags, n, tile_sums, offsets, total, s)) return err;
    hipLaunchKernelGGL(merge_scatter_kernel, grid, block, 0, s, flags, offsets, merge, codes, levels,
                       (const float4*)data, n, codes_out, levels_out, (float4*)data_out);
    return check_launch("ffn_octree_merge_level");
}

extern "C" int ffn_octree_refine_count(const uint8_t* action, int64_t num_leaves, uint8_t* flags,
                                       int* offsets, int* tile_sums, int* total, void* stream) {
    if (num_leaves < 1 || num_leaves > kOctMaxPoints / 8)
        return fail_arg("ffn_octree_refine_count: shape (1 <= num_leaves, 8 num_leaves < 2^31)");
    if (!action || !flags || !offsets || !tile_sums || !total)
        return fail_arg("ffn_octree_refine_count: null argument");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t slots = 8 * num_leaves;
    hipLaunchKernelGGL(refine_flags_kernel, dim3(oct_blocks(slots)), dim3(kOctThreads), 0, s, action,
                       slots, flags);
    return scan_flags(flags, slots, tile_sums, offsets, total, s);
}

extern "C" int ffn_octree_refine_scatter(const uint8_t* action, const uint8_t* flags,
                                         const int* offsets, const int64_t* leaf_ids,
                                         const float* rows, int64_t num_leaves, int channels,
                                         int64_t out_leaves, int64_t* ids_out, float* rows_out,
                                         int32_t* parent, void* stream) {
    if (num_leaves < 1 || num_leaves > kOctMaxPoints / 8 || channels < 0 || channels > 1024 ||
        out_leaves < 1 || out_leaves > 8 * num_leaves)
        return fail_arg("ffn_octree_refine_scatter: shape (1 <= num_leaves, 8 num_leaves < 2^31, "
                        "0 <= channels <= 1024, 1 <= out_leaves <= 8 num_leaves)");
    if (!action || !flags || !offsets || !leaf_ids || !ids_out || !parent ||
        (channels > 0 && (!rows || !rows_out)))
        return fail_arg("ffn_octree_refine_scatter: null argument");
    const bool vector = channels > 0 && channels % 4 == 0 && !misaligned16(rows, rows_out);
    const int chunks = channels == 0 ? 1 : (channels + 3) / 4;
    const int64_t slots = 8 * num_leaves;
    const int64_t blocks = (slots * chunks + kOctThreads - 1) / kOctThreads;
    if (blocks >= ((int64_t)1 << 31) / kOctThreads * 2)      // blocks * threads < 2^32
        return fail_arg("ffn_octree_refine_scatter: 8 num_leaves * ceil(channels / 4) < 2^32");
    const hipStream_t s = (hipStream_t)stream;
    if (vector)
        hipLaunchKernelGGL(refine_scatter_kernel<true>, dim3((unsigned)blocks), dim3(kOctThreads), 0,
                           s, action, flags, offsets, leaf_ids, (const uint32_t*)rows, slots,
                           channels, chunks, out_leaves, ids_out, (uint32_t*)rows_out, parent);
    else
        hipLaunchKernelGGL(refine_scatter_kernel<false>, dim3((unsigned)blocks), dim3(kOctThreads),
                           0, s, action, flags, offsets, leaf_ids, (const uint32_t*)rows, slots,
                           channels, chunks, out_leaves, ids_out, (uint32_t*)rows_out, parent);
    return check_launch("ffn_octree_refine_scatter");
}
