// K20  A total-variation prior between the leaves of a sparse octree that touch across a face.
//
//   K20a octree_neighbors   per (leaf, direction -x +x -y +y -z +z) the leaf on the other side of that
//                           face, integers only: the leaf's id gives its level d and its cell on the
//                           2^d grid; the cell one step along the axis is looked up from the root
//                           down with the binary searches of K12j (csrc/octree.hip).  A leaf found on
//                           the way is of equal size or coarser; an id in neither index is empty
//                           space (-1); an id that is still interior at level d means finer leaves on
//                           the other side (-1: they hold the adjacency from their side).
//   K20b tv_edges           one thread per (edge, quad of four columns): two 16-byte loads,
//                             d = a - b,  s = sqrtf(fmaf(d, d, eps * eps)),
//                             term = (s - eps) * scale_c,  derivative = (d / s) * scale_c,
//                           scale_c = lambda_c / (float)E made on the host in f32.  The derivative quad
//                           goes to an E * stride / 4 float4 buffer, the terms of a workgroup through
//                           a fixed shuffle / LDS tree into one partial.
//        tv_energy          one workgroup: thread t adds its contiguous share of the partials in index
//                           order, thread 0 the 256 shares in index order
//   K20c tv_reduce_first    the per-leaf sum of sign * derivative over the leaf's incidences, in the
//        tv_reduce          shape of K17b-4 / K17b-5 (csrc/octree_grad.hip) with K19b's compact rows:
//        tv_finish          level 0 adds runs of kTvChunk incidences through the plan's sorted order,
//                           further levels runs of kTvChunk partial sums, the finish writes every row
//                           (out = sum, or out = out + sum with accumulate).  Leaf l's run q of every
//                           level lives at row seg_base[l] + q, seg_base[l] = seg_lo[l] / 16 + (leaves
//                           with incidences before l): 2 E / 16 + L + 1 rows hold every level.
//
// No float atomics, no read-back.  The plan (edges, incidences sorted by leaf, ranges) is made once
// per tree by the caller.  Every index read from a plan array is held against its range before it
// is used: a plan of another tree gives wrong sums, never an access outside the buffers.
#include "common.h"

namespace ffn {

constexpr int kTvChunk = 16;            // terms added by one thread
constexpr int kTvMaxLevels = 21;        // 3 * 21 bits of path below the root in an int64 id
constexpr int kTvMaxStride = 64;
constexpr int kTvEnergyThreads = 256;

__device__ __forceinline__ int64_t tv_lower_bound(const int64_t* __restrict__ ids, int64_t n,
                                                  int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------- K20a
__global__ void __launch_bounds__(256)
octree_neighbors_kernel(const int64_t* __restrict__ node_index, int64_t num_nodes,
                        const int64_t* __restrict__ leaf_index, int64_t num_leaves,
                        int32_t* __restrict__ neighbors) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= num_leaves * 6) return;
    const int64_t leaf = t / 6;
    const int dir = (int)(t - leaf * 6);
    // the leaf's level and cell: child digits 4 [x] + 2 [y] + [z], the leaf's own in the low bits
    int64_t id = leaf_index[leaf];
    int64_t cell[3] = {0, 0, 0};
    int d = 0;
    while (id > 0 && d < kTvMaxLevels) {
        const int child = (int)((id - 1) & 7);
        cell[0] |= (int64_t)((child >> 2) & 1) << d;
        cell[1] |= (int64_t)((child >> 1) & 1) << d;
        cell[2] |= (int64_t)(child & 1) << d;
        id = (id - 1) >> 3;
        ++d;
    }
    int32_t result = -1;
    const int axis = dir >> 1;
    cell[axis] += (dir & 1) ? 1 : -1;
    if (id == 0 && cell[axis] >= 0 && cell[axis] < ((int64_t)1 << d)) {
        int64_t walk = 0;
        for (int level = 1; level <= d; ++level) {
            const int bit = d - level;
            const int child = (int)(4 * ((cell[0] >> bit) & 1) + 2 * ((cell[1] >> bit) & 1) +
                                    ((cell[2] >> bit) & 1));
            walk = 8 * walk + 1 + child;
            int64_t j = tv_lower_bound(leaf_index, num_leaves, walk);
            if (j < num_leaves && leaf_index[j] == walk) { result = (int32_t)j; break; }
            j = tv_lower_bound(node_index, num_nodes, walk);
            if (j == num_nodes || node_index[j] != walk) break;      // empty space
        }
    }
    neighbors[t] = result;
}

// ---------------------------------------------------------------------------------- K20b
struct TvScale { float c[kTvMaxStride]; };      // lambda_c / E per column

__device__ __forceinline__ void tv_column(float a, float b, float eps, float eps2, float scale,
                                          float& term, float& deriv) {
    const float d = a - b;
    const float s = sqrtf(fmaf(d, d, eps2));
    term = (s - eps) * scale;
    deriv = (d / s) * scale;
}

__global__ void __launch_bounds__(256)
tv_edges_kernel(const float4* __restrict__ rows, int64_t num_leaves, int quads,
                const int32_t* __restrict__ edge_i, const int32_t* __restrict__ edge_j,
                int64_t num_edges, TvScale scale, float eps, float4* __restrict__ deriv,
                float* __restrict__ partials) {
    __shared__ float lds[4];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float sum = 0.0f;
    if (t < num_edges * quads) {
        const int64_t e = t / quads;
        const int k = (int)(t - e * quads);
        const int64_t i = edge_i[e], j = edge_j[e];
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= 0 && i < num_leaves && j >= 0 && j < num_leaves) {
            const float4 a = rows[i * quads + k], b = rows[j * quads + k];
            const float eps2 = eps * eps;
            float tx, ty, tz, tw;
            tv_column(a.x, b.x, eps, eps2, scale.c[4 * k + 0], tx, g.x);
            tv_column(a.y, b.y, eps, eps2, scale.c[4 * k + 1], ty, g.y);
            tv_column(a.z, b.z, eps, eps2, scale.c[4 * k + 2], tz, g.z);
            tv_column(a.w, b.w, eps, eps2, scale.c[4 * k + 3], tw, g.w);
            sum = ((tx + ty) + tz) + tw;
        }
        deriv[t] = g;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ void __launch_bounds__(kTvEnergyThreads)
tv_energy_kernel(const float* __restrict__ partials, int64_t count, float* __restrict__ value) {
    __shared__ float shares[kTvEnergyThreads];
    const int64_t per = (count + kTvEnergyThreads - 1) / kTvEnergyThreads;
    const int64_t first = per * threadIdx.x;
    const int64_t last = first + per < count ? first + per : count;
    float acc = 0.0f;
    for (int64_t i = first; i < last; ++i) acc += partials[i];
    shares[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.0f;
        for (int k = 0; k < kTvEnergyThreads; ++k) total += shares[k];
        *value = total;
    }
}

// ---------------------------------------------------------------------------------- K20c
// The run of sorted position p and quad k at this level, or false: p's leaf l, q = p - seg_lo[l] the
// run's number, [first, end) its terms (positions of the sorted incidences at level 0, rows after).
struct TvRun { int64_t base; int q; int len; };

__device__ __forceinline__ bool tv_run(int64_t p, const int32_t* __restrict__ inc_leaf,
                                       int64_t incidences, int64_t num_leaves,
                                       const int32_t* __restrict__ seg_lo,
                                       const int32_t* __restrict__ seg_hi,
                                       const int32_t* __restrict__ seg_base, int level,
                                       int64_t row_capacity, TvRun& run, int& lo) {
    const int64_t l = inc_leaf[p];
    if (l < 0 || l >= num_leaves) return false;
    lo = seg_lo[l];
    const int hi = seg_hi[l];
    if (lo < 0 || hi < lo || hi > incidences) return false;
    int len = hi - lo;
    for (int j = 0; j < level; ++j) len = (len + kTvChunk - 1) / kTvChunk;
    const int64_t q = p - lo;
    if (q < 0 || q >= (len + kTvChunk - 1) / kTvChunk) return false;
    run.base = seg_base[l];
    run.q = (int)q;
    run.len = len;
    // the rows this run reads (levels >= 1) and the one it writes
    if (run.base < 0 || run.base + (level == 0 ? q + 1 : (int64_t)len) > row_capacity) return false;
    return true;
}

__global__ void __launch_bounds__(256)
tv_reduce_first_kernel(const int32_t* __restrict__ inc_leaf, const int32_t* __restrict__ inc_code,
                       int64_t incidences, int quads, const float4* __restrict__ deriv,
                       int64_t num_edges, int64_t num_leaves, const int32_t* __restrict__ seg_lo,
                       const int32_t* __restrict__ seg_hi, const int32_t* __restrict__ seg_base,
                       float4* __restrict__ dst, int64_t row_capacity) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= incidences * quads) return;
    const int64_t p = t / quads;
    const int k = (int)(t - p * quads);
    TvRun run;
    int lo;
    if (!tv_run(p, inc_leaf, incidences, num_leaves, seg_lo, seg_hi, seg_base, 0, row_capacity, run,
                lo))
        return;
    const int64_t first = (int64_t)lo + (int64_t)run.q * kTvChunk;
    const int64_t end = first + kTvChunk < (int64_t)lo + run.len ? first + kTvChunk
                                                                 : (int64_t)lo + run.len;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = first; i < end; ++i) {
        const int32_t code = inc_code[i];           // 2 * edge + (the leaf is the edge's j)
        const int64_t e = code >> 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (code >= 0 && e < num_edges) v = deriv[e * quads + k];
        if (code & 1) { v.x = -v.x; v.y = -v.y; v.z = -v.z; v.w = -v.w; }
        if (i == first) {
            acc = v;                                // K17b starts from the first term, not from 0
        } else {
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    dst[(run.base + run.q) * quads + k] = acc;
}

__global__ void __launch_bounds__(256)
tv_reduce_kernel(const int32_t* __restrict__ inc_leaf, int64_t incidences, int quads,
                 const float4* __restrict__ src, float4* __restrict__ dst, int64_t num_leaves,
                 const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                 const int32_t* __restrict__ seg_base, int level, int64_t row_capacity) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= incidences * quads) return;
    const int64_t p = t / quads;
    const int k = (int)(t - p * quads);
    TvRun run;
    int lo;
    if (!tv_run(p, inc_leaf, incidences, num_leaves, seg_lo, seg_hi, seg_base, level, row_capacity,
                run, lo))
        return;
    const int64_t first = run.base + (int64_t)run.q * kTvChunk;
    const int64_t last = first + kTvChunk < run.base + run.len ? first + kTvChunk
                                                               : run.base + run.len;
    float4 acc = src[first * quads + k];
    for (int64_t i = first + 1; i < last; ++i) {
        const float4 v = src[i * quads + k];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    dst[(run.base + run.q) * quads + k] = acc;
}

// every quad of every row: the leaf's sum, +0 for a leaf without an incidence (+ 0.0f as K17b-5: a
// sum of -0 ends at +0); with accumulate one more add per element
__global__ void __launch_bounds__(256)
tv_finish_kernel(const float4* __restrict__ sums, int quads, const int32_t* __restrict__ seg_lo,
                 const int32_t* __restrict__ seg_hi, const int32_t* __restrict__ seg_base,
                 int64_t num_leaves, int64_t row_capacity, int accumulate,
                 float4* __restrict__ d_rows) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= num_leaves * quads) return;
    const int64_t l = idx / quads;
    const int k = (int)(idx - l * quads);
    const int64_t base = seg_base[l];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (seg_hi[l] > seg_lo[l] && base >= 0 && base < row_capacity) v = sums[base * quads + k];
    v.x += 0.0f; v.y += 0.0f; v.z += 0.0f; v.w += 0.0f;
    if (accumulate) {
        const float4 o = d_rows[idx];
        v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
    }
    d_rows[idx] = v;
}

struct TvWorkspace {
    float4* deriv;          // E * quads
    float* partials;        // workgroups of K20b
    float4* rows[2];        // row_capacity * quads each
    int64_t row_capacity;
    int64_t blocks;
};

static inline int64_t tv_align256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

static int64_t tv_layout(int64_t num_leaves, int64_t num_edges, int stride, TvWorkspace* ws,
                         char* base) {
    const int64_t quads = stride / 4;
    const int64_t blocks = (num_edges * quads + 255) / 256;
    const int64_t row_capacity = 2 * num_edges / kTvChunk + num_leaves + 1;
    const int64_t sizes[4] = {16 * num_edges * quads, 4 * (blocks > 0 ? blocks : 1),
                              16 * row_capacity * quads, 16 * row_capacity * quads};
    TvWorkspace scratch;
    TvWorkspace* w = ws != nullptr ? ws : &scratch;
    void** slots[4] = {(void**)&w->deriv, (void**)&w->partials, (void**)&w->rows[0],
                       (void**)&w->rows[1]};
    int64_t off = 0;
    for (int r = 0; r < 4; ++r) {
        *slots[r] = base != nullptr ? base + off : nullptr;
        off += tv_align256(sizes[r]);
    }
    w->row_capacity = row_capacity;
    w->blocks = blocks;
    return off;
}

static inline bool tv_shape(int64_t num_leaves, int64_t num_edges, int stride) {
    return num_leaves >= 1 && num_leaves < ((int64_t)1 << 31) && num_edges >= 0 &&
           num_edges <= 6 * num_leaves && 2 * num_edges < ((int64_t)1 << 31) && stride >= 4 &&
           stride <= kTvMaxStride && stride % 4 == 0;
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_octree_neighbors(const int64_t* node_index, int64_t num_nodes,
                                    const int64_t* leaf_index, int64_t num_leaves,
                                    int32_t* neighbors, void* stream) {
    if (num_leaves < 1 || num_leaves >= ((int64_t)1 << 31) || num_nodes < 0)
        return fail_arg("ffn_octree_neighbors: shape (1 <= num_leaves < 2^31, num_nodes >= 0)");
    if (!leaf_index || !neighbors || (num_nodes > 0 && !node_index))
        return fail_arg("ffn_octree_neighbors: null argument");
    hipLaunchKernelGGL(octree_neighbors_kernel, dim3((unsigned)((num_leaves * 6 + 255) / 256)),
                       dim3(256), 0, (hipStream_t)stream, node_index, num_nodes, leaf_index,
                       num_leaves, neighbors);
    return check_launch("ffn_octree_neighbors");
}

extern "C" int64_t ffn_octree_tv_workspace_bytes(int64_t num_leaves, int64_t num_edges,
                                                 int stride) {
    if (!tv_shape(num_leaves, num_edges, stride)) {
        fail_arg("ffn_octree_tv_workspace_bytes: shape (1 <= num_leaves < 2^31, 0 <= num_edges <= "
                 "6 num_leaves, 2 num_edges < 2^31, stride a multiple of 4 in 4 .. 64)");
        return -1;
    }
    return tv_layout(num_leaves, num_edges, stride, nullptr, nullptr);
}

extern "C" int ffn_octree_tv(const float* rows, int64_t num_leaves, int stride,
                             const int32_t* edge_i, const int32_t* edge_j, int64_t num_edges,
                             const int32_t* inc_leaf, const int32_t* inc_code,
                             const int32_t* seg_lo, const int32_t* seg_hi,
                             const int32_t* seg_base, int64_t longest, const float* lambda,
                             float eps, float* value, float* d_rows, int accumulate,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "ffn_octree_tv";
    if (!tv_shape(num_leaves, num_edges, stride))
        return fail_arg("ffn_octree_tv: shape (1 <= num_leaves < 2^31, 0 <= num_edges <= 6 "
                        "num_leaves, 2 num_edges < 2^31, stride a multiple of 4 in 4 .. 64)");
    if (!(eps > 0.0f) || eps * eps == 0.0f || !(eps * eps < 3.0e38f))
        return fail_arg("ffn_octree_tv: eps > 0 (and eps * eps a finite, non-zero f32)");
    if (!rows || !value || !lambda || !seg_lo || !seg_hi || !seg_base)
        return fail_arg("ffn_octree_tv: null argument");
    if (num_edges > 0 && (!edge_i || !edge_j || !inc_leaf || !inc_code || !workspace))
        return fail_arg("ffn_octree_tv: null argument");
    if (accumulate && !d_rows) return fail_arg("ffn_octree_tv: accumulate needs d_rows");
    if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)d_rows & 15) != 0 ||
        ((uintptr_t)workspace & 15) != 0)
        return fail_arg("ffn_octree_tv: rows, d_rows and workspace must be 16-byte aligned");
    if (longest < 0 || longest > 2 * num_edges || (num_edges > 0 && longest < 1))
        return fail_arg("ffn_octree_tv: longest is the longest incidence list, 1 .. 2 num_edges");
    for (int c = 0; c < stride; ++c)
        if (!(lambda[c] >= 0.0f) || !(lambda[c] < 3.0e38f))
            return fail_arg("ffn_octree_tv: the weights are finite and >= 0");
    if (num_edges > 0 &&
        workspace_bytes < tv_layout(num_leaves, num_edges, stride, nullptr, nullptr))
        return fail_arg("ffn_octree_tv: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int quads = stride / 4;
    if (num_edges == 0) {
        (void)hipMemsetAsync(value, 0, 4, st);
        if (d_rows && !accumulate)
            (void)hipMemsetAsync(d_rows, 0, 4 * (int64_t)stride * num_leaves, st);
        return check_launch(who);
    }
    TvWorkspace ws;
    tv_layout(num_leaves, num_edges, stride, &ws, (char*)workspace);
    TvScale scale;
    for (int c = 0; c < kTvMaxStride; ++c)
        scale.c[c] = c < stride ? lambda[c] / (float)num_edges : 0.0f;

    hipLaunchKernelGGL(tv_edges_kernel, dim3((unsigned)ws.blocks), dim3(256), 0, st,
                       (const float4*)rows, num_leaves, quads, edge_i, edge_j, num_edges, scale, eps,
                       ws.deriv, ws.partials);
    hipLaunchKernelGGL(tv_energy_kernel, dim3(1), dim3(kTvEnergyThreads), 0, st, ws.partials,
                       ws.blocks, value);
    if (!d_rows) return check_launch(who);

    const int64_t incidences = 2 * num_edges;
    const unsigned over = (unsigned)((incidences * quads + 255) / 256);
    int levels = 1;
    for (int64_t reach = kTvChunk; reach < longest; reach *= kTvChunk) ++levels;
    hipLaunchKernelGGL(tv_reduce_first_kernel, dim3(over), dim3(256), 0, st, inc_leaf, inc_code,
                       incidences, quads, ws.deriv, num_edges, num_leaves, seg_lo, seg_hi, seg_base,
                       ws.rows[0], ws.row_capacity);
    const float4* src = ws.rows[0];
    for (int level = 1; level < levels; ++level) {
        float4* dst = ws.rows[level & 1];
        hipLaunchKernelGGL(tv_reduce_kernel, dim3(over), dim3(256), 0, st, inc_leaf, incidences,
                           quads, src, dst, num_leaves, seg_lo, seg_hi, seg_base, level,
                           ws.row_capacity);
        src = dst;
    }
    hipLaunchKernelGGL(tv_finish_kernel, dim3((unsigned)((num_leaves * quads + 255) / 256)),
                       dim3(256), 0, st, src, quads, seg_lo, seg_hi, seg_base, num_leaves,
                       ws.row_capacity, accumulate, (float4*)d_rows);
    return check_launch(who);
}
