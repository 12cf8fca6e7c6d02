// K17b  Per-leaf sums of the gradient walk's entries (K17a, csrc/octree_walk.hip) without float
// atomics, and K17c, the projection after the optimiser step.
//
// K17a leaves one entry per (ray, taken leaf): a float4 (d rgb, d sigma) and the leaf's number,
// ray-major at offsets[ray] + k -- a place that depends on the inputs only.  d_leaf_data[l] is the
// sum of the entries of leaf l.  As K10b (csrc/voxels.hip) this is the store-and-sum form: the
// entries are brought into a fixed order, leaf by leaf, and added in a fixed tree, so that the
// same inputs give the same bits on every call.  Unlike K10b-4, which ranks an entry by reading
// its whole list, nothing here reads a list longer than a fixed chunk -- one leaf may be taken by
// every ray (a root-only tree):
//
//   K17b-1 grad_scan_*      exclusive scan of the per-ray counts (the three kernels of K10b-2);
//                           the total E is read back once, to hold it against the caller's
//                           workspace and to size the launches below
//   K17b-2 grad_sort_*      stable LSD radix sort of (leaf, entry) by leaf, 8 bits a pass,
//                           ceil(bits(L - 1) / 8) passes: per tile of 1024 entries a digit histogram
//                           (integer LDS atomics), a scan of the digit-major (digit, tile) table,
//                           and a scatter in which an entry's place among its tile's equal digits
//                           comes from wave ballots and a 16 x 256 table of per-wave counts.  Stable,
//                           so the entries of a leaf stay in ray order.
//   K17b-3 grad_bounds      first and one-past-last sorted position of every leaf that has entries
//   K17b-4 grad_reduce      level j: every run of kGradChunk consecutive partial sums of a leaf
//                           into one, at the leaf's own range of the other buffer; ceil(log16 n)
//                           levels, since a ray takes a leaf once
//   K17b-5 grad_finish      every row of d_leaf_data: the leaf's sum, or zeros
//
// Integer atomics appear in the tile histogram only, where their order does not matter.
#include "common.h"
#include "octree_grad.h"
#include "sh_terms.h"

namespace ffn {

constexpr int kGradChunk = 16;          // partial sums added by one thread
constexpr int kGradScanBlock = 4096;    // elements per workgroup of the scan (256 x 16)
constexpr int kSortThreads = 256;
constexpr int kSortItems = 4;
constexpr int kSortTile = kSortThreads * kSortItems;
constexpr int kSortGroups = kSortItems * (kSortThreads / 64);   // (item, wave) pairs of a tile
static const int64_t kGradMaxEntries = ((int64_t)1 << 31) - 1;

// ---------------------------------------------------------------------------------- K17b-1
__global__ void __launch_bounds__(256)
grad_scan_sums_kernel(const int32_t* __restrict__ values, int64_t m,
                      int32_t* __restrict__ block_sums) {
    __shared__ int lds[4];
    const int64_t first = (int64_t)blockIdx.x * kGradScanBlock + threadIdx.x * 16;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (first + k < m) s += values[first + k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// one workgroup: exclusive scan of the block sums in place, and the total
__global__ void __launch_bounds__(1024)
grad_scan_top_kernel(int32_t* __restrict__ block_sums, int blocks, int32_t* __restrict__ total) {
    __shared__ int part[1024];
    int carry = 0;
    for (int t0 = 0; t0 < blocks; t0 += 1024) {
        const int t = t0 + threadIdx.x;
        const int v = t < blocks ? block_sums[t] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int add = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < blocks) block_sums[t] = carry + part[threadIdx.x] - v;
        carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0 && total != nullptr) *total = carry;
}

// in place: values[i] becomes the sum of everything before it
__global__ void __launch_bounds__(256)
grad_scan_apply_kernel(int32_t* values, int64_t m, const int32_t* __restrict__ block_sums) {
    __shared__ int wave_tot[4];
    const int64_t first = (int64_t)blockIdx.x * kGradScanBlock + threadIdx.x * 16;
    int local[16];
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        local[k] = first + k < m ? values[first + k] : 0;
        s += local[k];
    }
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off);
        if (lane >= off) inc += up;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int run = block_sums[blockIdx.x] + inc - s;
    for (int w = 0; w < wave; ++w) run += wave_tot[w];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (first + k < m) values[first + k] = run;
        run += local[k];
    }
}

static void exclusive_scan(int32_t* values, int64_t m, int32_t* block_sums, int32_t* total,
                           hipStream_t st) {
    const int blocks = (int)((m + kGradScanBlock - 1) / kGradScanBlock);
    hipLaunchKernelGGL(grad_scan_sums_kernel, dim3(blocks), dim3(256), 0, st, values, m, block_sums);
    hipLaunchKernelGGL(grad_scan_top_kernel, dim3(1), dim3(1024), 0, st, block_sums, blocks, total);
    hipLaunchKernelGGL(grad_scan_apply_kernel, dim3(blocks), dim3(256), 0, st, values, m, block_sums);
}

// ---------------------------------------------------------------------------------- K17b-2
// table[digit * tiles + tile]: how many entries of the tile have that digit
__global__ void __launch_bounds__(kSortThreads)
grad_sort_hist_kernel(const int32_t* __restrict__ keys, int32_t e, int shift, int32_t tiles,
                      int32_t* __restrict__ table) {
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kSortTile + j * kSortThreads + threadIdx.x;
        if (i < e) atomicAdd(&hist[(keys[i] >> shift) & 255], 1);
    }
    __syncthreads();
    table[(int64_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// table: scanned.  The order inside a tile is (item, wave, lane), which is the entry order.
// order_in null: the entries are still where K17a put them (the first pass).
__global__ void __launch_bounds__(kSortThreads)
grad_sort_scatter_kernel(const int32_t* __restrict__ keys_in, const int32_t* __restrict__ order_in,
                         int32_t e, int shift, int32_t tiles, const int32_t* __restrict__ table,
                         int32_t* __restrict__ keys_out, int32_t* __restrict__ order_out) {
    __shared__ int groups[kSortGroups][256];
    for (int g = 0; g < kSortGroups; ++g) groups[g][threadIdx.x] = 0;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    int key[kSortItems], rank[kSortItems];
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kSortTile + j * kSortThreads + threadIdx.x;
        const bool valid = i < e;
        key[j] = valid ? keys_in[i] : 0;
        const int digit = (key[j] >> shift) & 255;
        // the lanes of this wave that hold the same digit
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1;
            const uint64_t set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        rank[j] = __popcll(peers & below);
        if (valid && rank[j] == 0) groups[j * 4 + wave][digit] = __popcll(peers);
    }
    __syncthreads();
    // per digit: the groups' counts into the groups' starts
    int run = 0;
    for (int g = 0; g < kSortGroups; ++g) {
        const int c = groups[g][threadIdx.x];
        groups[g][threadIdx.x] = run;
        run += c;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kSortTile + j * kSortThreads + threadIdx.x;
        if (i < e) {
            const int digit = (key[j] >> shift) & 255;
            const int32_t at = table[(int64_t)digit * tiles + blockIdx.x] +
                               groups[j * 4 + wave][digit] + rank[j];
            if (at >= 0 && at < e) {          // always, for a table made from these keys
                keys_out[at] = key[j];
                order_out[at] = order_in != nullptr ? order_in[i] : (int32_t)i;
            }
        }
    }
}

// ---------------------------------------------------------------------------------- K17b-3
__global__ void __launch_bounds__(256)
grad_bounds_kernel(const int32_t* __restrict__ keys, int32_t e, int32_t num_leaves,
                   int32_t* __restrict__ seg_lo, int32_t* __restrict__ seg_hi) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= e) return;
    const int32_t l = keys[p];
    if (l < 0 || l >= num_leaves) return;
    if (p == 0 || keys[p - 1] != l) seg_lo[l] = (int32_t)p;
    if (p == e - 1 || keys[p + 1] != l) seg_hi[l] = (int32_t)p + 1;
}

// ---------------------------------------------------------------------------------- K17b-4
// order: level 0 only, where src is K17a's ray-major values
__global__ void __launch_bounds__(256)
grad_reduce_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ order,
                   const float4* __restrict__ src, float4* __restrict__ dst, int32_t e,
                   int32_t num_leaves, const int32_t* __restrict__ seg_lo,
                   const int32_t* __restrict__ seg_hi, int level) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= e) return;
    const int32_t l = keys[p];
    if (l < 0 || l >= num_leaves) return;
    const int lo = seg_lo[l];
    int len = seg_hi[l] - lo;
    for (int j = 0; j < level; ++j) len = (len + kGradChunk - 1) / kGradChunk;
    const int q = (int)p - lo;
    if (q < 0 || q >= (len + kGradChunk - 1) / kGradChunk) return;
    const int first = lo + q * kGradChunk;
    const int end = min(first + kGradChunk, lo + len);
    float4 acc = order != nullptr ? src[order[first]] : src[first];
    for (int i = first + 1; i < end; ++i) {
        const float4 v = order != nullptr ? src[order[i]] : src[i];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    dst[lo + q] = acc;
}

// ---------------------------------------------------------------------------------- K17b-5
__global__ void __launch_bounds__(256)
grad_finish_kernel(const float4* __restrict__ sums, const int32_t* __restrict__ seg_lo,
                   const int32_t* __restrict__ seg_hi, int64_t num_leaves,
                   float4* __restrict__ d_leaf_data) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= num_leaves) return;
    const int lo = seg_lo[l];
    // + 0: a leaf whose only entries are those of rays that touch it (a chord of length 0, terms
    // of -0 under a negative upstream gradient) ends at +0 like a leaf without entries
    float4 v = seg_hi[l] > lo ? sums[lo] : make_float4(0.f, 0.f, 0.f, 0.f);
    v.x += 0.0f; v.y += 0.0f; v.z += 0.0f; v.w += 0.0f;
    d_leaf_data[l] = v;
}

// ---------------------------------------------------------------------------------- K17c
__global__ void __launch_bounds__(256)
octree_project_kernel(float4* __restrict__ leaf_data, int64_t num_leaves) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= num_leaves) return;
    float4 v = leaf_data[l];
    // fmaxf / fminf return the other operand for a NaN: NaN -> 0
    v.x = fminf(fmaxf(v.x, 0.0f), 1.0f);
    v.y = fminf(fmaxf(v.y, 0.0f), 1.0f);
    v.z = fminf(fmaxf(v.z, 0.0f), 1.0f);
    v.w = fmaxf(v.w, 0.0f);
    leaf_data[l] = v;
}

// ---------------------------------------------------------------------------------- K19b
// Per-leaf sums of WIDE rows: the gradient of an SH leaf is [d sigma, d k_cb = sum e_c Y_b(u)], 3 B + 1
// values, but an entry of K19a stays K17a's float4 (e_r, e_g, e_b, d sigma) plus its ray's number: the
// rank-one factor Y_b(u) belongs to the ray.  K17b-1/2/3 run unchanged.  The first level of the
// reduce reads a leaf's entries in sorted order in runs of kGradChunk, rebuilds each entry's basis
// from its ray's direction (sh_terms.h, the walk's own bits), and writes ONE row of kWidth = 16 / 28
// floats per run; further levels add runs of kGradChunk rows; the finish writes every row of the
// output.  The summation tree is K17b's, so the density column has K17b's order.  Wide rows exist per
// partial sum only: leaf l's run q lands at row seg_lo[l] / 16 + (non-empty leaves before l) + q,
// which never collides with the next leaf's (ceil(len / 16) <= floor((lo + len) / 16) - floor(lo / 16)
// + 1), so E / 16 + L + 1 rows hold every level.
//
// Thread mapping.  Level 0: one thread per run, with the kWidth accumulators in registers (28 + 9
// basis values + the entry: no LDS, no scratch).  The cost of level 0 is its dependent gathers --
// order[i], then the entry's 16 + 4 bytes, then 12 bytes of its ray's direction, all at random
// places -- and a thread per run does each ONCE per entry; one thread per (run, 16-byte quad) would
// repeat them seven times at degree 2 to make the row's store coalesced, and the row is 7 bytes per
// entry against 36 gathered.  Further levels and the finish touch 1/16 of that: a thread per run
// walks the row quad by quad (16 float4 loads each), a thread per (leaf, quad) finishes.
constexpr int sh_bases(int degree) { return (degree + 1) * (degree + 1); }
constexpr int sh_width(int degree) { return (3 * sh_bases(degree) + 1 + 3) / 4 * 4; }

// before[l] = 1 where leaf l has entries; scanned in place to the number of such leaves before l
__global__ void __launch_bounds__(256)
grad_sh_nonempty_kernel(const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                        int64_t num_leaves, int32_t* __restrict__ before) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= num_leaves) return;
    before[l] = seg_hi[l] > seg_lo[l] ? 1 : 0;
}

template <int kDegree>
__global__ void __launch_bounds__(256)
grad_sh_reduce_first_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ order,
                            const float4* __restrict__ values, const int32_t* __restrict__ rays,
                            const float* __restrict__ directions, int64_t n,
                            float4* __restrict__ rows, int64_t row_capacity, int32_t e,
                            int32_t num_leaves, const int32_t* __restrict__ seg_lo,
                            const int32_t* __restrict__ seg_hi,
                            const int32_t* __restrict__ before) {
    constexpr int kBasis = sh_bases(kDegree);
    constexpr int kWidth = sh_width(kDegree);
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= e) return;
    const int32_t l = keys[p];
    if (l < 0 || l >= num_leaves) return;
    const int lo = seg_lo[l];
    const int len = seg_hi[l] - lo;
    const int q = (int)p - lo;
    if (q < 0 || q >= (len + kGradChunk - 1) / kGradChunk) return;
    const int64_t at = (int64_t)(lo / kGradChunk) + before[l] + q;
    if (at >= row_capacity) return;           // never, for a workspace laid out for e entries
    const int first = lo + q * kGradChunk;
    const int end = min(first + kGradChunk, lo + len);
    float acc[kWidth];
#pragma unroll
    for (int k = 0; k < kWidth; ++k) acc[k] = 0.0f;
    for (int i = first; i < end; ++i) {
        const int32_t j = order != nullptr ? order[i] : i;
        if (j < 0 || j >= e) continue;         // never, for an order made by the sort
        const float4 v = values[j];
        const int64_t ray = rays[j];
        float basis[kBasis];
        if (ray >= 0 && ray < n) {
            const float dx = directions[ray * 3 + 0], dy = directions[ray * 3 + 1],
                        dz = directions[ray * 3 + 2];
            sh_ray_basis<kDegree>(dx, dy, dz, ray_norm(dx, dy, dz), basis);
        } else {
#pragma unroll
            for (int b = 0; b < kBasis; ++b) basis[b] = 0.0f;
        }
        const bool head = i == first;          // K17b starts from the first term, not from 0
        const float e3[3] = {v.x, v.y, v.z};
        acc[0] = head ? v.w : acc[0] + v.w;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int b = 0; b < kBasis; ++b) {
                const float term = e3[c] * basis[b];
                acc[1 + c * kBasis + b] = head ? term : acc[1 + c * kBasis + b] + term;
            }
    }
    float4* dst = rows + at * (kWidth / 4);
#pragma unroll
    for (int k = 0; k < kWidth / 4; ++k)
        dst[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
}

// level >= 1: runs of kGradChunk rows of a leaf into one, at the leaf's own rows of the other buffer
__global__ void __launch_bounds__(256)
grad_sh_reduce_kernel(const int32_t* __restrict__ keys, const float4* __restrict__ src,
                      float4* __restrict__ dst, int64_t row_capacity, int quads, int32_t e,
                      int32_t num_leaves, const int32_t* __restrict__ seg_lo,
                      const int32_t* __restrict__ seg_hi, const int32_t* __restrict__ before,
                      int level) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= e) return;
    const int32_t l = keys[p];
    if (l < 0 || l >= num_leaves) return;
    const int lo = seg_lo[l];
    int len = seg_hi[l] - lo;
    for (int j = 0; j < level; ++j) len = (len + kGradChunk - 1) / kGradChunk;
    const int q = (int)p - lo;
    if (q < 0 || q >= (len + kGradChunk - 1) / kGradChunk) return;
    const int64_t base = (int64_t)(lo / kGradChunk) + before[l];
    const int64_t first = base + (int64_t)q * kGradChunk;
    const int64_t last = min(first + kGradChunk, base + len);
    if (last > row_capacity) return;          // never, as above
    for (int k = 0; k < quads; ++k) {
        float4 acc = src[first * quads + k];
        for (int64_t i = first + 1; i < last; ++i) {
            const float4 v = src[i * quads + k];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        dst[(base + q) * quads + k] = acc;
    }
}

// every quad of every row of d_leaf_rows: the leaf's sum, +0 for a leaf without entries and for the
// columns past the kernel's own width (stride > 4 quads)
__global__ void __launch_bounds__(256)
grad_sh_finish_kernel(const float4* __restrict__ sums, int quads, const int32_t* __restrict__ seg_lo,
                      const int32_t* __restrict__ seg_hi, const int32_t* __restrict__ before,
                      int64_t num_leaves, int stride_quads, float4* __restrict__ d_leaf_rows) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= num_leaves * stride_quads) return;
    const int64_t l = idx / stride_quads;
    const int k = (int)(idx - l * stride_quads);
    const int lo = seg_lo[l];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (seg_hi[l] > lo && k < quads) v = sums[((int64_t)(lo / kGradChunk) + before[l]) * quads + k];
    v.x += 0.0f; v.y += 0.0f; v.z += 0.0f; v.w += 0.0f;      // as K17b-5
    d_leaf_rows[idx] = v;
}

// ---------------------------------------------------------------------------------- K19c
__global__ void __launch_bounds__(256)
octree_project_sh_kernel(float4* __restrict__ rows, int64_t num_leaves, int stride_quads,
                         int channels) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= num_leaves * stride_quads) return;
    const int col = 4 * (int)(idx % stride_quads);
    if (col >= channels) return;              // padding: untouched
    const float4 v = rows[idx];
    float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (col + j == 0) x[j] = x[j] > 0.0f ? x[j] : 0.0f;              // density; NaN, -0 -> +0
        else if (col + j < channels) x[j] = x[j] != x[j] ? 0.0f : x[j];  // a logit: only NaN moves
    }
    rows[idx] = make_float4(x[0], x[1], x[2], x[3]);
}

struct GradWorkspace {
    int32_t* ray_slots;     // n + 1
    float* ray_color;       // 3n
    float* ray_trans;       // n
    int32_t* block_sums;    // of the longest of the scans
    float4* values;         // capacity, ray-major; K17b: then the odd reduce levels' target
    float4* sums;           // capacity (K17b only: K19b's partial sums are rows)
    int32_t* keys[2];       // capacity each
    int32_t* order[2];      // capacity each
    int32_t* table;         // 256 * tiles
    int32_t* seg_lo;        // num_leaves
    int32_t* seg_hi;        // num_leaves
    // K19b only
    int32_t* rays;          // capacity: the ray of every entry
    int32_t* before;        // num_leaves
    float4* rows[2];        // row_capacity rows of sh_width(degree) floats each
    int64_t row_capacity;
    // K29b only
    float* ray_dist;        // 3n: W_tot, M_tot, D per ray
};

static inline int64_t align256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

// The buffers of K17b (degree 0) or K19b (degree 1, 2) behind one another from `base` (null: sizes
// only) -> the bytes they take; a buffer the kind does not use stays null.  K19b: E / 16 + min(E, L)
// rows hold every level's partial sums; the second term is taken at L so that the size stays affine
// in max_entries.
// K29b: the same buffers at the same offsets and the per-ray triples BEHIND them, so that the sizes
// and the layout of the entries without the term are what they were.
static int64_t grad_layout(int64_t n, int64_t num_leaves, int64_t capacity, int degree,
                           GradWorkspace* ws, char* base, bool dist = false) {
    const bool sh = degree > 0;
    const int64_t tiles = (capacity + kSortTile - 1) / kSortTile;
    int64_t longest = 256 * tiles > n ? 256 * tiles : n;
    if (sh && num_leaves > longest) longest = num_leaves;     // the scan of `before`
    const int64_t blocks = (longest + kGradScanBlock - 1) / kGradScanBlock + 1;
    const int64_t row_capacity = sh ? capacity / kGradChunk + num_leaves + 1 : 0;
    const int64_t rows_bytes = sh ? 4 * (int64_t)sh_width(degree) * row_capacity : 0;
    GradWorkspace scratch;
    GradWorkspace& w = ws != nullptr ? *ws : scratch;
    w = GradWorkspace{};
    w.row_capacity = row_capacity;
    const struct { void** slot; int64_t bytes; bool used; } buffers[] = {
        {(void**)&w.ray_slots, 4 * (n + 1), true},      {(void**)&w.ray_color, 12 * n, true},
        {(void**)&w.ray_trans, 4 * n, true},            {(void**)&w.block_sums, 4 * blocks, true},
        {(void**)&w.values, 16 * capacity, true},       {(void**)&w.sums, 16 * capacity, !sh},
        {(void**)&w.keys[0], 4 * capacity, true},       {(void**)&w.keys[1], 4 * capacity, true},
        {(void**)&w.order[0], 4 * capacity, true},      {(void**)&w.order[1], 4 * capacity, true},
        {(void**)&w.table, 4 * 256 * tiles, true},      {(void**)&w.seg_lo, 4 * num_leaves, true},
        {(void**)&w.seg_hi, 4 * num_leaves, true},      {(void**)&w.rays, 4 * capacity, sh},
        {(void**)&w.before, 4 * num_leaves, sh},        {(void**)&w.rows[0], rows_bytes, sh},
        {(void**)&w.rows[1], rows_bytes, sh},           {(void**)&w.ray_dist, 12 * n, dist}};
    int64_t off = 0;
    for (const auto& b : buffers) {
        if (!b.used) continue;
        if (base != nullptr) *b.slot = base + off;
        off += align256(b.bytes);
    }
    return off;
}

// K17b-2 and K17b-3 on the e entries whose leaf numbers K17a / K19a left in ws.keys[0]: -> the sorted
// keys and the entries' order (null when a single leaf needs no pass: the entries are in place)
static void sort_and_bounds(const GradWorkspace& ws, int32_t e, int64_t num_leaves, hipStream_t st,
                            const int32_t** keys_out_p, const int32_t** order_out_p) {
    int bits = 0;
    while (bits < 31 && ((int64_t)1 << bits) < num_leaves) ++bits;
    const int passes = (bits + 7) / 8;
    const int32_t tiles = (e + kSortTile - 1) / kSortTile;
    const int32_t* keys = ws.keys[0];
    const int32_t* order = nullptr;
    for (int pass = 0; pass < passes; ++pass) {
        int32_t* keys_out = ws.keys[(pass + 1) & 1];
        int32_t* order_out = ws.order[(pass + 1) & 1];
        hipLaunchKernelGGL(grad_sort_hist_kernel, dim3(tiles), dim3(kSortThreads), 0, st, keys, e,
                           8 * pass, tiles, ws.table);
        exclusive_scan(ws.table, (int64_t)256 * tiles, ws.block_sums, nullptr, st);
        hipLaunchKernelGGL(grad_sort_scatter_kernel, dim3(tiles), dim3(kSortThreads), 0, st, keys,
                           order, e, 8 * pass, tiles, ws.table, keys_out, order_out);
        keys = keys_out;
        order = order_out;
    }
    const unsigned over_entries = (unsigned)(((int64_t)e + 255) / 256);
    (void)hipMemsetAsync(ws.seg_lo, 0, 4 * num_leaves, st);
    (void)hipMemsetAsync(ws.seg_hi, 0, 4 * num_leaves, st);
    hipLaunchKernelGGL(grad_bounds_kernel, dim3(over_entries), dim3(256), 0, st, keys, e,
                       (int32_t)num_leaves, ws.seg_lo, ws.seg_hi);
    *keys_out_p = keys;
    *order_out_p = order;
}

static inline bool grad_shape(int64_t n, int64_t num_leaves, int64_t max_entries) {
    return n >= 1 && n < ((int64_t)1 << 31) && num_leaves >= 1 && num_leaves < ((int64_t)1 << 31) &&
           max_entries >= 0 && max_entries <= kGradMaxEntries;
}

static int64_t grad_workspace_bytes(const char* who, int64_t n, int64_t num_leaves,
                                    int64_t max_entries, int degree, bool dist = false) {
    if (!grad_shape(n, num_leaves, max_entries)) {
        fail_who(who, "shape (1 <= n < 2^31, 1 <= num_leaves < 2^31, 0 <= max_entries < 2^31)");
        return -1;
    }
    return grad_layout(n, num_leaves, max_entries, degree, nullptr, nullptr, dist);
}

// what the front half of a backward leaves for its reduce: the e > 0 entries sorted by leaf
struct GradEntries {
    GradWorkspace ws;
    int32_t e;
    const int32_t* keys;
    const int32_t* order;
    unsigned over_entries;  // workgroups of 256 over the entries
    int levels;             // of the reduce
};

// The front half of both backwards, for a walk whose arguments the entry point has checked: the
// workspace laid out for grad.leaves.degree, the first walk (counts, C and T_{n+1} per ray), the
// scan, the read-back of the total E (*entries, where the caller wants it) and its refusal, the
// second walk (the entries), sort and bounds.  E == 0: every row of d_leaves (row_bytes each) is
// zeroed here and got->e is 0: nothing is left to reduce.
static int grad_entries(const char* who, GradWalk& grad, void* workspace, int64_t workspace_bytes,
                        int64_t max_entries, void* d_leaves, int64_t row_bytes, int64_t* entries,
                        GradEntries* got) {
    const int64_t n = grad.walk.n, num_leaves = grad.walk.num_leaves;
    const int degree = grad.leaves.degree;
    const hipStream_t st = grad.walk.stream;
    got->e = 0;
    // a ray crosses at most 3 * 2^(depth-1) + 1 regions: the entry offsets stay below 2^31
    if (!grad_shape(n, num_leaves, max_entries) ||
        n * (3 * ((int64_t)1 << (grad.walk.depth - 1)) + 1) > kGradMaxEntries)
        return fail_who(who, "shape (n * (3 * 2^(depth-1) + 1) < 2^31: split the rays)");
    if (workspace_bytes < grad_layout(n, num_leaves, max_entries, degree, nullptr, nullptr, grad.dist))
        return fail_who(who, "workspace too small for max_entries");
    GradWorkspace& ws = got->ws;
    grad_layout(n, num_leaves, max_entries, degree, &ws, (char*)workspace, grad.dist);
    grad.ray_dist = ws.ray_dist;
    grad.ray_slots = ws.ray_slots; grad.ray_color = ws.ray_color; grad.ray_trans = ws.ray_trans;
    grad.entry_values = ws.values; grad.entry_leaves = ws.keys[0]; grad.entry_rays = ws.rays;

    if (int err = octree_grad_walk(who, grad, 0)) return err;
    exclusive_scan(ws.ray_slots, n, ws.block_sums, ws.ray_slots + n, st);
    int32_t total = 0;
    hipError_t copied = hipMemcpyAsync(&total, ws.ray_slots + n, 4, hipMemcpyDeviceToHost, st);
    if (copied == hipSuccess) copied = hipStreamSynchronize(st);
    if (copied != hipSuccess) {
        set_error(who, copied);
        return (int)copied;
    }
    if (entries != nullptr) *entries = total;
    if (total < 0 || total > max_entries) {
        char text[160];
        snprintf(text, sizeof text, "%s: the rays take %lld leaves, the workspace holds %lld entries",
                 who, (long long)total, (long long)max_entries);
        return fail_arg(text);
    }
    if (total == 0) {
        (void)hipMemsetAsync(d_leaves, 0, row_bytes * num_leaves, st);
        return check_launch(who);
    }
    if (int err = octree_grad_walk(who, grad, 1)) return err;
    got->e = total;
    sort_and_bounds(ws, got->e, num_leaves, st, &got->keys, &got->order);
    got->over_entries = (unsigned)(((int64_t)got->e + 255) / 256);
    // a ray takes a leaf once: no list is longer than min(n, e)
    const int64_t longest = n < got->e ? n : got->e;
    got->levels = 1;
    for (int64_t reach = kGradChunk; reach < longest; reach *= kGradChunk) ++got->levels;
    return 0;
}

}  // namespace ffn

using namespace ffn;

extern "C" int64_t ffn_octree_grad_workspace_bytes(int64_t n, int64_t num_leaves,
                                                   int64_t max_entries) {
    return grad_workspace_bytes("ffn_octree_grad_workspace_bytes", n, num_leaves, max_entries, 0);
}

// K29b: what the two entries with the distortion term refuse before anything else, and the walk's
// three fields
static int grad_dist_args(const char* who, GradWalk& grad, float dist_scale, float* ray_distortion) {
    if (!(dist_scale >= 0.0f && dist_scale < __builtin_inff()))          // NaN fails too
        return fail_who(who, "dist_scale must be finite and >= 0");
    grad.dist = true;
    grad.dist_scale = dist_scale;
    grad.ray_distortion = ray_distortion;
    return 0;
}

// K17a + K17b, and with dist K29b: ffn_octree_render_volume_backward[_dist]
static int volume_backward(const char* who, bool dist, float dist_scale, float* ray_distortion,
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_data, int64_t* entries,
    void* stream) {
    GradWalk grad{{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                   num_leaves, t_min, (hipStream_t)stream},
                  {leaf_data, channels, 0, bg_r, bg_g, bg_b, min_transmittance}, d_color, d_alpha};
    if (entries != nullptr) *entries = -1;
    if (dist)
        if (int err = grad_dist_args(who, grad, dist_scale, ray_distortion)) return err;
    if (channels < 4) return fail_who(who, "channels >= 4");
    if (int err = check_volume_args(who, grad.walk, grad.leaves,
                                    !d_color || !d_alpha || !d_leaf_data || !workspace))
        return err;
    if (channels == 4 && misaligned16(leaf_data))
        return fail_who(who, "leaf_data with 4 channels must be 16-byte aligned");
    if (misaligned16(d_leaf_data) || misaligned16(workspace))
        return fail_who(who, "d_leaf_data and workspace must be 16-byte aligned");
    GradEntries got;
    const int err = grad_entries(who, grad, workspace, workspace_bytes, max_entries, d_leaf_data, 16,
                                 entries, &got);
    if (err != 0 || got.e == 0) return err;
    const GradWorkspace& ws = got.ws;
    const float4* src = ws.values;
    for (int level = 0; level < got.levels; ++level) {
        float4* dst = (level & 1) ? ws.values : ws.sums;
        hipLaunchKernelGGL(grad_reduce_kernel, dim3(got.over_entries), dim3(256), 0, grad.walk.stream,
                           got.keys, level == 0 ? got.order : (const int32_t*)nullptr, src, dst,
                           got.e, (int32_t)num_leaves, ws.seg_lo, ws.seg_hi, level);
        src = dst;
    }
    hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)((num_leaves + 255) / 256)), dim3(256), 0,
                       grad.walk.stream, src, ws.seg_lo, ws.seg_hi, num_leaves,
                       (float4*)d_leaf_data);
    return check_launch(who);
}

extern "C" int ffn_octree_render_volume_backward(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_data, int64_t* entries,
    void* stream) {
    return volume_backward("ffn_octree_render_volume_backward", false, 0.0f, nullptr, starts,
                           directions, n, scale, depth, node_index, num_nodes, leaf_index, num_leaves,
                           t_min, leaf_data, channels, bg_r, bg_g, bg_b, min_transmittance, d_color,
                           d_alpha, workspace, workspace_bytes, max_entries, d_leaf_data, entries,
                           stream);
}

extern "C" int64_t ffn_octree_grad_dist_workspace_bytes(int64_t n, int64_t num_leaves,
                                                        int64_t max_entries, int degree) {
    if (degree < 0 || degree > 2) {
        fail_arg("ffn_octree_grad_dist_workspace_bytes: degree is 0 (plain rows), 1 or 2");
        return -1;
    }
    return grad_workspace_bytes("ffn_octree_grad_dist_workspace_bytes", n, num_leaves, max_entries,
                                degree, true);
}

extern "C" int ffn_octree_render_volume_backward_dist(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_data, int64_t* entries,
    float dist_scale, float* ray_distortion, void* stream) {
    return volume_backward("ffn_octree_render_volume_backward_dist", true, dist_scale,
                           ray_distortion, starts, directions, n, scale, depth, node_index, num_nodes,
                           leaf_index, num_leaves, t_min, leaf_data, channels, bg_r, bg_g, bg_b,
                           min_transmittance, d_color, d_alpha, workspace, workspace_bytes,
                           max_entries, d_leaf_data, entries, stream);
}

extern "C" int ffn_octree_project(float* leaf_data, int64_t num_leaves, void* stream) {
    if (!leaf_data) return fail_arg("ffn_octree_project: null argument");
    if (num_leaves < 1) return fail_arg("ffn_octree_project: num_leaves >= 1");
    if (((uintptr_t)leaf_data & 15) != 0)
        return fail_arg("ffn_octree_project: leaf_data must be 16-byte aligned");
    hipLaunchKernelGGL(octree_project_kernel, dim3((unsigned)((num_leaves + 255) / 256)), dim3(256),
                       0, (hipStream_t)stream, (float4*)leaf_data, num_leaves);
    return check_launch("ffn_octree_project");
}

extern "C" int64_t ffn_octree_grad_sh_workspace_bytes(int64_t n, int64_t num_leaves,
                                                      int64_t max_entries, int degree) {
    if (degree != 1 && degree != 2) {
        fail_arg("ffn_octree_grad_sh_workspace_bytes: degree is 1 or 2");
        return -1;
    }
    return grad_workspace_bytes("ffn_octree_grad_sh_workspace_bytes", n, num_leaves, max_entries,
                                degree);
}

// K19a + K19b, and with dist K29b: ffn_octree_render_volume_sh_backward[_dist]
static int volume_sh_backward(const char* who, bool dist, float dist_scale, float* ray_distortion,
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_rows, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_rows, int64_t* entries, int degree,
    int row_stride, void* stream) {
    GradWalk grad{{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                   num_leaves, t_min, (hipStream_t)stream},
                  {leaf_rows, row_stride, degree, bg_r, bg_g, bg_b, min_transmittance}, d_color,
                  d_alpha};
    if (entries != nullptr) *entries = -1;
    if (dist)
        if (int err = grad_dist_args(who, grad, dist_scale, ray_distortion)) return err;
    if (degree != 1 && degree != 2) return fail_who(who, "degree is 1 or 2");
    if (row_stride < 3 * sh_bases(degree) + 1 || row_stride % 4 != 0 || row_stride > 64)
        return fail_who(who, "row_stride is a multiple of 4, 3 * (degree + 1)^2 + 1 <= row_stride "
                             "<= 64");
    if (int err = check_volume_args(who, grad.walk, grad.leaves,
                                    !d_color || !d_alpha || !d_leaf_rows || !workspace))
        return err;
    if (misaligned16(leaf_rows) || misaligned16(d_leaf_rows) || misaligned16(workspace))
        return fail_who(who, "leaf_rows, d_leaf_rows and workspace must be 16-byte aligned");
    GradEntries got;
    const int err = grad_entries(who, grad, workspace, workspace_bytes, max_entries, d_leaf_rows,
                                 4 * (int64_t)row_stride, entries, &got);
    if (err != 0 || got.e == 0) return err;
    const GradWorkspace& ws = got.ws;
    const hipStream_t st = grad.walk.stream;
    const unsigned over_leaves = (unsigned)((num_leaves + 255) / 256);
    hipLaunchKernelGGL(grad_sh_nonempty_kernel, dim3(over_leaves), dim3(256), 0, st, ws.seg_lo,
                       ws.seg_hi, num_leaves, ws.before);
    exclusive_scan(ws.before, num_leaves, ws.block_sums, nullptr, st);
    const int quads = sh_width(degree) / 4;
    if (degree == 1)
        hipLaunchKernelGGL(grad_sh_reduce_first_kernel<1>, dim3(got.over_entries), dim3(256), 0, st,
                           got.keys, got.order, ws.values, ws.rays, directions, n, ws.rows[0],
                           ws.row_capacity, got.e, (int32_t)num_leaves, ws.seg_lo, ws.seg_hi,
                           ws.before);
    else
        hipLaunchKernelGGL(grad_sh_reduce_first_kernel<2>, dim3(got.over_entries), dim3(256), 0, st,
                           got.keys, got.order, ws.values, ws.rays, directions, n, ws.rows[0],
                           ws.row_capacity, got.e, (int32_t)num_leaves, ws.seg_lo, ws.seg_hi,
                           ws.before);
    const float4* src = ws.rows[0];
    for (int level = 1; level < got.levels; ++level) {
        float4* dst = ws.rows[level & 1];
        hipLaunchKernelGGL(grad_sh_reduce_kernel, dim3(got.over_entries), dim3(256), 0, st, got.keys,
                           src, dst, ws.row_capacity, quads, got.e, (int32_t)num_leaves, ws.seg_lo,
                           ws.seg_hi, ws.before, level);
        src = dst;
    }
    const int stride_quads = row_stride / 4;
    hipLaunchKernelGGL(grad_sh_finish_kernel,
                       dim3((unsigned)((num_leaves * stride_quads + 255) / 256)), dim3(256), 0, st,
                       src, quads, ws.seg_lo, ws.seg_hi, ws.before, num_leaves, stride_quads,
                       (float4*)d_leaf_rows);
    return check_launch(who);
}

extern "C" int ffn_octree_render_volume_sh_backward(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_rows, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_rows, int64_t* entries, int degree,
    int row_stride, void* stream) {
    return volume_sh_backward("ffn_octree_render_volume_sh_backward", false, 0.0f, nullptr, starts,
                              directions, n, scale, depth, node_index, num_nodes, leaf_index,
                              num_leaves, t_min, leaf_rows, bg_r, bg_g, bg_b, min_transmittance,
                              d_color, d_alpha, workspace, workspace_bytes, max_entries, d_leaf_rows,
                              entries, degree, row_stride, stream);
}

extern "C" int ffn_octree_render_volume_sh_backward_dist(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_rows, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_rows, int64_t* entries, int degree,
    int row_stride, float dist_scale, float* ray_distortion, void* stream) {
    return volume_sh_backward("ffn_octree_render_volume_sh_backward_dist", true, dist_scale,
                              ray_distortion, starts, directions, n, scale, depth, node_index,
                              num_nodes, leaf_index, num_leaves, t_min, leaf_rows, bg_r, bg_g, bg_b,
                              min_transmittance, d_color, d_alpha, workspace, workspace_bytes,
                              max_entries, d_leaf_rows, entries, degree, row_stride, stream);
}

extern "C" int ffn_octree_project_sh(float* leaf_rows, int64_t num_leaves, int row_stride,
                                     int degree, void* stream) {
    if (degree != 1 && degree != 2) return fail_arg("ffn_octree_project_sh: degree is 1 or 2");
    if (row_stride < 3 * sh_bases(degree) + 1 || row_stride % 4 != 0 || row_stride > 64)
        return fail_arg("ffn_octree_project_sh: row_stride is a multiple of 4, "
                        "3 * (degree + 1)^2 + 1 <= row_stride <= 64");
    if (!leaf_rows) return fail_arg("ffn_octree_project_sh: null argument");
    if (num_leaves < 1 || num_leaves >= ((int64_t)1 << 31))
        return fail_arg("ffn_octree_project_sh: 1 <= num_leaves < 2^31");
    if (((uintptr_t)leaf_rows & 15) != 0)
        return fail_arg("ffn_octree_project_sh: leaf_rows must be 16-byte aligned");
    const int stride_quads = row_stride / 4;
    hipLaunchKernelGGL(octree_project_sh_kernel,
                       dim3((unsigned)((num_leaves * stride_quads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (float4*)leaf_rows, num_leaves, stride_quads,
                       3 * sh_bases(degree) + 1);
    return check_launch("ffn_octree_project_sh");
}
