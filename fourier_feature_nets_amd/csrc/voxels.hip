// K10b: backward of the dense voxel lookup K10 (csrc/occupancy.hip), i.e. of the reference's
// Voxels.forward (voxels_model.py:35-45: grid_sample of a (1,4,S,S,S) volume, trilinear,
// padding_mode="border", align_corners=False, plus a bias).  Training a voxel field
// (train_voxels.py of the reference) needs d(loss)/d(volume) and d(loss)/d(bias) from the
// per-sample d(loss)/d(logits).
//
// It is a scatter (every sample adds to the eight corners of its cell) done without float
// atomics, so that the same inputs give the same bits on every call: the store-and-sum form.
//
//   K10b-1 voxels_count      per sample: its cell (the corner `lo`), an arrival slot in the cell
//                            (integer atomics, one per run of equal cells in a wave), and the
//                            d_bias partial of the workgroup (fixed order)
//   K10b-2 voxels_scan_*     exclusive scan of the S^3 cell counts (per-4096-cell sums, one
//                            workgroup over those sums, then the per-block scans); d_bias
//   K10b-3 voxels_place      sample ids into their cell's list, in arrival order
//   K10b-4 voxels_rank       each list in sample-id order: an entry's place is the number of
//                            smaller ids in its list; (frac, cell, d_logits) stored there
//   K10b-5 voxels_chunks     per chunk of kChunk consecutive entries of a list, its 8 x 4 corner
//                            sums, stored at slot offsets[cell] + chunk (inside the cell's own
//                            entry range: no allocation, no atomics)
//   K10b-6 voxels_cells      lists longer than kChunk: their chunk sums added in chunk order into
//                            slot offsets[cell] (skewed inputs: no thread walks a long list)
//   K10b-7 voxels_gather     per voxel, the corner sums of the 8 cells it is a corner of, in a
//                            fixed order, in f32: every entry written
//
// The weights are K10's own: the same coordinate formula, clamp, lo / hi = min(lo+1, S-1) and
// weight products.  A corner clamped onto lo (lo = S-1, where the fraction is 0) receives
// nothing, as in ATen's within_bounds skip.
#include "common.h"

namespace ffn {

constexpr int kChunk = 16;            // entries summed by one thread (longer lists: in chunks)
constexpr int kScanBlock = 4096;      // cells per workgroup of the count scan (256 x 16)
constexpr int kCountBlocks = 1024;    // fixed grid of voxels_count: fixes the d_bias order

struct VoxMap {
    float inv_scale;
    int side;
};

// K10's coordinate arithmetic, written the same way (same contraction into FMAs)
__device__ __forceinline__ void voxel_coord(const VoxMap m, const float* __restrict__ p, int lo[3],
                                            float frac[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float c = ((p[d] * m.inv_scale + 1.0f) * (float)m.side - 1.0f) * 0.5f;
        c = fminf(fmaxf(c, 0.0f), (float)(m.side - 1));          // border padding
        const float f = floorf(c);
        lo[d] = (int)f;
        frac[d] = c - f;
    }
}

// K10's weight of corner k = dz*4 + dy*2 + dx of a cell (same product order)
__device__ __forceinline__ float corner_weight(const float4 f, int k) {
    const float wx = (k & 1) ? f.x : 1.0f - f.x;
    const float wy = (k & 2) ? f.y : 1.0f - f.y;
    const float wz = (k & 4) ? f.z : 1.0f - f.z;
    return wx * wy * wz;
}

struct VoxWorkspace {
    int32_t* counts;        // cells: per-cell counts
    int32_t* offsets;       // cells + 1
    int32_t* block_sums;    // ceil(cells / kScanBlock)
    float4* bias_partials;  // kCountBlocks
    int32_t* cell;          // n
    int32_t* slot;          // n
    int32_t* unsorted;      // n
    float4* entries;        // 2n: (frac.xyz, cell bits), d_logits
    float4* chunk_sums;     // 8 per entry slot (used at chunk slots only)
};

// ---------------------------------------------------------------------------------- K10b-1
__global__ void __launch_bounds__(256)
voxels_count_kernel(const float* __restrict__ positions, const float4* __restrict__ d_logits,
                    int64_t n, VoxMap m, int32_t* __restrict__ counts, int32_t* __restrict__ cell,
                    int32_t* __restrict__ slot, float4* __restrict__ bias_partials) {
    __shared__ float4 red[256];
    const int lane = lane_id();
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool valid = i < n;
        int c = -1;
        if (valid) {
            int lo[3];
            float frac[3];
            voxel_coord(m, positions + i * 3, lo, frac);
            c = (lo[2] * m.side + lo[1]) * m.side + lo[0];
            const float4 g = d_logits[i];
            bsum.x += g.x; bsum.y += g.y; bsum.z += g.z; bsum.w += g.w;
        }
        // runs of equal cells among consecutive lanes (samples along a ray) take one atomic
        const int prev = __shfl_up(c, 1);
        const bool head = valid && (lane == 0 || prev != c);
        const uint64_t heads = __ballot(head);
        const int nvalid = __popcll(__ballot(valid));
        const uint64_t upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
        const uint64_t mine = heads & upto;
        const int my_head = mine ? 63 - __clzll(mine) : 0;
        int base = 0;
        if (head) {
            const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = after ? __ffsll((unsigned long long)after) : nvalid - lane;
            base = atomicAdd(counts + c, len);
        }
        base = __shfl(base, my_head);
        if (valid) {
            cell[i] = c;
            slot[i] = base + lane - my_head;
        }
    }
    red[threadIdx.x] = bsum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            float4 a = red[threadIdx.x];
            const float4 b = red[threadIdx.x + s];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            red[threadIdx.x] = a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) bias_partials[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------------------------- K10b-2
__device__ __forceinline__ int block_sum_256(int v, int* lds) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ void __launch_bounds__(256)
voxels_scan_sums_kernel(const int32_t* __restrict__ counts, int64_t cells,
                        int32_t* __restrict__ block_sums) {
    __shared__ int lds[4];
    const int64_t first = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * 16;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (first + k < cells) s += counts[first + k];
    s = block_sum_256(s, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s;
}

// one workgroup: exclusive scan of the block sums in place; d_bias from the count partials
__global__ void __launch_bounds__(1024)
voxels_scan_top_kernel(int32_t* __restrict__ block_sums, int blocks,
                       const float4* __restrict__ bias_partials, int bias_blocks,
                       float* __restrict__ d_bias) {
    __shared__ int part[1024];
    __shared__ float4 red[1024];
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
    red[threadIdx.x] = threadIdx.x < bias_blocks ? bias_partials[threadIdx.x]
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            float4 a = red[threadIdx.x];
            const float4 b = red[threadIdx.x + s];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            red[threadIdx.x] = a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        d_bias[0] = red[0].x; d_bias[1] = red[0].y; d_bias[2] = red[0].z; d_bias[3] = red[0].w;
    }
}

__global__ void __launch_bounds__(256)
voxels_scan_apply_kernel(const int32_t* __restrict__ counts, int64_t cells,
                         const int32_t* __restrict__ block_sums, int32_t n,
                         int32_t* __restrict__ offsets) {
    __shared__ int wave_tot[4];
    const int64_t first = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * 16;
    int local[16];
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        local[k] = first + k < cells ? counts[first + k] : 0;
        s += local[k];
    }
    // inclusive scan of the thread totals inside the wave, then across the four waves
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
        if (first + k < cells) offsets[first + k] = run;
        run += local[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[cells] = n;
}

// ---------------------------------------------------------------------------------- K10b-3
__global__ void __launch_bounds__(256)
voxels_place_kernel(const int32_t* __restrict__ cell, const int32_t* __restrict__ slot, int32_t n,
                    const int32_t* __restrict__ offsets, int32_t* __restrict__ unsorted) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        unsorted[offsets[cell[i]] + slot[i]] = i;
}

// ---------------------------------------------------------------------------------- K10b-4
__global__ void __launch_bounds__(256)
voxels_rank_kernel(const float* __restrict__ positions, const float4* __restrict__ d_logits,
                   int32_t n, VoxMap m, const int32_t* __restrict__ cell,
                   const int32_t* __restrict__ offsets, const int32_t* __restrict__ unsorted,
                   float4* __restrict__ entries) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int c = cell[i];
        const int lo = offsets[c], len = offsets[c + 1] - lo;
        int r = 0;
        for (int k = 0; k < len; ++k) r += unsorted[lo + k] < i;
        int cl[3];
        float frac[3];
        voxel_coord(m, positions + (int64_t)i * 3, cl, frac);
        entries[2 * (int64_t)(lo + r)] = make_float4(frac[0], frac[1], frac[2], __int_as_float(c));
        entries[2 * (int64_t)(lo + r) + 1] = d_logits[i];
    }
}

// ---------------------------------------------------------------------------------- K10b-5
__global__ void __launch_bounds__(256)
voxels_chunks_kernel(const float4* __restrict__ entries, int32_t n,
                     const int32_t* __restrict__ offsets, float4* __restrict__ chunk_sums) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int c = __float_as_int(entries[2 * (int64_t)p].w);
        const int lo = offsets[c], len = offsets[c + 1] - lo;
        if ((p - lo) % kChunk != 0) continue;
        const int end = min(p + kChunk, lo + len);
        float4 acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int q = p; q < end; ++q) {
            const float4 f = entries[2 * (int64_t)q], g = entries[2 * (int64_t)q + 1];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float w = corner_weight(f, k);
                acc[k].x += g.x * w; acc[k].y += g.y * w; acc[k].z += g.z * w; acc[k].w += g.w * w;
            }
        }
        float4* dst = chunk_sums + 8 * ((int64_t)lo + (p - lo) / kChunk);
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = acc[k];
    }
}

// ---------------------------------------------------------------------------------- K10b-6
__global__ void __launch_bounds__(256)
voxels_cells_kernel(const float4* __restrict__ entries, int32_t n,
                    const int32_t* __restrict__ offsets, float4* __restrict__ chunk_sums) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int c = __float_as_int(entries[2 * (int64_t)p].w);
        const int lo = offsets[c], len = offsets[c + 1] - lo;
        if (p != lo || len <= kChunk) continue;
        float4* cell = chunk_sums + 8 * (int64_t)lo;
        const int chunks = (len + kChunk - 1) / kChunk;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float4 acc = cell[k];
            for (int j = 1; j < chunks; ++j) {
                const float4 s = cell[8 * (int64_t)j + k];
                acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
            }
            cell[k] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------- K10b-7
__global__ void __launch_bounds__(256)
voxels_gather_kernel(const int32_t* __restrict__ offsets, const float4* __restrict__ cell_sums,
                     int side, float* __restrict__ d_volume) {
    const uint32_t s = (uint32_t)side, plane = s * s, cells = plane * s;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < cells; v += gridDim.x * blockDim.x) {
        const uint32_t row = v / s, x = v - row * s, z = row / s, y = row - z * s;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        // voxel (z,y,x) is corner k = dz*4 + dy*2 + dx of cell (z-dz, y-dy, x-dx)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
            if (x < dx || y < dy || z < dz) continue;
            const uint32_t c = v - dz * plane - dy * s - dx;
            const int lo = offsets[c];
            if (offsets[c + 1] == lo) continue;
            const float4 t = cell_sums[8 * (int64_t)lo + k];
            acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        }
        d_volume[v] = acc.x;
        d_volume[cells + v] = acc.y;
        d_volume[2 * (int64_t)cells + v] = acc.z;
        d_volume[3 * (int64_t)cells + v] = acc.w;
    }
}

// workspace layout: every region starts on a 256-byte boundary
static inline int64_t align256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

static int64_t workspace_layout(int64_t n, int side, VoxWorkspace* ws, char* base) {
    const int64_t cells = (int64_t)side * side * side;
    const int64_t blocks = (cells + kScanBlock - 1) / kScanBlock;
    const int64_t sizes[9] = {4 * cells, 4 * (cells + 1), 4 * blocks, 16 * kCountBlocks,
                              4 * n, 4 * n, 4 * n, 32 * n, 128 * n};
    void** slots[9] = {(void**)&ws->counts, (void**)&ws->offsets, (void**)&ws->block_sums,
                       (void**)&ws->bias_partials, (void**)&ws->cell, (void**)&ws->slot,
                       (void**)&ws->unsorted, (void**)&ws->entries, (void**)&ws->chunk_sums};
    int64_t off = 0;
    for (int r = 0; r < 9; ++r) {
        if (base != nullptr) *slots[r] = base + off;
        off += align256(sizes[r]);
    }
    return off;
}

static inline bool valid_shape(int64_t n, int side) {
    return n >= 0 && n <= ((int64_t)1 << 30) && side >= 1 && side <= 1024;
}

static inline int grid_for(int64_t work) {
    int64_t g = (work + 255) / 256;
    if (g > 8192) g = 8192;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace ffn

using namespace ffn;

extern "C" int64_t ffn_voxels_backward_workspace(int64_t n, int side) {
    if (!valid_shape(n, side)) {
        fail_arg("ffn_voxels_backward_workspace: shape");
        return -1;
    }
    return workspace_layout(n, side, nullptr, nullptr);
}

extern "C" int ffn_voxels_backward(const float* positions, const float* d_logits, int64_t n,
                                   int side, float scale, void* workspace, int64_t workspace_bytes,
                                   float* d_volume, float* d_bias, void* stream) {
    if (!valid_shape(n, side)) return fail_arg("ffn_voxels_backward: shape");
    if (!(scale > 0.0f) || !(scale < __builtin_huge_valf()))
        return fail_arg("ffn_voxels_backward: scale");
    if (d_volume == nullptr || d_bias == nullptr || (n > 0 && (positions == nullptr || d_logits == nullptr)))
        return fail_arg("ffn_voxels_backward: null buffer");
    if (((uintptr_t)d_logits & 15) != 0) return fail_arg("ffn_voxels_backward: d_logits not 16-byte aligned");
    const int64_t need = workspace_layout(n, side, nullptr, nullptr);
    if (n > 0 && (workspace == nullptr || workspace_bytes < need))
        return fail_arg("ffn_voxels_backward: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail_arg("ffn_voxels_backward: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)side * side * side;
    if (n == 0) {
        (void)hipMemsetAsync(d_volume, 0, 4 * 4 * cells, st);
        (void)hipMemsetAsync(d_bias, 0, 4 * 4, st);
        return check_launch("ffn_voxels_backward");
    }
    VoxWorkspace ws;
    workspace_layout(n, side, &ws, (char*)workspace);
    const VoxMap m{1.0f / scale, side};
    const int n32 = (int)n;
    const int scan_blocks = (int)((cells + kScanBlock - 1) / kScanBlock);
    const int count_blocks = (int)((n + 255) / 256 < kCountBlocks ? (n + 255) / 256 : kCountBlocks);
    (void)hipMemsetAsync(ws.counts, 0, 4 * cells, st);
    hipLaunchKernelGGL(voxels_count_kernel, dim3(count_blocks), dim3(256), 0, st, positions,
                       (const float4*)d_logits, n, m, ws.counts, ws.cell, ws.slot, ws.bias_partials);
    hipLaunchKernelGGL(voxels_scan_sums_kernel, dim3(scan_blocks), dim3(256), 0, st, ws.counts, cells,
                       ws.block_sums);
    hipLaunchKernelGGL(voxels_scan_top_kernel, dim3(1), dim3(1024), 0, st, ws.block_sums, scan_blocks,
                       ws.bias_partials, count_blocks, d_bias);
    hipLaunchKernelGGL(voxels_scan_apply_kernel, dim3(scan_blocks), dim3(256), 0, st, ws.counts, cells,
                       ws.block_sums, n32, ws.offsets);
    hipLaunchKernelGGL(voxels_place_kernel, dim3(grid_for(n)), dim3(256), 0, st, ws.cell, ws.slot, n32,
                       ws.offsets, ws.unsorted);
    hipLaunchKernelGGL(voxels_rank_kernel, dim3(grid_for(n)), dim3(256), 0, st, positions,
                       (const float4*)d_logits, n32, m, ws.cell, ws.offsets, ws.unsorted, ws.entries);
    hipLaunchKernelGGL(voxels_chunks_kernel, dim3(grid_for(n)), dim3(256), 0, st, ws.entries, n32,
                       ws.offsets, ws.chunk_sums);
    hipLaunchKernelGGL(voxels_cells_kernel, dim3(grid_for(n)), dim3(256), 0, st, ws.entries, n32,
                       ws.offsets, ws.chunk_sums);
    hipLaunchKernelGGL(voxels_gather_kernel, dim3(grid_for(cells)), dim3(256), 0, st, ws.offsets,
                       ws.chunk_sums, side, d_volume);
    return check_launch("ffn_voxels_backward");
}
