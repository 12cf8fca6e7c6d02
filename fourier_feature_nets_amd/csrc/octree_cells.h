// What the dense-grid builders (K16 in octree.hip, K23 in carve.hip) share: the centre of a finest
// cell from its path code, and the select tail that turns per-cell flags and rows into the kept
// cells in code order.
#pragma once
#include "common.h"

namespace ffn {

// Centre of the finest cell (level depth - 1) with path code `code`: the f32 chain +-scale / 2^k
// from 0, level by level from the root as K12k makes it for the cell's id, then one f32 add of
// the cube centre.  Every operation is rounded on its own.
__device__ __forceinline__ void oct_cell_center(int64_t code, float ox, float oy, float oz,
                                                float scale, int depth, float* x, float* y,
                                                float* z) {
#pragma clang fp contract(off)
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, half = scale;
    for (int level = 1; level < depth; ++level) {
        const int child = (int)((code >> (3 * (depth - 1 - level))) & 7);
        half *= 0.5f;
        cx = (child & 4) ? cx + half : cx - half;
        cy = (child & 2) ? cy + half : cy - half;
        cz = (child & 1) ? cz + half : cz - half;
    }
    *x = cx + ox;
    *y = cy + oy;
    *z = cz + oz;
}

// octree.hip.  flags (count) and rows (count,4; read where the flag is set) of the cells
// first_code .. first_code + count - 1 -> the K12b/c scan and the stable scatter: codes_out and
// data_out (count entries each) hold the flagged cells in code order, *total (device) of them.
// The caller has checked the arguments and checks the launch.
// octree.hip.  The K12b/c exclusive scan of n u8 flags (n <= ffn_octree_max_points()): offsets (n),
// *total (device) the number of set flags; tile_sums holds ffn_octree_scan_tiles(n) ints.
int octree_scan_flags(const uint8_t* flags, int64_t n, int* tile_sums, int* offsets, int* total,
                      hipStream_t stream);

int octree_select_flagged(const uint8_t* flags, const float* rows, int64_t first_code,
                          int64_t count, int* offsets, int* tile_sums, int* codes_out,
                          float* data_out, int* total, hipStream_t stream);

}  // namespace ffn
