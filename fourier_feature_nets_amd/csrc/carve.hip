// K23  Space carving: which finest cells of the root cube can be part of the object, judged from
// the images' silhouettes alone, and a first colour for them.
//
// No reference counterpart (the reference gets a tree from a mesh or from a trained model's depth
// renders only).  This is the grid loop of K16 with the model replaced by a projection: a chunk
// holds the cells first_code .. first_code + count - 1 in path-code order (K16a's order, so
// neighbouring lanes are neighbouring cells and read neighbouring pixels), one thread per cell.
//
//   centre   oct_cell_center (octree_cells.h): the f32 chain of K16a, cube centre included
//   project  camera c = 0 .. C-1 in that order, P = proj[c] (3x4 f32, row-major):
//              x = ((P00 px + P01 py) + P02 pz) + P03, likewise y (row 1) and w (row 2), every
//              product and sum rounded on its own (this file is compiled with -ffp-contract=off)
//              !(w > 0): the camera does not see the cell (NaN falls here)
//              fu = x / w + 0.5f, fv = y / w + 0.5f (IEEE divisions)
//              seen iff fu >= 0 && fu < W && fv >= 0 && fv < H; col = (int)fu, row = (int)fv: the
//              nearest pixel, pixel (x, y) being the ray through the integer coordinates (x, y)
//   vote     seen += 1.  mask[c, row, col] == 0: misses += 1, and once misses > max_misses the
//            loop ends, the cell is carved.  Otherwise the pixel's own RGBA (one aligned 4-byte
//            load); if its alpha >= alpha_u8 its three channels go into three uint32 sums and
//            colored += 1.  Integer sums: exact, whatever the order.
//   keep     iff not carved and seen >= min_views.  row = [r, g, b, sigma0] with
//            r = (float)sum_r / (float)(255 colored), one f32 division per channel; 0.5f for all
//            three when colored == 0.  255 C <= 2^24 keeps both operands exact in f32: at most
//            kCarveMaxCameras = 65793 cameras, refused above.
//   select   flag and row -> the K12b/c scan and K16b's stable scatter (octree_select_flagged).
//
// No atomics, no LDS beyond the scan's, no scratch.  A carved cell leaves the loop at its first
// max_misses + 1 background pixels, so the cost is about (kept cells x C) + (empty cells x a few
// cameras); lanes of a wave wait for its longest-lived cell.  This test cannot be run coarse to
// fine: it is a point sample of the cell centre, which is not conservative (a coarse cell whose
// centre falls on the background can have children whose centres do not), so a coarse level
// cannot safely reject its children.  The hierarchical carve is K27 (carve_box.hip), which tests
// a cell's whole projected footprint instead.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), carve_flags_kernel:
// 27 VGPRs, 58 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS, occupancy 8
// waves per SIMD.
#include "common.h"
#include "octree_cells.h"

namespace ffn {

constexpr int kCarveThreads = 256;
constexpr int kCarveMaxCameras = (1 << 24) / 255;   // 255 C <= 2^24
constexpr int kCarveMaxSide = 1 << 24;              // (float)W and (float)H are exact

__global__ void __launch_bounds__(kCarveThreads)
carve_flags_kernel(const uint32_t* __restrict__ images, const uint8_t* __restrict__ mask,
                   const float* __restrict__ proj, int cameras, int height, int width,
                   int64_t first_code, int64_t count, float ox, float oy, float oz, float scale,
                   int depth, uint32_t alpha_u8, int max_misses, int min_views, float sigma0,
                   float4* __restrict__ rows, uint8_t* __restrict__ flags,
                   int* __restrict__ visited) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kCarveThreads + threadIdx.x;
    if (i >= count) return;
    float px, py, pz;
    oct_cell_center(first_code + i, ox, oy, oz, scale, depth, &px, &py, &pz);

    const float fw = (float)width, fh = (float)height;
    int seen = 0, misses = 0, looked = 0;
    uint32_t colored = 0, sum_r = 0, sum_g = 0, sum_b = 0;
    bool carved = false;
    for (int c = 0; c < cameras; ++c) {
        const float* p = proj + 12 * (int64_t)c;    // the same address in every lane
        ++looked;
        const float w = ((p[8] * px + p[9] * py) + p[10] * pz) + p[11];
        if (!(w > 0.0f)) continue;
        const float x = ((p[0] * px + p[1] * py) + p[2] * pz) + p[3];
        const float y = ((p[4] * px + p[5] * py) + p[6] * pz) + p[7];
        const float fu = x / w + 0.5f, fv = y / w + 0.5f;
        if (!(fu >= 0.0f && fu < fw && fv >= 0.0f && fv < fh)) continue;
        // 0 <= col < width and 0 <= row < height: inside image c of both arrays
        const int64_t pixel = ((int64_t)c * height + (int)fv) * width + (int)fu;
        ++seen;
        if (mask[pixel] == 0) {
            if (++misses > max_misses) {
                carved = true;
                break;
            }
            continue;
        }
        const uint32_t rgba = images[pixel];        // bytes r, g, b, a from the lowest up
        if ((rgba >> 24) >= alpha_u8) {
            sum_r += rgba & 255u;
            sum_g += (rgba >> 8) & 255u;
            sum_b += (rgba >> 16) & 255u;
            ++colored;
        }
    }
    if (visited) visited[i] = looked;
    const bool keep = !carved && seen >= min_views;
    flags[i] = keep;
    if (!keep) return;
    float r = 0.5f, g = 0.5f, b = 0.5f;
    if (colored > 0) {
        const float denominator = (float)(255u * colored);
        r = (float)sum_r / denominator;
        g = (float)sum_g / denominator;
        b = (float)sum_b / denominator;
    }
    rows[i] = make_float4(r, g, b, sigma0);
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_octree_carve_max_cameras(void) { return kCarveMaxCameras; }

extern "C" int ffn_octree_carve_select(const uint8_t* images, const uint8_t* mask,
                                       const float* proj, int cameras, int height, int width,
                                       int64_t first_code, int64_t count, float center_x,
                                       float center_y, float center_z, float scale, int depth,
                                       int alpha_u8, int max_misses, int min_views, float sigma0,
                                       uint8_t* flags, int* offsets, int* tile_sums, float* rows,
                                       int* visited, int* codes_out, float* data_out, int* total,
                                       void* stream) {
    if (depth < 1 || depth > ffn_octree_max_depth())
        return fail_arg("ffn_octree_carve_select: shape (1 <= depth <= 11)");
    if (count < 1 || count > ffn_octree_max_points() || first_code < 0 ||
        first_code + count > ((int64_t)1 << (3 * (depth - 1))))
        return fail_arg("ffn_octree_carve_select: shape (count >= 1, codes inside "
                        "[0, 8^(depth-1)))");
    if (cameras < 1 || cameras > kCarveMaxCameras)
        return fail_arg("ffn_octree_carve_select: 1 <= cameras <= 65793 (255 * cameras must be "
                        "exact in f32)");
    if (height < 1 || width < 1 || height > kCarveMaxSide || width > kCarveMaxSide)
        return fail_arg("ffn_octree_carve_select: images (1 <= height, width <= 2^24)");
    if (alpha_u8 < 1 || alpha_u8 > 255 || max_misses < 0 || min_views < 0)
        return fail_arg("ffn_octree_carve_select: 1 <= alpha_u8 <= 255, max_misses >= 0, "
                        "min_views >= 0");
    if (!images || !mask || !proj || !flags || !offsets || !tile_sums || !rows || !codes_out ||
        !data_out || !total)
        return fail_arg("ffn_octree_carve_select: null argument");
    if (((uintptr_t)images & 3) != 0 || (((uintptr_t)rows | (uintptr_t)data_out) & 15) != 0)
        return fail_arg("ffn_octree_carve_select: images must be 4-byte aligned, rows and "
                        "data_out 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((count + kCarveThreads - 1) / kCarveThreads);
    hipLaunchKernelGGL(carve_flags_kernel, dim3(blocks), dim3(kCarveThreads), 0, s,
                       (const uint32_t*)images, mask, proj, cameras, height, width, first_code,
                       count, center_x, center_y, center_z, scale, depth, (uint32_t)alpha_u8,
                       max_misses, min_views, sigma0, (float4*)rows, flags, visited);
    if (int err = octree_select_flagged(flags, rows, first_code, count, offsets, tile_sums,
                                        codes_out, data_out, total, s))
        return err;
    return check_launch("ffn_octree_carve_select");
}
