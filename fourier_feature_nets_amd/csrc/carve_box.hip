// K27  Conservative space carving: one level of a coarse-to-fine carve.  A cell of level k is
// refuted by a camera only when the camera sees all of it and the whole projected footprint of
// the cell lies on the background, so structure thinner than a cell or a pixel is never lost,
// and a cell that passes implies that its parent passes: a coarse level may reject its children.
//
// No reference counterpart.  The mode beside K23 (carve.hip), whose point test stays the default.
// One thread per candidate cell, candidates in path-code order (given as a list, or as the eight
// children of a list of parents: thread i tests (parents[i >> 3] << 3) | (i & 7), so the
// children are never written out), cameras c = 0 .. C-1 in that order.
//
//   points   q0 = oct_cell_center(code, .., depth = k + 1), h = that chain's final half
//            (scale * 0.5^k, every halving rounded on its own); q1 .. q8 = (q0.x -+ h, q0.y -+ h,
//            q0.z -+ h), x slowest: one f32 add or subtract per coordinate
//   project  each point through K23's expression, operation for operation (this file is
//            compiled with -ffp-contract=off): x = ((P00 px + P01 py) + P02 pz) + P03, likewise
//            y and w; in front iff w > 0; fu = x / w + 0.5f, fv = y / w + 0.5f.  A non-finite fu
//            or fv of a point in front leaves the camera undecided for this cell.
//   pixel    col = (int)floorf(clamp(fu, -2^30, 2^30)), row likewise (negative values occur)
//   rect     [c0, c1] x [r0, r1]: min / max of col and row over the points in front, widened by
//            pad = 1 + (depth - 1 - k) pixels on every side
//   inside   all nine in front, not undecided, 0 <= c0, c1 <= W - 1, 0 <= r0, r1 <= H - 1
//   miss     inside and no foreground pixel of the grown mask in the rectangle: four loads from
//            the camera's summed-area table sat[c] ((H + 1, W + 1) int32, sat[r][q] = foreground
//            pixels in rows < r and columns < q; exact integers)
//   seen     some point in front, and (undecided, or some point not in front, or the padded
//            rectangle meets the image)
//   reject   misses > max_misses ends the loop, as in K23.  A camera that cannot see the whole
//            cell (behind it, off the image, partly off the image) cannot refute it.
//   keep     not rejected, and at the finest level (k == depth - 1) also seen >= min_views
//   row      at the finest level only, K23's colour from q0's own projection with K23's
//            operations: in front and on the image, the pixel votes iff its own alpha >= alpha_u8
//            (under a grown mask, mask == 0 implies own alpha < alpha_u8, so the votes K23 skips
//            on a miss never counted); r = (float)sum_r / (float)(255 colored), grey 0.5 without
//            a vote, and sigma0.  A cell both carves keep has the same row bit for bit.
//   select   flag and row -> the K12b/c scan and K16b's stable scatter (octree_select_flagged
//            with first_code = 0, which yields candidate indices), then one gather of the codes.
//
// Why a coarse level may reject its children (the proof obligation of the hierarchy).  A child
// of a level-k cell is a box inside its parent's box.  Where all of the parent is in front of
// the camera (w > 0 on its corners, hence on the box, w being affine), the projection maps the
// box into the convex hull of its projected corners, so in exact arithmetic every projected
// point of the child lies in the bounding rectangle of the parent's projected corners.  The f32
// chain moves each projected coordinate by a rounding error e; as long as 2 e < 1 pixel (it is
// some 1e-4 pixels at 400 x 400), the child's unpadded rectangle lies within one pixel of the
// parent's unpadded rectangle.  The child's pad is exactly one pixel smaller than the parent's,
// so the child's padded rectangle lies inside the parent's padded rectangle: a camera that
// refutes the parent (inside, no foreground in the rectangle) refutes every child, and
// misses(child) >= misses(parent).  The pad's first pixel is the same allowance at the finest
// level: a point of the cell, projected in any arithmetic with error below one pixel, lands
// inside the padded rectangle.
//
// No atomics, no LDS beyond the scan's, no scratch: the nine points are unrolled into scalar
// running minima and maxima (no per-lane array), and the camera's 12 floats sit at a
// wave-uniform address.  Per (cell, camera): 81 products, 81 sums, up to 18 IEEE divisions.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), carve_box_flags_kernel:
// 62 VGPRs, 82 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS, occupancy 8 waves per SIMD
// (carve_box_codes_kernel: 6 VGPRs, 12 SGPRs, no scratch, no spills).
#include "common.h"
#include "octree_cells.h"

namespace ffn {

constexpr int kBoxThreads = 256;
constexpr int kBoxMaxSide = 1 << 24;                // as K23: (float)W and (float)H are exact

struct BoxRect {
    int c0, c1, r0, r1;     // running min / max of the pixels of the points in front
    int front;              // how many of the points so far are in front
    bool undecided;         // a point in front whose pixel coordinate is not finite
};

// One point of the footprint through camera p: K23's expression, then the floor of the clamped
// pixel coordinates into the running rectangle.
__device__ __forceinline__ void box_point(const float* __restrict__ p, float px, float py, float pz,
                                          BoxRect& b) {
#pragma clang fp contract(off)
    const float w = ((p[8] * px + p[9] * py) + p[10] * pz) + p[11];
    if (!(w > 0.0f)) return;
    ++b.front;
    const float x = ((p[0] * px + p[1] * py) + p[2] * pz) + p[3];
    const float y = ((p[4] * px + p[5] * py) + p[6] * pz) + p[7];
    const float fu = x / w + 0.5f, fv = y / w + 0.5f;
    if (!(fabsf(fu) < INFINITY) || !(fabsf(fv) < INFINITY)) {    // an infinity or a NaN
        b.undecided = true;
        return;
    }
    const float limit = 1073741824.0f;                           // 2^30
    const int col = (int)floorf(fminf(fmaxf(fu, -limit), limit));
    const int row = (int)floorf(fminf(fmaxf(fv, -limit), limit));
    b.c0 = min(b.c0, col);
    b.c1 = max(b.c1, col);
    b.r0 = min(b.r0, row);
    b.r1 = max(b.r1, row);
}

__global__ void __launch_bounds__(kBoxThreads)
carve_box_flags_kernel(const uint32_t* __restrict__ images, const int32_t* __restrict__ sat,
                       const float* __restrict__ proj, int cameras, int height, int width,
                       const int32_t* __restrict__ candidates, int64_t count, int expand,
                       int level, float ox, float oy, float oz, float scale, int depth,
                       uint32_t alpha_u8, int max_misses, int min_views, float sigma0,
                       float4* __restrict__ rows, uint8_t* __restrict__ flags,
                       int* __restrict__ visited) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBoxThreads + threadIdx.x;
    if (i >= count) return;
    // i >> 3 < count / 8 entries of the parents' list when expanding (count is a multiple of 8)
    const int64_t code = expand ? (((int64_t)candidates[i >> 3] << 3) | (i & 7))
                                : (int64_t)candidates[i];
    float qx, qy, qz;
    oct_cell_center(code, ox, oy, oz, scale, level + 1, &qx, &qy, &qz);
    float h = scale;                                 // the chain's final half
    for (int l = 0; l < level; ++l) h *= 0.5f;
    const float xl = qx - h, xh = qx + h, yl = qy - h, yh = qy + h, zl = qz - h, zh = qz + h;

    const bool finest = level == depth - 1;
    const int pad = 1 + (depth - 1 - level);
    const float fw = (float)width, fh = (float)height;
    const int64_t pitch = (int64_t)width + 1, table = ((int64_t)height + 1) * pitch;
    int seen = 0, misses = 0, looked = 0;
    uint32_t colored = 0, sum_r = 0, sum_g = 0, sum_b = 0;
    bool carved = false;
    for (int c = 0; c < cameras; ++c) {
        const float* p = proj + 12 * (int64_t)c;    // the same address in every lane
        ++looked;
        BoxRect b = {INT_MAX, INT_MIN, INT_MAX, INT_MIN, 0, false};
        box_point(p, qx, qy, qz, b);
        const bool center_front = b.front > 0;
        box_point(p, xl, yl, zl, b);
        box_point(p, xl, yl, zh, b);
        box_point(p, xl, yh, zl, b);
        box_point(p, xl, yh, zh, b);
        box_point(p, xh, yl, zl, b);
        box_point(p, xh, yl, zh, b);
        box_point(p, xh, yh, zl, b);
        box_point(p, xh, yh, zh, b);
        if (b.front == 0) continue;                 // nothing in front: not seen, not a miss
        if (b.undecided || b.front < 9) {
            ++seen;
        } else {
            // every point in front and finite: |col|, |row| <= 2^30, pad <= 11, no overflow
            const int c0 = b.c0 - pad, c1 = b.c1 + pad, r0 = b.r0 - pad, r1 = b.r1 + pad;
            if (c1 >= 0 && c0 <= width - 1 && r1 >= 0 && r0 <= height - 1) ++seen;
            if (c0 >= 0 && c1 <= width - 1 && r0 >= 0 && r1 <= height - 1) {
                // rows r0 .. r1 + 1 <= height and columns c0 .. c1 + 1 <= width of table c
                const int32_t* t = sat + (int64_t)c * table;
                const int32_t inside = (t[(r1 + 1) * pitch + (c1 + 1)] - t[r0 * pitch + (c1 + 1)])
                                       - (t[(r1 + 1) * pitch + c0] - t[r0 * pitch + c0]);
                if (inside == 0 && ++misses > max_misses) {
                    carved = true;
                    break;
                }
            }
        }
        if (!finest || !center_front) continue;
        // K23's colour vote of the centre, with K23's operations
        const float w = ((p[8] * qx + p[9] * qy) + p[10] * qz) + p[11];
        const float x = ((p[0] * qx + p[1] * qy) + p[2] * qz) + p[3];
        const float y = ((p[4] * qx + p[5] * qy) + p[6] * qz) + p[7];
        const float fu = x / w + 0.5f, fv = y / w + 0.5f;
        if (!(fu >= 0.0f && fu < fw && fv >= 0.0f && fv < fh)) continue;
        // 0 <= col < width and 0 <= row < height: inside image c
        const uint32_t rgba = images[((int64_t)c * height + (int)fv) * width + (int)fu];
        if ((rgba >> 24) >= alpha_u8) {
            sum_r += rgba & 255u;
            sum_g += (rgba >> 8) & 255u;
            sum_b += (rgba >> 16) & 255u;
            ++colored;
        }
    }
    if (visited) visited[i] = looked;
    const bool keep = !carved && (!finest || seen >= min_views);
    flags[i] = keep;
    if (!keep || !finest) return;
    float r = 0.5f, g = 0.5f, bl = 0.5f;
    if (colored > 0) {
        const float denominator = (float)(255u * colored);
        r = (float)sum_r / denominator;
        g = (float)sum_g / denominator;
        bl = (float)sum_b / denominator;
    }
    rows[i] = make_float4(r, g, bl, sigma0);
}

// codes_out[o] holds the index of survivor o in the candidate list (the scatter's "code" with
// first_code = 0); it becomes that candidate's code, each thread in its own slot.
__global__ void __launch_bounds__(kBoxThreads)
carve_box_codes_kernel(const int32_t* __restrict__ candidates, int64_t count, int expand,
                       const int* __restrict__ total, int* __restrict__ codes_out) {
    const int64_t o = (int64_t)blockIdx.x * kBoxThreads + threadIdx.x;
    if (o >= count || o >= *total) return;
    const int64_t i = codes_out[o];                 // 0 <= i < count, written by the scatter
    codes_out[o] = expand ? ((candidates[i >> 3] << 3) | (int)(i & 7)) : candidates[i];
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_octree_carve_box_level(const uint8_t* images, const int32_t* sat,
                                          const float* proj, int cameras, int height, int width,
                                          const int32_t* candidates, int64_t count, int expand,
                                          int level, float center_x, float center_y,
                                          float center_z, float scale, int depth, int alpha_u8,
                                          int max_misses, int min_views, float sigma0,
                                          uint8_t* flags, int* offsets, int* tile_sums,
                                          float* rows, int* visited, int* codes_out,
                                          float* data_out, int* total, void* stream) {
    if (depth < 1 || depth > ffn_octree_max_depth())
        return fail_arg("ffn_octree_carve_box_level: shape (1 <= depth <= 11)");
    if (level < 0 || level > depth - 1)
        return fail_arg("ffn_octree_carve_box_level: level must lie in 0 .. depth - 1");
    if (count < 1 || count > ffn_octree_max_points() || (expand && (count & 7) != 0))
        return fail_arg("ffn_octree_carve_box_level: shape (1 <= count < 2^31 candidates, a "
                        "multiple of 8 when expand is set)");
    if (expand != 0 && expand != 1)
        return fail_arg("ffn_octree_carve_box_level: expand is 0 or 1");
    if (expand && level < 1)
        return fail_arg("ffn_octree_carve_box_level: expand needs level >= 1 (level 0 has no "
                        "parent)");
    if (cameras < 1 || cameras > ffn_octree_carve_max_cameras())
        return fail_arg("ffn_octree_carve_box_level: 1 <= cameras <= 65793 (255 * cameras must "
                        "be exact in f32)");
    if (height < 1 || width < 1 || height > kBoxMaxSide || width > kBoxMaxSide)
        return fail_arg("ffn_octree_carve_box_level: images (1 <= height, width <= 2^24)");
    if ((int64_t)height * width >= ((int64_t)1 << 31))
        return fail_arg("ffn_octree_carve_box_level: images (height * width < 2^31: the "
                        "summed-area table holds int32 counts)");
    if (alpha_u8 < 1 || alpha_u8 > 255 || max_misses < 0 || min_views < 0)
        return fail_arg("ffn_octree_carve_box_level: 1 <= alpha_u8 <= 255, max_misses >= 0, "
                        "min_views >= 0");
    if (!images || !sat || !proj || !candidates || !flags || !offsets || !tile_sums || !rows ||
        !codes_out || !data_out || !total)
        return fail_arg("ffn_octree_carve_box_level: null argument");
    if ((((uintptr_t)images | (uintptr_t)sat | (uintptr_t)candidates) & 3) != 0 ||
        (((uintptr_t)rows | (uintptr_t)data_out) & 15) != 0)
        return fail_arg("ffn_octree_carve_box_level: images, sat and candidates must be 4-byte "
                        "aligned, rows and data_out 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((count + kBoxThreads - 1) / kBoxThreads);
    hipLaunchKernelGGL(carve_box_flags_kernel, dim3(blocks), dim3(kBoxThreads), 0, s,
                       (const uint32_t*)images, sat, proj, cameras, height, width, candidates,
                       count, expand, level, center_x, center_y, center_z, scale, depth,
                       (uint32_t)alpha_u8, max_misses, min_views, sigma0, (float4*)rows, flags,
                       visited);
    if (int err = octree_select_flagged(flags, rows, 0, count, offsets, tile_sums, codes_out,
                                        data_out, total, s))
        return err;
    hipLaunchKernelGGL(carve_box_codes_kernel, dim3(blocks), dim3(kBoxThreads), 0, s, candidates,
                       count, expand, total, codes_out);
    return check_launch("ffn_octree_carve_box_level");
}
