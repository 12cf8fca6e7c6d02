// What K31 (mesh_raster.hip) and K32 (mesh_raster_grad.hip) share of a (triangle, pixel) pair: the
// constants, the limits and raster_terms().  One function, so K31b, K31c and K32a see the same
// bits.  Both files are compiled with -ffp-contract=off: / is the IEEE division and nothing here
// is contracted into an fma.
#pragma once
#include "common.h"

namespace ffn {

constexpr int kRasterThreads = 256;
constexpr int kRasterMaxSide = 16384;
constexpr float kRasterGuard = 16384.0f;
constexpr uint64_t kRasterEmpty = ~(uint64_t)0;

struct RasterTerms {
    float q0, q1, q2, depth_w;
    bool covered;
};

// What K31b and K31c both need of (triangle, pixel): the same function, so the same bits.
__device__ __forceinline__ RasterTerms raster_terms(int4 r0, int4 r1, int w2_bits, int px, int py) {
    const int64_t x0 = r0.x, y0 = r0.y, x1 = r0.z, y1 = r0.w, x2 = r1.x, y2 = r1.y;
    const float w0 = __int_as_float(r1.z), w1 = __int_as_float(r1.w), w2 = __int_as_float(w2_bits);
    const int64_t area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    const int64_t qx = 256 * (int64_t)px, qy = 256 * (int64_t)py;
    int64_t e0 = (x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1);
    int64_t e1 = (x0 - x2) * (qy - y2) - (y0 - y2) * (qx - x2);
    int64_t e2 = (x1 - x0) * (qy - y0) - (y1 - y0) * (qx - x0);
    if (area < 0) e0 = -e0, e1 = -e1, e2 = -e2;
    const float denominator = (float)(area < 0 ? -area : area);
    RasterTerms t;
    t.covered = e0 >= 0 && e1 >= 0 && e2 >= 0;
    t.q0 = ((float)e0 / denominator) / w0;
    t.q1 = ((float)e1 / denominator) / w1;
    t.q2 = ((float)e2 / denominator) / w2;
    const float inv_w = (t.q0 + t.q1) + t.q2;
    t.depth_w = 1.0f / inv_w;
    return t;
}

inline bool raster_bad_image(int width, int height) {
    return width < 1 || height < 1 || width > kRasterMaxSide || height > kRasterMaxSide;
}

inline bool raster_bad_mesh(int64_t num_vertices, int64_t num_triangles) {
    const int64_t most = 0x7fffffff / 3;
    return num_vertices < 1 || num_vertices > most || num_triangles < 1 || num_triangles > most;
}

}  // namespace ffn
