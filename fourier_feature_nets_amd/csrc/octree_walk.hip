// K13  Ray walk through the sparse octree of K12: the regions a ray crosses, in order.
//
// Replaces the host-side (Python / Numba, one ray at a time) walker of the reference:
// octree.py:418-482 (_trace_ray_path), octree.py:485-501 (_batch_intersect) behind
// OcTree.intersect (octree.py:707-731).
//
// A REGION is a leaf, or a maximal empty cell: a child slot of an interior node that is in
// neither index.  The regions tile the root cube, so a ray that hits the cube crosses a sequence
// of them; stop k of a ray is the t at which it enters its k-th region and that region's index
// into leaf_index (-1 for an empty cell).
//
// Where the ray is, and where it goes next, is decided on INTEGERS: the ray owns a cell
// (ix, iy, iz) of the finest grid, 2^(depth-1) cells per axis.  The region of a cell is found by
// descending from the root along the cell's bits (binary searches in the two sorted id arrays,
// as K12j).  Leaving a region, the cell steps across the exit face on the exit axis -- to the
// first cell beyond the region, an integer operation that cannot land inside the region again --
// and on the other two axes takes the cell of the exit point inside the region's own range,
// never moving against the ray's direction.  There is no epsilon nudge and no re-test of a
// moved point (the reference advances by t += 1e-5 until a containment test fails; its own
// comment asks for integers).
//
// Floating point only produces the t-values: the entry of a region is the crossing of its
// bounding plane, (plane - o) / d in f32, with plane = c +- scale / 2^k from the f32 chain of
// node centres that K12e / K12j / K12k replay (this file is compiled with -ffp-contract=off).
//
// One lane per ray, no stack and no per-lane array: the state is the node id, its level, its
// centre and the three cell coordinates.  After a step the descent starts again at the root, but
// the levels above the deepest common ancestor of the old and the new cell are known to be
// interior and are replayed in registers without a lookup.  Rays of one wave diverge in trip
// count (the wave runs as long as its longest ray), so a workgroup is ONE wave: a long ray holds
// back 63 neighbours, not 255, and a finished wave frees its slot at once.  The kernel is bound
// by the latency of dependent L2 reads (the binary searches); neighbouring rays search the same
// ids, so the top of both arrays stays in cache.
//
// K14  First hit: the same walk, ended at the first leaf whose exit t is > t_min (the predicate of
// the span form).  The leaves of a voxelized model are opaque surface cells with one colour each
// and no density, so the first one a ray meets IS the render: no stop arrays, no compositing.  The
// hit gives the leaf, its entry t (depth) and the face the ray came in through -- the exit axis of
// the region before it -- and, in the same launch, the leaf's colour.  Replaces the scenepic view
// of the leaf cubes (voxelize_model.py:90-110 of the reference) on top of octree.py:418-501.
//
// K15  Volume: the same walk, composited front to back.  A baked tree (ffn_octree_bake) holds the
// model's own colour and density in every leaf; the walk has the entry and the exit t of a leaf in
// registers, so the chord, its opacity 1 - exp(-sigma * length) and the running transmittance are
// a handful of VALU operations per leaf on top of one 16-byte load, and nothing is written per
// stop.  The walk ends early once the transmittance is at or below a threshold.  No counterpart in
// the reference.
//
// K17a  Gradient walk: the backward of K15, a fifth mode of the same kernel (same integer stepping,
// same t0, chord, sigma = max(data[leaf,3], 0) and early end, same f32 operations in the same
// order, so the colour it accumulates has the forward's bits).  With x_k = sigma_k L_k,
// a_k = 1 - exp(-x_k), T_k = prod_{j<k}(1 - a_j), w_k = T_k a_k, C = sum w_k c_k + T_{n+1} bg and
// upstream gradients g_C, g_A, taken leaf k of a ray gets ONE entry
//     d c_k     = w_k g_C
//     d sigma_k = L_k [ g_C . (T_{k+1} c_k - S_k) + g_A T_{n+1} ],   S_k = C - sum_{j<=k} w_j c_j
// (0 where the stored density is negative or NaN; it passes at exactly 0).  C and T_{n+1} come from
// a FIRST WALK of this same mode, not from the forward's outputs: the entries of a ray need a
// place in the entry list, so its taken leaves have to be counted before anything is written, and
// the walk that counts them composites on the way (phase 0: count, C, T_{n+1} per ray; phase 1,
// after a scan of the counts: the entries, ray-major at offsets[ray] + k).  T_{n+1} is then the
// transmittance itself and not 1 - alpha.  The per-leaf sums are K17b (csrc/octree_grad.hip).
// The mode reuses the parameters the other modes leave idle (see grad_walk below) so that their
// instantiations are compiled from unchanged code.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), kGrad: 61 VGPRs, 99 SGPRs,
// 0 bytes of scratch, 0 spills, 0 bytes of LDS, occupancy 8 waves/SIMD; the other four instantiations
// compile to the instructions they had before the mode existed (38 / 40 / 50 / 53 VGPRs).
// Divergence and dependent reads: as K15, a wave runs as long as its longest ray (one wave per
// workgroup) and waits on the binary searches; the entry stores are one 16-byte and one 4-byte
// store per lane and leaf into the lane's own run of the list, off the dependent chain.
//
// K18a  SH volume: K15 with a view-dependent leaf colour, two more modes of the same kernel (one per
// degree, B = (degree + 1)^2 = 4 or 9).  A leaf holds 3 B logit-space coefficients and a density;
// its colour for the ray's unit direction u is sigmoid(sum_b k_cb Y_b(u)), Y the real SH basis
// (sh_terms below).  u is constant along a ray: the B basis values are computed once before the
// loop and stay in registers, and a leaf costs B fused multiply-adds and one sigmoid per channel
// on top of K15's steps.  t0, the chord, sigma, a, w, T, the depth and the early end are K15's
// operations in K15's order, so alpha and depth have K15's bits on the same densities.  The device
// copy of the leaf data is a layout of its own: rows of `stride` floats, a multiple of four and
// 16-byte aligned, [sigma, k_r0 .. k_r(B-1), k_g0 .., k_b0 .., padding], read as stride / 4
// 16-byte loads (4 at degree 1, 7 at degree 2) of which the first holds the density.  first.channels
// carries the stride.  No counterpart in the reference.
// Resource report, kVolumeSH1 / kVolumeSH2: 56 / 72 VGPRs (occupancy 8 / 7 waves per SIMD), 0 bytes
// of scratch, 0 spills, 0 bytes of LDS; the five older instantiations compile to the instructions
// they had before (38 / 40 / 50 / 53 / 61 VGPRs).
//
// K19a  Gradient walk through SH leaves: the backward of K18a, two more modes (kGradSH1 / kGradSH2),
// to K18a what K17a is to K15: the same two phases (0 counts and composites, 1 emits), the same reuse
// of idle parameters (first.leaf carries the entries' ray numbers), and K18a's arithmetic operation
// for operation for t0, the chord, sigma, a, w, T, the basis Y(u) (csrc/sh_terms.h) and the colour
// c = sigmoid(k . Y(u)), so phase 0 reproduces the forward's C and T_{n+1} bit for bit.  Taken leaf k
// of a ray leaves ONE narrow entry, as K17a:
//     (e_r, e_g, e_b) with e_c = (w_k g_c) (c_kc (1 - c_kc)),   d sigma_k as K17a with the sigmoid colour
// plus the leaf's and the ray's number; d k_cb = e_c Y_b(u) is formed where the entries are summed
// (K19b, csrc/octree_grad.hip): the rank-one factor belongs to the ray, not to the entry.
// Resource report, kGradSH1 / kGradSH2: 64 / 82 VGPRs, 102 / 102 SGPRs, 0 bytes of scratch, 0 spills,
// 0 bytes of LDS, occupancy 7 / 5 waves per SIMD (kGradSH1 is held to 7 by its 102 SGPRs; the whole row is held as in K18a: 7 16-byte loads at
// degree 2; it did not need to be consumed channel by channel).  The seven older instantiations
// compile to the instructions they had before (38 / 40 / 50 / 53 / 61 / 56 / 72 VGPRs).
//
// K21a  Per-leaf maximum weight: a tenth mode (kLeafWeight).  K15's walk without its colours and without
// any per-ray output: the taken-leaf rule, t0, the chord, sigma = max(density, 0), a, w = T a, T and the
// early end are K15's operations in K15's order, so w has the bits K15 composites with.  The density is
// read alone, at first.shading floats into a row of first.channels floats (3 of 4 on plain rows, 0 of
// 16 / 28 on the SH device layout): one mode serves plain and SH trees.  Per taken leaf with w > 0 the
// walk raises weights[leaf] to w.  weights holds f32 bit patterns as uint32: for w >= 0 the pattern is
// monotone in w, so the maximum is an INTEGER atomicMax -- exact, and independent of the order of the
// rays and of how they are split over calls (no float atomic, the same bits every call).  The atomic
// returns nothing to the lane and sits off the dependent chain of the binary searches.  Contention: the
// lanes of a wave are neighbouring rays and often sit in the same leaf, and a leaf in front of the
// camera is hit by thousands of rays; same-address atomics are serialised in L2.  A plain load comes
// first and the atomic is skipped when the stored value is already >= w: after the first few rays a
// hot leaf costs a cached load.  The load may be stale (a value only grows), which can only send an
// atomic that changes nothing: the result does not depend on the shortcut.
// The idle parameters carry its buffers, as for kGrad: span_hit the uint32 weights, first.shading the
// density's offset in a row.
// Resource report, kLeafWeight: 39 VGPRs, 80 SGPRs, 0 bytes of scratch, 0 spills,
// 0 bytes of LDS, occupancy 8 waves per SIMD; the nine older instantiations compile to the
// instructions they had before (38 / 40 / 50 / 53 / 61 / 56 / 72 / 64 / 82 VGPRs).
//
// K24  Visible votes: an eleventh mode (kVisible).  A lane is a (leaf, camera) pair -- the leaf from
// blockIdx.x and the lane, the camera from blockIdx.y, so one launch covers every camera of a call and a
// small tree still fills the chip with waves -- and the L x C rays exist in registers only.  The lane
// projects its leaf's centre with K23's operations (csrc/carve.hip) through the camera's block of 16
// floats (P' for cube-relative points, the eye; the block's address is uniform in a workgroup, so it
// arrives by scalar loads), and leaves before the first tree lookup when the centre lies behind the
// camera, off the image, or on a pixel whose alpha is below alpha_u8.  Otherwise the ray o = eye,
// d = centre - eye (the centre at t = 1) takes K21a's walk with t_min = 0: the taken-leaf rule, t0, the
// chord, sigma = max(density, 0), a, T and the early end are K21a's operations in K21a's order, and the
// walk ends "visible" at the lane's own leaf, "occluded" once T <= min_transmittance, and not visible
// when it runs out.  A visible pair adds the pixel's r, g, b and 1 to its leaf's four uint32 fields as
// two 64-bit INTEGER atomic adds of two fields each (a sum stays below 2^24 and the count below 2^17,
// so no carry crosses a field): exact, whatever the order of the cameras and however they are split
// over calls; no float atomic.  The atomics return nothing and come after the walk.  Contention: the C
// cameras of a leaf share its two words, the lanes of a wave write 1 KiB of neighbouring words.
// Divergence: lanes rejected before the walk idle while the wave's longest walk runs; neighbouring
// lanes are neighbouring leaves of one camera, so their walks are alike.  The idle parameters carry
// its buffers (see kVisible above the kernel); the kernel's parameter list is unchanged.
// Resource report, kVisible: 39 VGPRs, 89 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS,
// occupancy 8 waves per SIMD.  The ten older instantiations compile to the instructions they had
// before: their disassembly was compared with the previous commit's, instruction for instruction
// (758 / 809 / 851 / 887 / 975 / 1002 / 1034 / 1095 / 1132 / 845 instructions, 38 / 40 / 50 / 53 / 61 /
// 56 / 72 / 64 / 82 / 39 VGPRs).
//
// K26  Focus samples from the tree's own weights: a SIBLING kernel (octree_focus_kernel), not a twelfth
// mode.  It needs a per-ray id gather, near and far, a loop over two phases around the walk and a merge
// state of its own, none of which fits the idle parameters, so it takes its arguments as one struct and
// shares the device functions above (find_id, chain_bits, root_slab, exit_t, step_axis) and K13's loop
// bounds.  One lane per ray in one-wave workgroups, as the modes.  Per taken leaf (t0 = max(t, near),
// t1 = min(t_exit, far), t1 > t0) K21a's chain sigma = max(density, 0), a, w = T a, T, and the running
// sum c of w.  The walk is ONE piece of code run for phase 0 (M = c at the end) and phase 1 (the
// targets y_j = u_j M are placed where c passes them, linearly inside the leaf), so the second walk
// repeats the first one's c bit for bit by construction, not by the compiler's grace.  Rays without
// mass, rays that miss and rays with an empty [near, far] emit the uniform fall-back.
// The emits: DIRECT per-lane row stores.  A lane owns row r of the (R, S) output and writes it front to
// back, merging its ascending emits with the row's uniform samples by two pointers (the next uniform
// sample waits in a register); lanes of a wave write 4 bytes each at a stride of 4 S bytes, so a store
// instruction touches up to 64 lines, and a line is completed by 16 consecutive emits of one lane while
// it sits in L2.  Staging a wave's rows through LDS for whole-line stores was not built, so there is no
// measurement to set against this one; the stores are off the dependent chain of the binary searches
// that bounds the walk.  No LDS, no atomics, no limit on S.
// Divergence: as every mode a wave runs as long as its longest ray, here for two walks; the inner emit
// loop runs as long as the lane with the most targets in the current leaf.
// Resource report, octree_focus_kernel: 75 VGPRs, 106 SGPRs (6 of them spilled to VGPR lanes, none to
// memory), 0 bytes of scratch, 0 VGPR spills, 0 bytes of LDS, occupancy 6 waves per SIMD, 1316
// instructions.  The eleven instantiations of octree_walk_kernel compile to the instructions they had
// before: their disassembly was compared with the previous commit's, instruction for instruction
// (758 / 809 / 851 / 887 / 975 / 1002 / 1034 / 1095 / 1132 / 845 / 959 instructions).
// Measured (MI355X, profiles/r24_octree_focus_microbench.json, S = 128, best of 5): 9.61 ms for 4096 shuffled
// rays and 16.59 ms for 160 000 rays of one camera in a depth-8 carved tree, 2.1x / 2.2x K15's one walk on the
// same rays (4.57 / 7.71 ms); depth 10: 37.24 / 71.58 ms, 2.1x.  Latency-bound like every mode: 4096 rays are 64
// waves.  Kernel times under rocprofv3 and LDS-staged emits were not measured.
//
// K28a  Visible moments: a twelfth mode (kVisibleMoments), kVisible operation for operation -- the
// pair, the projection, the early rejects, the walk, the taken-leaf rule, the transmittance and the
// three endings are the same code (kSees below) -- with a wider write-back: a leaf's row is eight
// uint32, [sum_r, sum_g, sum_b, count, sq_r, sq_g, sq_b, 0], and a visible pair sends FOUR 64-bit
// integer atomic adds of two fields each: K24's two words, then [sq_r, sq_g] and [sq_b, 0] with
// sq_c = c c of the pixel's byte.  The atomics return nothing and come after the walk; no float
// atomic.  The limit: a square is at most 65025 and 65025 C < 2^32 holds for C <= 66051 cameras folded
// into one buffer (kMomentsMaxCameras, the caller's to keep), so no carry crosses a field and the
// sums are exact in any order of the cameras, in one call or split over many.  The lanes of a wave
// write 2 KiB of neighbouring words.  Not a sibling kernel: it needs nothing that the idle parameters
// cannot carry (`leaves` is the moments buffer).
// Resource report, kVisibleMoments: 39 VGPRs, 89 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of
// LDS, occupancy 8 waves per SIMD, 966 instructions (kVisible's 959 and seven: the squares, the
// two further atomics and their operands).  The eleven older instantiations and octree_focus_kernel compile
// to the instructions they had before: their disassembly was compared with the previous commit's,
// instruction for instruction (758 / 809 / 851 / 887 / 975 / 1002 / 1034 / 1095 / 1132 / 845 / 959
// and 1316 instructions; 38 / 40 / 50 / 53 / 61 / 56 / 72 / 64 / 82 / 39 / 39 and 75 VGPRs).
//
// K29  Per-ray distortion (the distortion loss of Mip-NeRF 360 on the piecewise-constant weights of
// an octree ray): four more modes.  With the taken leaves of K15 in walk order, their w_k = T_k a_k,
// L_k and the chord's midpoint m_k = (0.5 (t0_k + t_exit_k)) |d| as a world length, and the running
// (exclusive) W_k = sum_{j<k} w_j, M_k = sum_{j<k} w_j m_j,
//     D = sum_k [ (2 w_k) (m_k W_k - M_k) + (w_k w_k) (L_k / 3) ]
// which is sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 L_i because the leaves are disjoint and
// ordered along the ray: O(n) per ray, three more registers, no per-lane array.
// K29a (kDistortion), built as kLeafWeight is: the density alone at first.shading floats into a row of
// first.channels floats, t0, the chord, sigma, a, w, T and the early end K15's operations in K15's
// order, dist_step() per taken leaf, and ONE store per ray (first.depth, +0 for a ray that takes no
// leaf).  Nothing per leaf, no atomics.
// K29b (kGradDist / kGradSH1Dist / kGradSH2Dist): kGrad / kGradSH1 / kGradSH2 with the term folded into
// their two walks -- the SAME branches of the loop, with the additions under `if (kDist)`, so that
// t0, the chord, sigma, a, w, T and the colour arithmetic are the parents' operations in their order.
// Phase 0 runs dist_step() (the one piece of code K29a runs: D has K29a's bits on the same rays and
// densities) and also leaves W_tot, M_tot and D per ray (first.depth, n x 3) and D for the caller
// (first.t_hit, may be null).  Phase 1 keeps the running W, M and P_k = sum_{j<=k} w_j G_j and adds to
// the d sigma of the entry it writes anyway
//     pad * L_k [ T_{k+1} G_k - (2 D - P_k) ]          pad carries dist_scale: one multiply, one add
//     G_k = 2 [ (m_k W_k - M_k) + (M_tot - M_{k+1}) - m_k (W_tot - W_{k+1}) ] + (2/3) (w_k L_k)
// (sum_j w_j G_j = 2 D, D being homogeneous of degree 2 in w, so the sum over the leaves BEHIND k
// needs no third walk); 0 where the stored density is negative or NaN, K17a's rule.  The entry list,
// K17b / K19b and everything behind them are unchanged; no float atomics.  The differences
// 2 D - P_k and M_tot - M_{k+1} cancel towards the end of a ray: their error is one ulp of D and of
// the ray's length per step, absolute, which the tests' budget counts.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), kGradDist / kGradSH1Dist /
// kGradSH2Dist: 74 / 80 / 91 VGPRs (their parents: 61 / 64 / 82), 106 / 106 / 106 SGPRs, 0 bytes of
// scratch, 0 spills, 0 bytes of LDS, occupancy 6 / 6 / 5 waves per SIMD (their parents: 8 / 7 / 5).
// kDistortion: 47 VGPRs, 84 SGPRs, 0 bytes of scratch, 0 spills, 0 bytes of LDS, occupancy 8.
// The twelve older instantiations and octree_focus_kernel compile to the instructions they had
// before: their disassembly (hipcc -S, labels renumbered) was compared with the previous commit's,
// instruction for instruction.
#include "common.h"
#include "composite_terms.h"
#include "octree_grad.h"
#include "sh_terms.h"

namespace ffn {

constexpr int kWalkThreads = 64;
constexpr int kWalkMaxDepth = 11;     // as K12's path codes: at most 10 levels below the root
static const int64_t kWalkMaxRays = (int64_t)1 << 31;
constexpr int kVisibleMaxSide = 1 << 24;              // (float)W and (float)H are exact
constexpr int kVisibleMaxLaunchCameras = 65535;       // gridDim.y
constexpr int kMomentsMaxCameras = 66051;             // K28a: 255 * 255 * C < 2^32 (the caller's to keep)
static_assert(65025ull * kMomentsMaxCameras < (1ull << 32) &&
              65025ull * (kMomentsMaxCameras + 1) >= (1ull << 32), "the field bound of K28a");

// is key in the sorted ids?  *at = its position
__device__ __forceinline__ bool find_id(const int64_t* __restrict__ ids, int64_t n, int64_t key,
                                        int64_t* at) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    *at = lo;
    return lo < n && ids[lo] == key;
}

// `count` levels of the one-axis centre chain below centre c (half = the half side at c): the
// bits of p's cell, highest first.  The octree.py:274-286 comparison, one axis of K12e's descend.
__device__ __forceinline__ int chain_bits(float p, float c, float half, int count) {
    int bits = 0;
    for (int k = 0; k < count; ++k) {
        half *= 0.5f;
        const bool up = p >= c;
        c = up ? c + half : c - half;
        bits = (bits << 1) | (up ? 1 : 0);
    }
    return bits;
}

// one axis of the root cube [-scale, scale] against o + t d.  A zero component constrains
// nothing when o lies in the slab and misses otherwise.
__device__ __forceinline__ void root_slab(float o, float d, float scale, int axis, float& t_in,
                                          float& t_out, int& axis_in, bool& miss) {
    if (d == 0.0f) {
        miss = miss || !(fabsf(o) <= scale);
        return;
    }
    const float near = ((d > 0.0f ? -scale : scale) - o) / d;
    const float far = ((d > 0.0f ? scale : -scale) - o) / d;
    miss = miss || near != near || far != far;
    if (near > t_in) { t_in = near; axis_in = axis; }
    if (far < t_out) t_out = far;
}

// t at which o + t d leaves the slab c +- half on one axis (+inf: never, on this axis)
__device__ __forceinline__ float exit_t(float o, float d, float c, float half) {
    if (d == 0.0f || d != d) return __builtin_inff();
    return ((d > 0.0f ? c + half : c - half) - o) / d;
}

// The cell coordinate on one axis after leaving a region that spans 2^span cells from
// (i >> span) << span.  On the exit axis: the first cell beyond the region.  Elsewhere: the cell
// of the exit point p inside the region's range, not behind the cell the ray already owns.
__device__ __forceinline__ int step_axis(int i, bool is_exit_axis, float d, float p, float c,
                                         float half, int span) {
    const int base = (i >> span) << span;
    if (is_exit_axis) return d > 0.0f ? base + (1 << span) : base - 1;
    if (d == 0.0f || d != d) return i;
    const int at = base | chain_bits(p, c, half, span);
    return d > 0.0f ? max(i, at) : min(i, at);
}

// one factor per axis pair, 1 for a clamped entry (face 6): FFN_OCTREE_FACE_SHADE without a table
// in memory (a table indexed per lane would live in scratch)
__device__ __forceinline__ float face_shade(int face) {
    const int pair = face >> 1;
    return pair == 0 ? FFN_OCTREE_SHADE_X
                     : pair == 1 ? FFN_OCTREE_SHADE_Y : pair == 2 ? FFN_OCTREE_SHADE_Z : 1.0f;
}

// what only the first-hit and the volume mode read and write; any of leaf / t_hit / face, and all
// of color / alpha / depth together, may be null in the first-hit mode.  The volume mode reads
// four channels (colour and density) and writes color / alpha / depth only.
struct FirstHit {
    int64_t* leaf;
    float* t_hit;
    int8_t* face;
    const float* leaf_data;      // (num_leaves, channels), the first three channels are used
    int channels;
    int shading;                 // FFN_OCTREE_SHADING_*
    float bg_r, bg_g, bg_b;
    float min_transmittance;     // kVolume: the walk ends once T <= this
    float* color;
    float* alpha;
    float* depth;
};

enum WalkMode { kPath = 0, kSpan = 1, kFirstHit = 2, kVolume = 3, kGrad = 4, kVolumeSH1 = 5,
                kVolumeSH2 = 6, kGradSH1 = 7, kGradSH2 = 8, kLeafWeight = 9, kVisible = 10,
                kVisibleMoments = 11, kGradDist = 12, kGradSH1Dist = 13, kGradSH2Dist = 14,
                kDistortion = 15 };

// K29: what one taken leaf adds to a ray's distortion D and to the running W = sum w, M = sum w m
// (both exclusive on entry).  ONE piece of code for K29a and for phase 0 of K29b, so that the two
// form D with the same f32 operations in the same order.
__device__ __forceinline__ void dist_step(float w, float m, float length, float& run_w, float& run_m,
                                          float& dist) {
    dist = dist + ((2.0f * w) * (m * run_w - run_m) + (w * w) * (length * (1.0f / 3.0f)));
    run_w = run_w + w;
    run_m = run_m + w * m;
}

// kPath:     Path rows (t_stops, leaves), max_length entries per ray.
// kSpan:     per ray t_in / t_out / hit over the leaves that end after t_min.
// kFirstHit: the first of those leaves, where the loop ends (K14).
// kVolume:   colour, opacity and depth composited front to back over those leaves (K15).
// kVolumeSH1 / kVolumeSH2: kVolume with the leaf colour of K18a, degree 1 / 2; first.leaf_data is the
//            padded device layout and first.channels its row stride.
// kGrad:     K17a.  The idle parameters carry its buffers: max_length the phase (0 count, 1 emit),
//            span_hit the int32 ray counts (phase 0, written) / offsets (phase 1, n + 1 read),
//            first.color / first.alpha the per-ray C and T_{n+1} (written in phase 0, read in
//            phase 1), span_in / span_out the upstream d_color / d_alpha, t_stops the entries'
//            float4 values and leaves their int32 leaf numbers.
// kGradSH1 / kGradSH2: K19a, kGrad with the leaf colour of K18a.  As kGrad, and first.leaf carries
//            the entries' int32 ray numbers; first.leaf_data / first.channels as kVolumeSH*.
// kLeafWeight: K21a.  span_hit the (num_leaves) uint32 weights (f32 bit patterns, raised, never
//            lowered), first.leaf_data / first.channels rows and their stride, first.shading the
//            density's offset in a row.  Nothing is written per ray.
// kVisible:  K24.  n the leaves, blockIdx.y the camera; starts the (num_leaves,3) leaf centres,
//            directions the per-camera blocks of 16 floats (P' row-major, the eye, one of padding),
//            t_stops the camera-major uint32 RGBA pixels, leaves the (num_leaves) pairs of 64-bit
//            vote words, max_length alpha_u8, first.bg_r / first.bg_g the image's width / height as
//            floats (exact: at most 2^24), first.leaf_data / channels / shading as kLeafWeight.
// kVisibleMoments: K28a.  kVisible, and leaves the (num_leaves) rows of FOUR 64-bit words.
// kGradDist / kGradSH1Dist / kGradSH2Dist: K29b.  kGrad / kGradSH1 / kGradSH2, and pad carries
//            dist_scale, first.depth the per-ray (W_tot, M_tot, D) triples (n,3; written in phase 0,
//            read in phase 1), first.t_hit the caller's (n) ray_distortion (phase 0, may be null).
// kDistortion: K29a.  first.leaf_data / channels / shading as kLeafWeight, first.depth the (n) D.
template <int kMode>
__global__ void __launch_bounds__(kWalkThreads)
octree_walk_kernel(const float* __restrict__ starts, const float* __restrict__ directions,
                   int64_t n, float scale, int depth, const int64_t* __restrict__ node_index,
                   int64_t num_nodes, const int64_t* __restrict__ leaf_index, int64_t num_leaves,
                   int max_length, float* __restrict__ t_stops, int64_t* __restrict__ leaves,
                   float t_min, float pad, float* __restrict__ span_in,
                   float* __restrict__ span_out, uint8_t* __restrict__ span_hit, FirstHit first) {
    constexpr bool kSpans = kMode == kSpan;
    constexpr bool kSees = kMode == kVisible || kMode == kVisibleMoments;      // K24, K28a
    constexpr bool kSH = kMode == kVolumeSH1 || kMode == kVolumeSH2;
    constexpr bool kSHGrad = kMode == kGradSH1 || kMode == kGradSH2 || kMode == kGradSH1Dist ||
                             kMode == kGradSH2Dist;
    constexpr bool kPlainGrad = kMode == kGrad || kMode == kGradDist;
    constexpr bool kDist = kMode == kGradDist || kMode == kGradSH1Dist || kMode == kGradSH2Dist;  // K29b
    constexpr int kBasis = kMode == kVolumeSH2 || kMode == kGradSH2 || kMode == kGradSH2Dist ? 9 : 4;
    const int64_t r = (int64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (r >= n) return;
    const float sx = starts[r * 3 + 0], sy = starts[r * 3 + 1], sz = starts[r * 3 + 2];
    // K24: the pair's pixel, and the cheap rejects before the first tree lookup
    const float* camera = directions + (kSees ? 16 * (int64_t)blockIdx.y : 0);
    uint32_t rgba = 0;
    if (kSees) {
        const float w = ((camera[8] * sx + camera[9] * sy) + camera[10] * sz) + camera[11];
        if (!(w > 0.0f)) return;                         // behind the camera (NaN too)
        const float x = ((camera[0] * sx + camera[1] * sy) + camera[2] * sz) + camera[3];
        const float y = ((camera[4] * sx + camera[5] * sy) + camera[6] * sz) + camera[7];
        const float fu = x / w + 0.5f, fv = y / w + 0.5f;
        if (!(fu >= 0.0f && fu < first.bg_r && fv >= 0.0f && fv < first.bg_g)) return;
        // 0 <= col < width and 0 <= row < height: inside image blockIdx.y
        const int64_t pixel = ((int64_t)blockIdx.y * (int)first.bg_g + (int)fv) * (int)first.bg_r +
                              (int)fu;
        rgba = reinterpret_cast<const uint32_t*>(t_stops)[pixel];   // bytes r, g, b, a from the lowest up
        if ((rgba >> 24) < (uint32_t)max_length) return;            // background
    }
    // K24: from the eye to the leaf's centre, which lies at t = 1
    const float ox = kSees ? camera[12] : sx, oy = kSees ? camera[13] : sy,
                oz = kSees ? camera[14] : sz;
    const float dx = kSees ? sx - ox : directions[r * 3 + 0],
                dy = kSees ? sy - oy : directions[r * 3 + 1],
                dz = kSees ? sz - oz : directions[r * 3 + 2];
    const int levels = depth - 1;
    const int cells = 1 << levels;

    float root_in = -__builtin_inff(), root_out = __builtin_inff();
    int axis_in = 0;
    bool miss = false;
    root_slab(ox, dx, scale, 0, root_in, root_out, axis_in, miss);
    root_slab(oy, dy, scale, 1, root_in, root_out, axis_in, miss);
    root_slab(oz, dz, scale, 2, root_in, root_out, axis_in, miss);
    // a chord of positive, finite length (three zero components: a point, not a ray)
    const bool hit = !miss && root_in < root_out && fabsf(root_in) < __builtin_inff() &&
                     fabsf(root_out) < __builtin_inff();

    // the cell the ray enters the cube in: on the entry axis the face's own layer
    int ix = axis_in == 0 ? (dx > 0.0f ? 0 : cells - 1) : chain_bits(ox + root_in * dx, 0.0f, scale, levels);
    int iy = axis_in == 1 ? (dy > 0.0f ? 0 : cells - 1) : chain_bits(oy + root_in * dy, 0.0f, scale, levels);
    int iz = axis_in == 2 ? (dz > 0.0f ? 0 : cells - 1) : chain_bits(oz + root_in * dz, 0.0f, scale, levels);

    // A walk writes at most max_length - 1 stops (the reference's stop == max_length - 1 rule,
    // octree.py:460); a span walk has no such cap, but every step moves one cell coordinate
    // forward for good, so a chord has at most 3 * cells + 1 regions.
    const int max_stops = kMode == kPath ? max_length - 1 : 3 * cells + 1;
    // Every region costs at most `depth` trips: depth - 1 descents and the region itself.  The
    // loop condition holds the trip count to max_stops * depth for ANY input (NaNs, a tree
    // whose two indices contradict each other): nothing below can extend it.
    const int max_trips = max_stops * depth;

    int64_t id = 0;
    int level = 0, known = 0, stop = 0;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, half = scale, t = root_in;
    bool inside = hit, any_leaf = false;
    float first_in = 0.0f, last_out = 0.0f;
    // first hit: the axis of the plane the ray crossed into the current region, and the answer
    int axis_prev = axis_in, hit_face = -1;
    int64_t hit_leaf = -1;
    // volume: world length per unit of t, transmittance, colour, and the heaviest leaf's entry
    const float norm = kMode == kVolume || kPlainGrad || kSH || kSHGrad ||
                               kMode == kLeafWeight || kSees || kMode == kDistortion
                           ? sqrtf(dx * dx + dy * dy + dz * dz) : 0.0f;
    float trans = 1.0f, acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, w_best = 0.0f, t_best = 0.0f;
    // gradient walk: the ray's entries [base, base + mine), its C, T_{n+1} and upstream gradients
    const bool emit = (kPlainGrad || kSHGrad) && max_length != 0;
    int32_t* ray_slots = reinterpret_cast<int32_t*>(span_hit);
    float4* entry_values = reinterpret_cast<float4*>(t_stops);
    int32_t* entry_leaves = reinterpret_cast<int32_t*>(leaves);
    int32_t* entry_rays = reinterpret_cast<int32_t*>(first.leaf);        // K19a
    unsigned* leaf_weights = reinterpret_cast<unsigned*>(span_hit);      // K21a
    bool visible = false;                                                // K24
    int taken = 0, base = 0, mine = 0;
    float c_r = 0.0f, c_g = 0.0f, c_b = 0.0f, t_end = 0.0f, g_r = 0.0f, g_g = 0.0f, g_b = 0.0f,
          g_a = 0.0f;
    // K18a, K19a: the basis at the ray's unit direction (sh_terms.h)
    float basis[kBasis];
    if (kSH || kSHGrad) sh_ray_basis<kBasis == 9 ? 2 : 1>(dx, dy, dz, norm, basis);
    if (emit) {
        base = ray_slots[r];
        mine = ray_slots[r + 1] - base;
        // a ray without entries has nothing to walk for
        if (mine <= 0) return;
        c_r = first.color[r * 3 + 0]; c_g = first.color[r * 3 + 1]; c_b = first.color[r * 3 + 2];
        t_end = first.alpha[r];
        g_r = span_in[r * 3 + 0]; g_g = span_in[r * 3 + 1]; g_b = span_in[r * 3 + 2];
        g_a = span_out[r];
    }
    // K29: the running W, M (exclusive) and D; phase 1 of K29b: W_tot, M_tot, 2 D and the running
    // sum of w_j G_j (inclusive)
    float run_w = 0.0f, run_m = 0.0f, dist = 0.0f, w_tot = 0.0f, m_tot = 0.0f, dist2 = 0.0f,
          run_wg = 0.0f;
    if (kDist && emit) {
        w_tot = first.depth[r * 3 + 0]; m_tot = first.depth[r * 3 + 1];
        dist2 = 2.0f * first.depth[r * 3 + 2];
    }
    for (int trip = 0; trip < max_trips && stop < max_stops && inside; ++trip) {
        int64_t at;
        const bool interior = level < known ||
                              (level < levels && find_id(node_index, num_nodes, id, &at));
        if (interior) {
            const int shift = levels - 1 - level;
            const int bx = (ix >> shift) & 1, by = (iy >> shift) & 1, bz = (iz >> shift) & 1;
            half *= 0.5f;
            cx = bx ? cx + half : cx - half;
            cy = by ? cy + half : cy - half;
            cz = bz ? cz + half : cz - half;
            id = 8 * id + 1 + (4 * bx + 2 * by + bz);
            ++level;
            continue;
        }
        // a region: a leaf or an empty cell
        const int64_t leaf = find_id(leaf_index, num_leaves, id, &at) ? at : -1;
        const float tx = exit_t(ox, dx, cx, half), ty = exit_t(oy, dy, cy, half),
                    tz = exit_t(oz, dz, cz, half);
        int axis_out = 0;
        float t_exit = tx;
        if (ty < t_exit) { t_exit = ty; axis_out = 1; }
        if (tz < t_exit) { t_exit = tz; axis_out = 2; }
        if (kMode == kFirstHit) {
            if (leaf >= 0 && t_exit > t_min) {
                const float d_in = axis_prev == 0 ? dx : axis_prev == 1 ? dy : dz;
                hit_leaf = leaf;
                first_in = t > t_min ? t : t_min;
                hit_face = t < t_min ? 6 : 2 * axis_prev + (d_in > 0.0f ? 0 : 1);
                break;
            }
            axis_prev = axis_out;
        } else if (kMode == kVolume) {
            if (leaf >= 0 && t_exit > t_min) {
                float lr, lg, lb, ls;
                if (first.channels == 4) {
                    const float4 v = reinterpret_cast<const float4*>(first.leaf_data)[leaf];
                    lr = v.x; lg = v.y; lb = v.z; ls = v.w;
                } else {
                    const float* data = first.leaf_data + leaf * first.channels;
                    lr = data[0]; lg = data[1]; lb = data[2]; ls = data[3];
                }
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                const float w = trans * a;
                acc_r += w * lr; acc_g += w * lg; acc_b += w * lb;
                if (w > w_best) { w_best = w; t_best = t0; }
                trans = trans * (1.0f - a);
                if (trans <= first.min_transmittance) break;
            }
        } else if (kSH) {
            if (leaf >= 0 && t_exit > t_min) {
                constexpr int kQuads = (3 * kBasis + 1 + 3) / 4;
                const float4* row4 = reinterpret_cast<const float4*>(first.leaf_data +
                                                                     leaf * first.channels);
                float row[4 * kQuads];
#pragma unroll
                for (int q = 0; q < kQuads; ++q) {
                    const float4 v = row4[q];
                    row[4 * q + 0] = v.x; row[4 * q + 1] = v.y; row[4 * q + 2] = v.z;
                    row[4 * q + 3] = v.w;
                }
                const float ls = row[0];
                float rgb[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float z = row[1 + c * kBasis] * basis[0];
#pragma unroll
                    for (int b = 1; b < kBasis; ++b)
                        z = __builtin_fmaf(row[1 + c * kBasis + b], basis[b], z);
                    rgb[c] = sigmoid_f(z);
                }
                const float lr = rgb[0], lg = rgb[1], lb = rgb[2];
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                const float w = trans * a;
                acc_r += w * lr; acc_g += w * lg; acc_b += w * lb;
                if (w > w_best) { w_best = w; t_best = t0; }
                trans = trans * (1.0f - a);
                if (trans <= first.min_transmittance) break;
            }
        } else if (kPlainGrad) {
            if (leaf >= 0 && t_exit > t_min) {
                float lr, lg, lb, ls;
                if (first.channels == 4) {
                    const float4 v = reinterpret_cast<const float4*>(first.leaf_data)[leaf];
                    lr = v.x; lg = v.y; lb = v.z; ls = v.w;
                } else {
                    const float* data = first.leaf_data + leaf * first.channels;
                    lr = data[0]; lg = data[1]; lb = data[2]; ls = data[3];
                }
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                const float w = trans * a;
                acc_r += w * lr; acc_g += w * lg; acc_b += w * lb;
                trans = trans * (1.0f - a);                    // T_{k+1}
                if (emit && taken < mine) {
                    const float behind = g_r * (trans * lr - (c_r - acc_r)) +
                                         g_g * (trans * lg - (c_g - acc_g)) +
                                         g_b * (trans * lb - (c_b - acc_b));
                    float ds = ls >= 0.0f ? length * (behind + g_a * t_end) : 0.0f;
                    if (kDist) {
                        // G_k, the prefix of w_j G_j, and dD/dsigma_k = L_k [T_{k+1} G_k - sum_{j>k} w_j G_j]
                        const float m = (0.5f * (t0 + t_exit)) * norm;
                        const float next_w = run_w + w, next_m = run_m + w * m;
                        const float g = 2.0f * (((m * run_w - run_m) + (m_tot - next_m)) -
                                                m * (w_tot - next_w)) +
                                        (2.0f / 3.0f) * (w * length);
                        run_wg = run_wg + w * g;
                        const float dd = length * (trans * g - (dist2 - run_wg));
                        if (ls >= 0.0f) ds = ds + pad * dd;
                        run_w = next_w; run_m = next_m;
                    }
                    entry_values[base + taken] = make_float4(w * g_r, w * g_g, w * g_b, ds);
                    entry_leaves[base + taken] = (int32_t)leaf;
                }
                if (kDist && !emit)
                    dist_step(w, (0.5f * (t0 + t_exit)) * norm, length, run_w, run_m, dist);
                ++taken;
                if (trans <= first.min_transmittance) break;
            }
        } else if (kSHGrad) {
            if (leaf >= 0 && t_exit > t_min) {
                // the row, the dot product and the sigmoid are the kSH branch's, line for line.  They
                // are not shared through a device function: with one (forced inline, with or without
                // __restrict__) kVolumeSH1 / kVolumeSH2 compile to different instructions, and those
                // two must keep the ones they have
                constexpr int kQuads = (3 * kBasis + 1 + 3) / 4;
                const float4* row4 = reinterpret_cast<const float4*>(first.leaf_data +
                                                                     leaf * first.channels);
                float row[4 * kQuads];
#pragma unroll
                for (int q = 0; q < kQuads; ++q) {
                    const float4 v = row4[q];
                    row[4 * q + 0] = v.x; row[4 * q + 1] = v.y; row[4 * q + 2] = v.z;
                    row[4 * q + 3] = v.w;
                }
                const float ls = row[0];
                float rgb[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float z = row[1 + c * kBasis] * basis[0];
#pragma unroll
                    for (int b = 1; b < kBasis; ++b)
                        z = __builtin_fmaf(row[1 + c * kBasis + b], basis[b], z);
                    rgb[c] = sigmoid_f(z);
                }
                const float lr = rgb[0], lg = rgb[1], lb = rgb[2];
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                const float w = trans * a;
                acc_r += w * lr; acc_g += w * lg; acc_b += w * lb;
                trans = trans * (1.0f - a);                    // T_{k+1}
                if (emit && taken < mine) {
                    const float behind = g_r * (trans * lr - (c_r - acc_r)) +
                                         g_g * (trans * lg - (c_g - acc_g)) +
                                         g_b * (trans * lb - (c_b - acc_b));
                    float ds = ls >= 0.0f ? length * (behind + g_a * t_end) : 0.0f;
                    if (kDist) {
                        // G_k, the prefix of w_j G_j, and dD/dsigma_k = L_k [T_{k+1} G_k - sum_{j>k} w_j G_j]
                        const float m = (0.5f * (t0 + t_exit)) * norm;
                        const float next_w = run_w + w, next_m = run_m + w * m;
                        const float g = 2.0f * (((m * run_w - run_m) + (m_tot - next_m)) -
                                                m * (w_tot - next_w)) +
                                        (2.0f / 3.0f) * (w * length);
                        run_wg = run_wg + w * g;
                        const float dd = length * (trans * g - (dist2 - run_wg));
                        if (ls >= 0.0f) ds = ds + pad * dd;
                        run_w = next_w; run_m = next_m;
                    }
                    // e_kc = w g_c (c (1 - c)): the factor of Y_b(u) in d k_cb
                    entry_values[base + taken] = make_float4((w * g_r) * (lr * (1.0f - lr)),
                                                             (w * g_g) * (lg * (1.0f - lg)),
                                                             (w * g_b) * (lb * (1.0f - lb)), ds);
                    entry_leaves[base + taken] = (int32_t)leaf;
                    entry_rays[base + taken] = (int32_t)r;
                }
                if (kDist && !emit)
                    dist_step(w, (0.5f * (t0 + t_exit)) * norm, length, run_w, run_m, dist);
                ++taken;
                if (trans <= first.min_transmittance) break;
            }
        } else if (kMode == kLeafWeight) {
            if (leaf >= 0 && t_exit > t_min) {
                const float ls = first.leaf_data[leaf * first.channels + first.shading];
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                const float w = trans * a;
                if (w > 0.0f) {                                // a NaN w fails too
                    const unsigned bits = __float_as_uint(w);
                    if (leaf_weights[leaf] < bits) atomicMax(leaf_weights + leaf, bits);
                }
                trans = trans * (1.0f - a);
                if (trans <= first.min_transmittance) break;
            }
        } else if (kMode == kDistortion) {
            if (leaf >= 0 && t_exit > t_min) {
                const float ls = first.leaf_data[leaf * first.channels + first.shading];
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                const float w = trans * a;
                dist_step(w, (0.5f * (t0 + t_exit)) * norm, length, run_w, run_m, dist);
                trans = trans * (1.0f - a);
                if (trans <= first.min_transmittance) break;
            }
        } else if (kSees) {
            if (leaf >= 0 && t_exit > t_min) {
                if (leaf == r) {                               // nothing opaque came first
                    visible = true;
                    break;
                }
                const float ls = first.leaf_data[leaf * first.channels + first.shading];
                const float t0 = t > t_min ? t : t_min;
                const float length = (t_exit - t0) * norm;
                const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                const float a = 1.0f - expf(-(sigma * length));
                trans = trans * (1.0f - a);
                if (trans <= first.min_transmittance) break;
            }
        } else if (kSpans) {
            if (leaf >= 0 && t_exit > t_min) {
                if (!any_leaf) first_in = t > t_min ? t : t_min;
                any_leaf = true;
                last_out = t_exit;
            }
        } else {
            t_stops[r * max_length + stop] = t;      // stop < max_length - 1
            leaves[r * max_length + stop] = leaf;
        }
        ++stop;
        // step to the next cell
        const int span = levels - level;
        const int nx = step_axis(ix, axis_out == 0, dx, ox + t_exit * dx, cx, half, span);
        const int ny = step_axis(iy, axis_out == 1, dy, oy + t_exit * dy, cy, half, span);
        const int nz = step_axis(iz, axis_out == 2, dz, oz + t_exit * dz, cz, half, span);
        inside = ((nx | ny | nz) >= 0) && nx < cells && ny < cells && nz < cells;
        // the levels above the deepest common ancestor of the two cells were interior on the
        // way down to this region (the new cell lies outside it)
        const int differ = (ix ^ nx) | (iy ^ ny) | (iz ^ nz);
        known = inside ? min(level, levels - (32 - __clz(differ)) + 1) : 0;
        ix = nx; iy = ny; iz = nz;
        t = t_exit;
        id = 0; level = 0;
        cx = 0.0f; cy = 0.0f; cz = 0.0f; half = scale;
    }
    if (kMode == kFirstHit) {
        const bool found = hit_leaf >= 0;
        if (first.leaf) first.leaf[r] = hit_leaf;
        if (first.t_hit) first.t_hit[r] = first_in;
        if (first.face) first.face[r] = (int8_t)hit_face;
        if (first.color) {
            float cr = first.bg_r, cg = first.bg_g, cb = first.bg_b;
            if (found) {
                const float* data = first.leaf_data + hit_leaf * first.channels;
                cr = data[0]; cg = data[1]; cb = data[2];
                if (first.shading == FFN_OCTREE_SHADING_FACES) {
                    const float k = face_shade(hit_face);
                    cr *= k; cg *= k; cb *= k;
                }
            }
            first.color[r * 3 + 0] = cr;
            first.color[r * 3 + 1] = cg;
            first.color[r * 3 + 2] = cb;
            first.alpha[r] = found ? 1.0f : 0.0f;
            first.depth[r] = first_in;
        }
    } else if (kMode == kVolume || kSH) {
        first.color[r * 3 + 0] = acc_r + trans * first.bg_r;
        first.color[r * 3 + 1] = acc_g + trans * first.bg_g;
        first.color[r * 3 + 2] = acc_b + trans * first.bg_b;
        first.alpha[r] = 1.0f - trans;
        first.depth[r] = t_best;
    } else if (kPlainGrad || kSHGrad) {
        if (!emit) {
            if (kDist) {
                first.depth[r * 3 + 0] = run_w; first.depth[r * 3 + 1] = run_m;
                first.depth[r * 3 + 2] = dist;
                if (first.t_hit) first.t_hit[r] = dist;
            }
            ray_slots[r] = taken;
            first.color[r * 3 + 0] = acc_r + trans * first.bg_r;
            first.color[r * 3 + 1] = acc_g + trans * first.bg_g;
            first.color[r * 3 + 2] = acc_b + trans * first.bg_b;
            first.alpha[r] = trans;
        }
    } else if (kMode == kLeafWeight) {
        // nothing per ray
    } else if (kMode == kDistortion) {
        first.depth[r] = dist;                               // +0 for a ray that takes no leaf
    } else if (kSees) {
        if (visible) {
            // [sum_r, sum_g] and [sum_b, count] as two 64-bit words, the first field in the low half:
            // a sum stays below 2^24 and the count below 2^17, so no carry crosses a field
            // K28a: a leaf's row is four words, K24's two and then [sq_r, sq_g] and [sq_b, 0]; a square
            // is at most 65025 and 65025 C < 2^32 for at most kMomentsMaxCameras cameras per buffer
            constexpr int kWords = kMode == kVisibleMoments ? 4 : 2;
            unsigned long long* votes = reinterpret_cast<unsigned long long*>(leaves) + kWords * r;
            atomicAdd(votes, (unsigned long long)(rgba & 255u) |
                                 ((unsigned long long)((rgba >> 8) & 255u) << 32));
            atomicAdd(votes + 1, (unsigned long long)((rgba >> 16) & 255u) | (1ull << 32));
            if (kMode == kVisibleMoments) {
                const uint32_t cr = rgba & 255u, cg = (rgba >> 8) & 255u, cb = (rgba >> 16) & 255u;
                atomicAdd(votes + 2, (unsigned long long)(cr * cr) |
                                         ((unsigned long long)(cg * cg) << 32));
                atomicAdd(votes + 3, (unsigned long long)(cb * cb));
            }
        }
    } else if (kSpans) {
        // pad finest-cell sides along the ray, in t
        const float side = 2.0f * scale / (float)cells;
        const float widen = pad * side / sqrtf(dx * dx + dy * dy + dz * dz);
        span_hit[r] = any_leaf ? 1 : 0;
        span_in[r] = any_leaf ? first_in - widen : 0.0f;
        span_out[r] = any_leaf ? last_out + widen : 0.0f;
    } else {
        // unwritten entries: the cube's exit t and -1 (octree.py:429-430); a miss has no stop
        const float fill = hit ? root_out : 0.0f;
        for (int k = stop; k < max_length; ++k) {
            t_stops[r * max_length + k] = fill;
            leaves[r * max_length + k] = -1;
        }
    }
}

int check_walk_args(const char* who, const Walk& walk) {
    if (walk.n < 1 || walk.n >= kWalkMaxRays || walk.depth < 1 || walk.depth > kWalkMaxDepth ||
        walk.num_leaves < 1 || walk.num_nodes < 0)
        return fail_who(who, "shape (1 <= n < 2^31, 1 <= depth <= 11, num_leaves >= 1)");
    if (!walk.starts || !walk.directions || !walk.leaf_index ||
        (walk.num_nodes > 0 && !walk.node_index))
        return fail_who(who, "null argument");
    return 0;
}

int check_volume_args(const char* who, const Walk& walk, const VolumeLeaves& leaves,
                      bool any_null) {
    if (walk.t_min != walk.t_min) return fail_who(who, "t_min is NaN");
    if (!(leaves.min_transmittance >= 0.0f && leaves.min_transmittance < 1.0f))
        return fail_who(who, "0 <= min_transmittance < 1");
    if (!leaves.data || any_null) return fail_who(who, "null argument");
    return check_walk_args(who, walk);
}

// one launch of mode kMode; what the mode leaves idle stays at its default
template <int kMode>
static int launch_walk(const char* who, const Walk& walk, const FirstHit& first = FirstHit{},
                       int max_length = 0, float* t_stops = nullptr, int64_t* leaves = nullptr,
                       float pad = 0.0f, float* span_in = nullptr, float* span_out = nullptr,
                       uint8_t* span_hit = nullptr) {
    const unsigned blocks = (unsigned)((walk.n + kWalkThreads - 1) / kWalkThreads);
    hipLaunchKernelGGL(octree_walk_kernel<kMode>, dim3(blocks), dim3(kWalkThreads), 0, walk.stream,
                       walk.starts, walk.directions, walk.n, walk.scale, walk.depth,
                       walk.node_index, walk.num_nodes, walk.leaf_index, walk.num_leaves,
                       max_length, t_stops, leaves, walk.t_min, pad, span_in, span_out, span_hit,
                       first);
    return check_launch(who);
}

// the SH modes come in pairs: kDegree1 is degree 1's, kDegree1 + 1 degree 2's
template <int kDegree1, typename... Args>
static int launch_walk_sh(int degree, const Args&... args) {
    return degree == 1 ? launch_walk<kDegree1>(args...) : launch_walk<kDegree1 + 1>(args...);
}

// what the volume modes read of `first`: the leaves, the background and the three per-ray outputs
static FirstHit volume_first_hit(const VolumeLeaves& leaves, float* color, float* alpha,
                                 float* depth) {
    FirstHit first{};
    first.leaf_data = leaves.data; first.channels = leaves.stride;
    first.bg_r = leaves.bg_r; first.bg_g = leaves.bg_g; first.bg_b = leaves.bg_b;
    first.min_transmittance = leaves.min_transmittance;
    first.color = color; first.alpha = alpha; first.depth = depth;
    return first;
}

// K17a / K19a: the typed buffers of the gradient walk onto the idle parameters, as the comment above
// the kernel lays them out
int octree_grad_walk(const char* who, const GradWalk& grad, int phase) {
    FirstHit first = volume_first_hit(grad.leaves, grad.ray_color, grad.ray_trans, nullptr);
    first.leaf = (int64_t*)grad.entry_rays;
    float* values = (float*)grad.entry_values;                  // t_stops
    int64_t* entry_leaves = (int64_t*)grad.entry_leaves;        // leaves
    float* d_color = const_cast<float*>(grad.d_color);          // span_in
    float* d_alpha = const_cast<float*>(grad.d_alpha);          // span_out
    uint8_t* slots = (uint8_t*)grad.ray_slots;                  // span_hit; max_length: the phase
    if (grad.dist) {
        // K29b: pad carries dist_scale, first.depth the (W_tot, M_tot, D) triples, first.t_hit the
        // caller's ray_distortion
        first.depth = grad.ray_dist;
        first.t_hit = grad.ray_distortion;
        if (grad.leaves.degree == 0)
            return launch_walk<kGradDist>(who, grad.walk, first, phase, values, entry_leaves,
                                          grad.dist_scale, d_color, d_alpha, slots);
        return launch_walk_sh<kGradSH1Dist>(grad.leaves.degree, who, grad.walk, first, phase, values,
                                            entry_leaves, grad.dist_scale, d_color, d_alpha, slots);
    }
    if (grad.leaves.degree == 0)
        return launch_walk<kGrad>(who, grad.walk, first, phase, values, entry_leaves, 0.0f, d_color,
                                  d_alpha, slots);
    return launch_walk_sh<kGradSH1>(grad.leaves.degree, who, grad.walk, first, phase, values,
                                    entry_leaves, 0.0f, d_color, d_alpha, slots);
}

// K26: what ffn_octree_focus_sample passes, one struct by value
struct FocusWalk {
    const float* starts;
    const float* directions;
    const float* near_far;
    int64_t num_rays_total;
    const int64_t* ray_index;
    int num_rays;
    float center_x, center_y, center_z, scale;
    int depth;
    const int64_t* node_index;
    int64_t num_nodes;
    const int64_t* leaf_index;
    int64_t num_leaves;
    const float* leaf_rows;
    int stride, sigma_offset;
    const float* u;
    int n_focus;
    const float* t_uniform;
    int uniform_stride, n_uniform;
    float min_mass;
    float* t_out;
    float* mass_out;
};

// K26  The sibling of octree_walk_kernel: K13's stepping (the device functions above, the same loop
// bounds) walked twice by one lane per ray.  Both walks are ONE piece of code run for phase = 0 and
// phase = 1, so phase 1 repeats phase 0's c bit for bit by construction.
__global__ void __launch_bounds__(kWalkThreads) octree_focus_kernel(const FocusWalk f) {
    const int r = (int)blockIdx.x * kWalkThreads + (int)threadIdx.x;
    if (r >= f.num_rays) return;
    const int64_t i = f.ray_index[r];
    if (i < 0 || i >= f.num_rays_total) return;          // a foreign id: its row is left alone
    const float ox = f.starts[i * 3 + 0] - f.center_x, oy = f.starts[i * 3 + 1] - f.center_y,
                oz = f.starts[i * 3 + 2] - f.center_z;
    const float dx = f.directions[i * 3 + 0], dy = f.directions[i * 3 + 1],
                dz = f.directions[i * 3 + 2];
    const float near = f.near_far[i], far = f.near_far[f.num_rays_total + i];
    const float scale = f.scale;
    const int depth = f.depth, levels = depth - 1, cells = 1 << levels;
    const int n_focus = f.n_focus, n_uniform = f.n_uniform;

    float root_in = -__builtin_inff(), root_out = __builtin_inff();
    int axis_in = 0;
    bool miss = false;
    root_slab(ox, dx, scale, 0, root_in, root_out, axis_in, miss);
    root_slab(oy, dy, scale, 1, root_in, root_out, axis_in, miss);
    root_slab(oz, dz, scale, 2, root_in, root_out, axis_in, miss);
    const bool hit = !miss && root_in < root_out && fabsf(root_in) < __builtin_inff() &&
                     fabsf(root_out) < __builtin_inff();
    const bool ordered = near < far;                     // false for a NaN end too
    const int ix0 = axis_in == 0 ? (dx > 0.0f ? 0 : cells - 1) : chain_bits(ox + root_in * dx, 0.0f, scale, levels);
    const int iy0 = axis_in == 1 ? (dy > 0.0f ? 0 : cells - 1) : chain_bits(oy + root_in * dy, 0.0f, scale, levels);
    const int iz0 = axis_in == 2 ? (dz > 0.0f ? 0 : cells - 1) : chain_bits(oz + root_in * dz, 0.0f, scale, levels);
    const int max_stops = 3 * cells + 1;
    const int max_trips = max_stops * depth;
    const float norm = sqrtf(dx * dx + dy * dy + dz * dz);

    // the merge: k entries of the row are written, ku of the uniform samples among them; `un` is the
    // uniform sample that goes next.  put() is called at most n_focus times (every caller holds
    // j < n_focus) and moves every uniform sample at most once, so k stays below n_uniform + n_focus
    float* out = f.t_out + (int64_t)r * (n_uniform + n_focus);
    const float* uniform = n_uniform > 0 ? f.t_uniform + (int64_t)r * f.uniform_stride : nullptr;
    const float* targets = f.u + (int64_t)r * n_focus;
    int k = 0, ku = 0, j = 0;
    float un = n_uniform > 0 ? uniform[0] : 0.0f;
    auto put = [&](float v) {
        while (ku < n_uniform && un <= v) {
            out[k++] = un;
            ++ku;
            un = ku < n_uniform ? uniform[ku] : 0.0f;
        }
        out[k++] = v;
    };

    float mass = 0.0f, t_last = near, last = -__builtin_inff();
    bool use_tree = false;
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1) {
            use_tree = mass > 0.0f && mass >= f.min_mass;        // a NaN mass fails
            if (!use_tree) break;
        }
        int64_t id = 0;
        int level = 0, known = 0, stop = 0, ix = ix0, iy = iy0, iz = iz0;
        float cx = 0.0f, cy = 0.0f, cz = 0.0f, half = scale, t = root_in;
        bool inside = hit && ordered;
        float trans = 1.0f, c = 0.0f;
        float y = phase == 1 ? targets[0] * mass : 0.0f;
        for (int trip = 0; trip < max_trips && stop < max_stops && inside; ++trip) {
            int64_t at;
            const bool interior = level < known ||
                                  (level < levels && find_id(f.node_index, f.num_nodes, id, &at));
            if (interior) {
                const int shift = levels - 1 - level;
                const int bx = (ix >> shift) & 1, by = (iy >> shift) & 1, bz = (iz >> shift) & 1;
                half *= 0.5f;
                cx = bx ? cx + half : cx - half;
                cy = by ? cy + half : cy - half;
                cz = bz ? cz + half : cz - half;
                id = 8 * id + 1 + (4 * bx + 2 * by + bz);
                ++level;
                continue;
            }
            const int64_t leaf = find_id(f.leaf_index, f.num_leaves, id, &at) ? at : -1;
            const float tx = exit_t(ox, dx, cx, half), ty = exit_t(oy, dy, cy, half),
                        tz = exit_t(oz, dz, cz, half);
            int axis_out = 0;
            float t_exit = tx;
            if (ty < t_exit) { t_exit = ty; axis_out = 1; }
            if (tz < t_exit) { t_exit = tz; axis_out = 2; }
            if (leaf >= 0) {
                const float t0 = fmaxf(t, near), t1 = fminf(t_exit, far);
                if (t1 > t0) {
                    const float ls = f.leaf_rows[leaf * f.stride + f.sigma_offset];
                    const float length = (t1 - t0) * norm;
                    const float sigma = fmaxf(ls, 0.0f);           // NaN -> 0
                    const float a = 1.0f - expf(-(sigma * length));
                    const float w = trans * a;
                    const float c_next = c + w;
                    if (w > 0.0f) {                                // a NaN w fails too
                        t_last = t1;
                        if (phase == 1) {
                            while (j < n_focus && y < c_next) {
                                const float fr = (y - c) / w;
                                float v = fminf(fmaxf(t0 + fr * (t1 - t0), t0), t1);
                                v = fmaxf(v, last);
                                put(v);
                                last = v;
                                ++j;
                                y = j < n_focus ? targets[j] * mass : 0.0f;
                            }
                        }
                    }
                    c = c_next;
                    trans = trans * (1.0f - a);
                    // every later w is exactly 0; phase 1 has nothing left to place
                    if (trans == 0.0f || (phase == 1 && j >= n_focus)) break;
                }
            }
            if (!(t_exit < far)) break;          // the next region would begin at or beyond far
            ++stop;
            const int span = levels - level;
            const int nx = step_axis(ix, axis_out == 0, dx, ox + t_exit * dx, cx, half, span);
            const int ny = step_axis(iy, axis_out == 1, dy, oy + t_exit * dy, cy, half, span);
            const int nz = step_axis(iz, axis_out == 2, dz, oz + t_exit * dz, cz, half, span);
            inside = ((nx | ny | nz) >= 0) && nx < cells && ny < cells && nz < cells;
            const int differ = (ix ^ nx) | (iy ^ ny) | (iz ^ nz);
            known = inside ? min(level, levels - (32 - __clz(differ)) + 1) : 0;
            ix = nx; iy = ny; iz = nz;
            t = t_exit;
            id = 0; level = 0;
            cx = 0.0f; cy = 0.0f; cz = 0.0f; half = scale;
        }
        if (phase == 0) mass = c;
    }
    if (f.mass_out) f.mass_out[r] = mass;
    if (use_tree) {
        // u == 1, a target that rounding, a NaN or a broken order left behind: the end of the mass
        const float v = fmaxf(t_last, last);
        for (; j < n_focus; ++j) put(v);
    } else {
        const float span = far - near;
        for (; j < n_focus; ++j) put(ordered ? near + targets[j] * span : near);
    }
    for (; ku < n_uniform; ++ku) {
        out[k++] = un;
        un = ku + 1 < n_uniform ? uniform[ku + 1] : 0.0f;
    }
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_octree_focus_sample(const float* starts, const float* directions,
                                       const float* near_far, int64_t num_rays_total,
                                       const int64_t* ray_index, int num_rays, float center_x,
                                       float center_y, float center_z, float scale, int depth,
                                       const int64_t* node_index, int64_t num_nodes,
                                       const int64_t* leaf_index, int64_t num_leaves,
                                       const float* leaf_rows, int stride, int sigma_offset,
                                       const float* u, int n_focus, const float* t_uniform,
                                       int uniform_stride, int n_uniform, float min_mass,
                                       float* t_out, float* mass_out, void* stream) {
    const char* who = "ffn_octree_focus_sample";
    if (num_rays == 0) return 0;
    if (num_rays < 0 || num_rays_total < 1) return fail_who(who, "num_rays >= 0, num_rays_total >= 1");
    if (n_focus < 1) return fail_who(who, "n_focus >= 1");
    if (n_uniform < 0) return fail_who(who, "n_uniform >= 0");
    if (n_uniform > 0 && !t_uniform) return fail_who(who, "t_uniform is null with n_uniform > 0");
    if (n_uniform > 0 && uniform_stride < n_uniform)
        return fail_who(who, "uniform_stride >= n_uniform");
    if (depth < 1 || depth > kWalkMaxDepth) return fail_who(who, "depth (1 <= depth <= 11)");
    if (num_leaves < 1 || num_nodes < 0) return fail_who(who, "num_leaves >= 1, num_nodes >= 0");
    if (stride < 1 || sigma_offset < 0 || sigma_offset >= stride)
        return fail_who(who, "stride >= 1, 0 <= sigma_offset < stride");
    if (!(min_mass >= 0.0f)) return fail_who(who, "min_mass >= 0 (and not NaN)");
    if ((int64_t)num_rays * ((int64_t)n_uniform + n_focus) >= kWalkMaxRays)
        return fail_who(who, "num_rays * (n_uniform + n_focus) < 2^31");
    if (!(center_x == center_x && center_y == center_y && center_z == center_z))
        return fail_who(who, "center is NaN");
    if (!starts || !directions || !near_far || !ray_index || !leaf_index ||
        (num_nodes > 0 && !node_index) || !leaf_rows || !u || !t_out)
        return fail_who(who, "null argument");
    if (n_uniform > 0) {
        // the merge reads uniform samples after it has written entries of the same row
        const int64_t total = (int64_t)n_uniform + n_focus;
        const float* out_end = t_out + (int64_t)num_rays * total;
        const float* uni_end = t_uniform + ((int64_t)num_rays - 1) * uniform_stride + n_uniform;
        if (t_uniform < out_end && t_out < uni_end)
            return fail_who(who, "t_out must not alias t_uniform");
    }
    const FocusWalk f{starts, directions, near_far, num_rays_total, ray_index, num_rays, center_x,
                      center_y, center_z, scale, depth, node_index, num_nodes, leaf_index,
                      num_leaves, leaf_rows, stride, sigma_offset, u, n_focus, t_uniform,
                      uniform_stride, n_uniform, min_mass, t_out, mass_out};
    const unsigned blocks = (unsigned)(((int64_t)num_rays + kWalkThreads - 1) / kWalkThreads);
    hipLaunchKernelGGL(octree_focus_kernel, dim3(blocks), dim3(kWalkThreads), 0,
                       (hipStream_t)stream, f);
    return check_launch(who);
}

extern "C" int ffn_octree_walk(const float* starts, const float* directions, int64_t n, float scale,
                               int depth, const int64_t* node_index, int64_t num_nodes,
                               const int64_t* leaf_index, int64_t num_leaves, int max_length,
                               float* t_stops, int64_t* leaves, void* stream) {
    const char* who = "ffn_octree_walk";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, 0.0f, (hipStream_t)stream};
    if (int err = check_walk_args(who, walk)) return err;
    if (max_length < 2 || max_length > (1 << 16))
        return fail_arg("ffn_octree_walk: 2 <= max_length <= 65536");
    if (!t_stops || !leaves) return fail_arg("ffn_octree_walk: null argument");
    return launch_walk<kPath>(who, walk, FirstHit{}, max_length, t_stops, leaves);
}

extern "C" int ffn_octree_spans(const float* starts, const float* directions, int64_t n, float scale,
                                int depth, const int64_t* node_index, int64_t num_nodes,
                                const int64_t* leaf_index, int64_t num_leaves, float t_min,
                                float pad, float* t_in, float* t_out, uint8_t* hit, void* stream) {
    const char* who = "ffn_octree_spans";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    if (int err = check_walk_args(who, walk)) return err;
    if (!t_in || !t_out || !hit) return fail_arg("ffn_octree_spans: null argument");
    if (!(pad >= 0.0f)) return fail_arg("ffn_octree_spans: pad >= 0");
    return launch_walk<kSpan>(who, walk, FirstHit{}, 0, nullptr, nullptr, pad, t_in, t_out, hit);
}

extern "C" int ffn_octree_first_hit(const float* starts, const float* directions, int64_t n,
                                    float scale, int depth, const int64_t* node_index,
                                    int64_t num_nodes, const int64_t* leaf_index,
                                    int64_t num_leaves, float t_min, int64_t* leaf, float* t_hit,
                                    int8_t* face, void* stream) {
    const char* who = "ffn_octree_first_hit";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    // scalars first: which check refuses does not depend on the pointers
    if (t_min != t_min) return fail_arg("ffn_octree_first_hit: t_min is NaN");
    if (int err = check_walk_args(who, walk)) return err;
    if (!leaf || !t_hit || !face) return fail_arg("ffn_octree_first_hit: null argument");
    FirstHit first{};
    first.leaf = leaf; first.t_hit = t_hit; first.face = face;
    return launch_walk<kFirstHit>(who, walk, first);
}

extern "C" int ffn_octree_render(const float* starts, const float* directions, int64_t n,
                                 float scale, int depth, const int64_t* node_index,
                                 int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
                                 float t_min, const float* leaf_data, int channels, float bg_r,
                                 float bg_g, float bg_b, int shading, float* color, float* alpha,
                                 float* depth_out, int64_t* leaf, float* t_hit, int8_t* face,
                                 void* stream) {
    const char* who = "ffn_octree_render";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    if (channels < 3) return fail_arg("ffn_octree_render: channels >= 3");
    if (shading != FFN_OCTREE_SHADING_FLAT && shading != FFN_OCTREE_SHADING_FACES)
        return fail_arg("ffn_octree_render: unknown shading mode");
    if (t_min != t_min) return fail_arg("ffn_octree_render: t_min is NaN");
    if (int err = check_walk_args(who, walk)) return err;
    if (!leaf_data || !color || !alpha || !depth_out)
        return fail_arg("ffn_octree_render: null argument");
    FirstHit first{};
    first.leaf = leaf; first.t_hit = t_hit; first.face = face;
    first.leaf_data = leaf_data; first.channels = channels; first.shading = shading;
    first.bg_r = bg_r; first.bg_g = bg_g; first.bg_b = bg_b;
    first.color = color; first.alpha = alpha; first.depth = depth_out;
    return launch_walk<kFirstHit>(who, walk, first);
}

extern "C" int ffn_octree_render_volume(const float* starts, const float* directions, int64_t n,
                                        float scale, int depth, const int64_t* node_index,
                                        int64_t num_nodes, const int64_t* leaf_index,
                                        int64_t num_leaves, float t_min, const float* leaf_data,
                                        int channels, float bg_r, float bg_g, float bg_b,
                                        float min_transmittance, float* color, float* alpha,
                                        float* depth_out, void* stream) {
    const char* who = "ffn_octree_render_volume";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    const VolumeLeaves rows{leaf_data, channels, 0, bg_r, bg_g, bg_b, min_transmittance};
    if (channels < 4) return fail_arg("ffn_octree_render_volume: channels >= 4");
    if (int err = check_volume_args(who, walk, rows, !color || !alpha || !depth_out)) return err;
    // four channels are read as one 16-byte load per leaf
    if (channels == 4 && misaligned16(leaf_data))
        return fail_arg("ffn_octree_render_volume: leaf_data with 4 channels must be 16-byte aligned");
    return launch_walk<kVolume>(who, walk, volume_first_hit(rows, color, alpha, depth_out));
}

extern "C" int ffn_octree_render_volume_sh(const float* starts, const float* directions, int64_t n,
                                           float scale, int depth, const int64_t* node_index,
                                           int64_t num_nodes, const int64_t* leaf_index,
                                           int64_t num_leaves, float t_min, const float* leaf_data,
                                           int channels, float bg_r, float bg_g, float bg_b,
                                           float min_transmittance, float* color, float* alpha,
                                           float* depth_out, int degree, int row_stride,
                                           void* stream) {
    const char* who = "ffn_octree_render_volume_sh";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    const VolumeLeaves rows{leaf_data, row_stride, degree, bg_r, bg_g, bg_b, min_transmittance};
    if (degree != 1 && degree != 2) return fail_arg("ffn_octree_render_volume_sh: degree is 1 or 2");
    if (channels != 3 * (degree + 1) * (degree + 1) + 1)
        return fail_arg("ffn_octree_render_volume_sh: channels == 3 * (degree + 1)^2 + 1");
    if (row_stride < channels || row_stride % 4 != 0 || row_stride > 64)
        return fail_arg("ffn_octree_render_volume_sh: row_stride is a multiple of 4, channels <= "
                        "row_stride <= 64");
    if (int err = check_volume_args(who, walk, rows, !color || !alpha || !depth_out)) return err;
    // a row is read as 16-byte loads
    if (misaligned16(leaf_data))
        return fail_arg("ffn_octree_render_volume_sh: leaf_data must be 16-byte aligned");
    return launch_walk_sh<kVolumeSH1>(degree, who, walk,
                                      volume_first_hit(rows, color, alpha, depth_out));
}

extern "C" int ffn_octree_leaf_weights(const float* starts, const float* directions, int64_t n,
                                       float scale, int depth, const int64_t* node_index,
                                       int64_t num_nodes, const int64_t* leaf_index,
                                       int64_t num_leaves, float t_min, const float* leaf_data,
                                       int stride, int sigma_offset, float min_transmittance,
                                       uint32_t* weights, void* stream) {
    const char* who = "ffn_octree_leaf_weights";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    const VolumeLeaves rows{leaf_data, stride, 0, 0.0f, 0.0f, 0.0f, min_transmittance};
    if (stride < 1 || sigma_offset < 0 || sigma_offset >= stride)
        return fail_arg("ffn_octree_leaf_weights: stride >= 1, 0 <= sigma_offset < stride");
    if (int err = check_volume_args(who, walk, rows, !weights)) return err;
    FirstHit first = volume_first_hit(rows, nullptr, nullptr, nullptr);
    first.shading = sigma_offset;
    return launch_walk<kLeafWeight>(who, walk, first, 0, nullptr, nullptr, 0.0f, nullptr, nullptr,
                                    (uint8_t*)weights);
}

extern "C" int ffn_octree_distortion(const float* starts, const float* directions, int64_t n,
                                     float scale, int depth, const int64_t* node_index,
                                     int64_t num_nodes, const int64_t* leaf_index,
                                     int64_t num_leaves, float t_min, const float* rows, int stride,
                                     int sigma_offset, float min_transmittance, float* distortion,
                                     void* stream) {
    const char* who = "ffn_octree_distortion";
    const Walk walk{starts, directions, n, scale, depth, node_index, num_nodes, leaf_index,
                    num_leaves, t_min, (hipStream_t)stream};
    const VolumeLeaves leaves{rows, stride, 0, 0.0f, 0.0f, 0.0f, min_transmittance};
    if (stride < 1 || sigma_offset < 0 || sigma_offset >= stride)
        return fail_who(who, "stride >= 1, 0 <= sigma_offset < stride");
    if (int err = check_volume_args(who, walk, leaves, !distortion)) return err;
    FirstHit first = volume_first_hit(leaves, nullptr, nullptr, distortion);
    first.shading = sigma_offset;
    return launch_walk<kDistortion>(who, walk, first);
}

// K24 and K28a: one list of arguments and checks, kMode the write-back; `votes` is (num_leaves,4)
// uint32 for kVisible and (num_leaves,8) for kVisibleMoments
template <int kMode>
static int visible_pairs(const char* who, const float* leaf_centers, int64_t num_leaves, float scale,
                         int depth, const int64_t* node_index, int64_t num_nodes,
                         const int64_t* leaf_index, const float* leaf_data, int stride,
                         int sigma_offset, const uint8_t* images, const float* camera_blocks,
                         int cameras, int height, int width, int alpha_u8, float min_transmittance,
                         uint32_t* votes, void* stream) {
    if (depth < 1 || depth > kWalkMaxDepth) return fail_who(who, "shape (1 <= depth <= 11)");
    if (num_leaves < 1 || num_leaves > kWalkMaxRays || num_nodes < 0)
        return fail_who(who, "shape (1 <= num_leaves <= 2^31, num_nodes >= 0)");
    if (cameras < 1) return fail_who(who, "cameras >= 1");
    if (height < 1 || width < 1 || height > kVisibleMaxSide || width > kVisibleMaxSide)
        return fail_who(who, "images (1 <= height, width <= 2^24)");
    if (alpha_u8 < 1 || alpha_u8 > 255) return fail_who(who, "1 <= alpha_u8 <= 255");
    if (!(min_transmittance >= 0.0f && min_transmittance < 1.0f))        // NaN fails too
        return fail_who(who, "0 <= min_transmittance < 1");
    if (stride < 1 || sigma_offset < 0 || sigma_offset >= stride)
        return fail_who(who, "stride >= 1, 0 <= sigma_offset < stride");
    if (!leaf_centers || !leaf_index || (num_nodes > 0 && !node_index) || !leaf_data || !images ||
        !camera_blocks || !votes)
        return fail_who(who, "null argument");
    if (((uintptr_t)images & 3) != 0 || misaligned16(votes))
        return fail_who(who, kMode == kVisible
                                 ? "images must be 4-byte aligned, votes 16-byte aligned"
                                 : "images must be 4-byte aligned, moments 16-byte aligned");
    // a pixel's index within one launch stays far inside int64
    const int64_t pixels = (int64_t)height * width;
    if (pixels > ((int64_t)1 << 46)) return fail_who(who, "images (height * width <= 2^46)");
    FirstHit first{};
    first.leaf_data = leaf_data; first.channels = stride; first.shading = sigma_offset;
    first.bg_r = (float)width; first.bg_g = (float)height;       // exact: at most 2^24
    first.min_transmittance = min_transmittance;
    const unsigned blocks = (unsigned)((num_leaves + kWalkThreads - 1) / kWalkThreads);
    // blockIdx.y is the camera within a launch: at most kVisibleMaxLaunchCameras of them at a time
    for (int done = 0; done < cameras; done += kVisibleMaxLaunchCameras) {
        const int now = cameras - done < kVisibleMaxLaunchCameras ? cameras - done
                                                                  : kVisibleMaxLaunchCameras;
        hipLaunchKernelGGL(octree_walk_kernel<kMode>, dim3(blocks, (unsigned)now),
                           dim3(kWalkThreads), 0, (hipStream_t)stream, leaf_centers,
                           camera_blocks + 16 * (int64_t)done, num_leaves, scale, depth, node_index,
                           num_nodes, leaf_index, num_leaves, alpha_u8,
                           (float*)const_cast<uint8_t*>(images + 4 * pixels * done), (int64_t*)votes, 0.0f, 0.0f,
                           (float*)nullptr, (float*)nullptr, (uint8_t*)nullptr, first);
        if (int err = check_launch(who)) return err;
    }
    return 0;
}

extern "C" int ffn_octree_visible_votes(const float* leaf_centers, int64_t num_leaves, float scale,
                                        int depth, const int64_t* node_index, int64_t num_nodes,
                                        const int64_t* leaf_index, const float* leaf_data,
                                        int stride, int sigma_offset, const uint8_t* images,
                                        const float* camera_blocks, int cameras, int height,
                                        int width, int alpha_u8, float min_transmittance,
                                        uint32_t* votes, void* stream) {
    return visible_pairs<kVisible>("ffn_octree_visible_votes", leaf_centers, num_leaves, scale,
                                   depth, node_index, num_nodes, leaf_index, leaf_data, stride,
                                   sigma_offset, images, camera_blocks, cameras, height, width,
                                   alpha_u8, min_transmittance, votes, stream);
}

extern "C" int ffn_octree_visible_moments(const float* leaf_centers, int64_t num_leaves,
                                          float scale, int depth, const int64_t* node_index,
                                          int64_t num_nodes, const int64_t* leaf_index,
                                          const float* leaf_data, int stride, int sigma_offset,
                                          const uint8_t* images, const float* camera_blocks,
                                          int cameras, int height, int width, int alpha_u8,
                                          float min_transmittance, uint32_t* moments,
                                          void* stream) {
    return visible_pairs<kVisibleMoments>("ffn_octree_visible_moments", leaf_centers, num_leaves,
                                          scale, depth, node_index, num_nodes, leaf_index,
                                          leaf_data, stride, sigma_offset, images, camera_blocks,
                                          cameras, height, width, alpha_u8, min_transmittance,
                                          moments, stream);
}

extern "C" void ffn_octree_face_shade(float* table) {
    const float k[7] = FFN_OCTREE_FACE_SHADE;
    for (int i = 0; i < 7; ++i) table[i] = k[i];
}
