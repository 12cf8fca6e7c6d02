/*
 * ffn_hip.h -- C ABI of libffn_hip.so: the MI355X (gfx950) kernels behind the
 * fourier_feature_nets volume-rendering hot path.
 *
 * The reference (matajoh/fourier_feature_nets) is pure Python on PyTorch and has no
 * FFI of its own; its "operator interface" for this path is the set of Python methods
 * cited next to each entry point below (paths relative to the reference root).  Each
 * entry point replaces the ATen op sequence those lines launch.
 *
 * Conventions
 *   - every function returns 0 on success or a hipError_t value; the message of the
 *     last failure on the calling thread is available from ffn_last_error_string();
 *     nothing throws across this boundary
 *   - the caller owns every buffer and passes raw DEVICE pointers; all arrays are
 *     contiguous row-major float32 unless the comment says otherwise
 *   - no hidden allocation, no hidden synchronisation; kernels are enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the default stream)
 *   - memory: an entry point writes only through its non-const pointers (or, for
 *     ffn_mlp_pack_jobs and ffn_render_fused_fwd, through the output pointers that its job
 *     table or ffn_render_out names) and only within the extents documented for them; on
 *     success it writes every output word that the comment does not call undefined; it
 *     reads its inputs only within their extents.  tests/test_memory_bounds_gpu.py holds
 *     every entry point that takes a `stream` to this, between red zones
 *   - arguments: the entry points trust the extents they are given.  The Python wrappers refuse a
 *     tensor whose shape does not give a pointer its documented extent before anything is
 *     launched; tests/test_wrapper_refusals_cpu.py holds every wrapper to that
 *   - functions are re-entrant and keep no mutable global state
 *   - one device per call: the device that is current on the calling thread
 */
#ifndef FFN_HIP_H
#define FFN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFN_ABI_VERSION 3

int ffn_abi_version(void);
const char* ffn_last_error_string(void);

/* ------------------------------------------------------------------------------------
 * K1  ray generation + AABB slab test.
 * Replaces CameraInfo.raycast (camera_info.py:99-109) and RaySampler._near_far
 * (ray_sampler.py:202-232) for every pixel of every camera.
 *   unproj      (C,16)  per-camera 4x4 pixel->world matrix (camera_info.py:66-70,
 *                       computed on the host exactly as the reference does)
 *   cam_pos     (C,3)   camera positions (extrinsics[:3,3])
 *   points      (W*H,2) explicit pixel coordinates shared by all cameras, or NULL for the
 *                       integer grid x = id % W, y = id / W (ray_sampler.py:133-136)
 *   box_lo/hi   (3)     HOST pointers: AABB corners (ray_sampler.py:101-104)
 *   starts      (C*W*H,3), directions (C*W*H,3), near_far (2,C*W*H)
 *   valid       (C*W*H) uint8: 1 where near < far (the complement of invalid_rays)
 * Ray id = cam*W*H + y*W + x, integer pixel coordinates, no half-pixel offset.
 */
int ffn_raygen_nearfar(const float* unproj, const float* cam_pos, const float* points,
                       int num_cameras, int width, int height, const float* box_lo,
                       const float* box_hi,
                       float* starts, float* directions, float* near_far, uint8_t* valid,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * K2a  t-sampling: gather + anneal + linspace (+ stratified jitter).
 * Replaces RaySampler.sample up to t_values (ray_sampler.py:364-386) and utils.linspace
 * (utils.py:179-194).  Bit-exact w.r.t. the reference for identical inputs: every
 * multiply and add is rounded separately (no FMA contraction).
 *   near_far    (2,num_rays_total)
 *   ray_index   (R) int64 ray ids
 *   unit        (count) torch.linspace(0,1,count) computed on the host
 *   noise       (R,count) uniform [0,1) block or NULL (not stratified)
 *   anneal      factor already clamped to [anneal_start,1]; pass a negative value when
 *               no annealing applies (step is None or step >= num_anneal_steps)
 *   t_out       (R, t_stride) -- the first `count` entries of each row are written
 */
int ffn_sample_t(const float* near_far, int64_t num_rays_total, const int64_t* ray_index,
                 int num_rays, int count, const float* unit, const float* noise,
                 float anneal, float* t_out, int t_stride, void* stream);

/* K2b  positions = start + t * dir and view_directions = dir repeated
 * (ray_sampler.py:394-397).  positions/views are (R,S,3); views may be NULL. */
int ffn_materialise_samples(const float* starts, const float* directions,
                            const int64_t* ray_index, const float* t_values, int num_rays,
                            int num_samples, float* positions, float* views, void* stream);

/* K2a + K2b in one launch (ray_sampler.py:372-397 for a sampler WITHOUT an opacity model, where
 * nothing merges into t between the two): the arguments of ffn_sample_t with t_stride == count,
 * plus the ray starts / directions; t_out (R,count), positions / views (R,count,3), views may be
 * NULL.  Bit-identical to ffn_sample_t followed by ffn_materialise_samples.  The three outputs
 * must be 16-byte aligned (the kernel stores whole float4 lines of 1024-sample chunks); a pointer
 * that is not is refused with an error, never written through. */
int ffn_sample_materialise(const float* near_far, int64_t num_rays_total, const float* starts,
                           const float* directions, const int64_t* ray_index, int num_rays,
                           int count, const float* unit, const float* noise, float anneal,
                           float* t_out, float* positions, float* views, void* stream);

/* K2c  per-ray CDF from probe opacities (ray_sampler.py:59-67, _determine_cdf).
 *   t_probe (P,n), opacity (P,n) -> cdf (P,n-1) */
int ffn_cdf_build(const float* t_probe, const float* opacity, int64_t num_rays, int n,
                  float* cdf, void* stream);

/* K2c on the coarse model's raw outputs: logits (P,n,4); sigma = softplus(logits[...,3])
 * (ray_sampler.py:261-265) is applied inside.  Used by the live focus sampler, which builds
 * CDF rows per batch instead of a per-sampler table. */
int ffn_cdf_build_logits(const float* t_probe, const float* logits, int64_t num_rays, int n,
                         float* cdf, void* stream);

/* K2d  inverse-transform focus samples + merge with the uniform half + sort
 * (ray_sampler.py:301-357 and :388-392).
 *   cdfs (num_rays_total, n_focus-1) indexed by global ray id
 *   u    (R,n_focus) uniform block (torch.rand, or linspace(0,1,n) repeated)
 *   t_io (R,S): on entry the first S-n_focus entries of each row hold the uniform
 *        samples (from ffn_sample_t with t_stride=S); on exit the row holds all S
 *        samples sorted ascending.  S <= 256. */
int ffn_focus_sample_merge(const float* near_far, int64_t num_rays_total,
                           const float* cdfs, const int64_t* ray_index, const float* u,
                           const float* unit_focus, int num_rays, int num_samples,
                           int n_focus, float* t_io, void* stream);

/* K2d with one CDF row per BATCH ray: cdf_rows (R, n_focus-1), row r belongs to
 * ray_index[r].  Everything else as ffn_focus_sample_merge. */
int ffn_focus_sample_merge_rows(const float* near_far, int64_t num_rays_total,
                                const float* cdf_rows, const int64_t* ray_index, const float* u,
                                const float* unit_focus, int num_rays, int num_samples,
                                int n_focus, float* t_io, void* stream);

/* ------------------------------------------------------------------------------------
 * K3  standalone Fourier feature encoding.
 * Replaces fourier_feature_models.py:59-68 (scale = pi, optional a_values) and
 * nerf_model.py:97-102 (scale = 1, include_input appends x).  Output is (N, 2F[+3]),
 * cos block first.  b is (3,F); a is (F) or NULL.  F == 0 copies x (class MLP).
 * `out` must be 16-byte aligned (rows are assembled in LDS and leave as whole float4 lines).
 * A block assembles at least four rows, at most 64 KiB of them: 2F[+3] <= 4096 columns, i.e.
 * F <= 2048 without and F <= 2046 with include_input.  The workgroup's whole LDS need is those
 * rows plus 1536 B of staged points; it is stated to the runtime and held against the device's
 * per-workgroup limit.
 * Refused by name, before anything is launched or written: n < 0, num_freq < 0; null x or out
 * (n > 0); null b with F > 0; out not 16-byte aligned (F > 0); a row too wide; an LDS need
 * above the device's limit (the message carries both figures).  n == 0 does nothing.
 */
int ffn_fourier_encode(const float* x, int64_t n, const float* b, const float* a,
                       int num_freq, float scale, int include_input, float* out,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * K5  activations + front-to-back alpha compositing, one wavefront per ray.
 * Replaces Raycaster.render after the model call (ray_caster.py:66-93) and
 * utils.calculate_blend_weights (utils.py:72-97).
 *   logits (R,S,4) raw [r,g,b,sigma]; t (R,S)
 *   color (R,3), alpha (R), depth (R) or NULL
 *   nan_flag: int32 on the device, OR-ed with 1 if a NaN is seen in sigmoid(rgb) or
 *             softplus(sigma) (the asserts at ray_caster.py:73-74); may be NULL
 */
int ffn_composite_fwd(const float* logits, const float* t, int num_rays, int num_samples,
                      float* color, float* alpha, float* depth, int32_t* nan_flag,
                      void* stream);

/* K5w  utils.calculate_blend_weights (utils.py:72-97) on its own: t (R,S), sigma (R,S)
 * already activated -> weights (R,S). */
int ffn_blend_weights(const float* t, const float* sigma, int num_rays, int num_samples,
                      float* weights, void* stream);

/* K5w backward: the autograd of utils.py:72-97 in closed form.  d_weights (R,S) ->
 * d_sigma (R,S) and, when d_t is not NULL, d_t (R,S).  S <= 256. */
int ffn_blend_weights_bwd(const float* t, const float* sigma, const float* d_weights,
                          int num_rays, int num_samples, float* d_sigma, float* d_t,
                          void* stream);

/* K5b backward of K5: d(loss)/d(logits) from d/d(color) (R,3) and d/d(alpha) (R). */
int ffn_composite_bwd(const float* logits, const float* t, const float* d_color,
                      const float* d_alpha, int num_rays, int num_samples,
                      float* d_logits, void* stream);

/* ------------------------------------------------------------------------------------
 * K6  ground-truth gather + MSE loss + its gradient.
 * Replaces ImageDataset.render / .loss (image_dataset.py:224-262).
 *   gt_colors (num_rays_total,3), gt_alphas (num_rays_total) or NULL
 *   sums      (2) device floats: sum((c-c_gt)^2), sum((a-a_gt)^2) over this call
 *   d_color = color_scale * 2 (c - c_gt), d_alpha = alpha_scale * 2 (a - a_gt);
 *   the caller picks color_scale = 1/(3R) and alpha_scale = alpha_weight/R (or the
 *   global counts under data parallelism).  d_color/d_alpha may be NULL (loss only).
 *   scratch   (2*ceil(R/256)) floats of workspace
 */
int ffn_mse_loss(const float* color, const float* alpha, const float* gt_colors,
                 const float* gt_alphas, const int64_t* ray_index, int num_rays,
                 float color_scale, float alpha_scale, float* sums, float* d_color,
                 float* d_alpha, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------
 * K7  clip_grad_value_ -> clip_grad_norm_ -> Adam(L2 weight decay) on one flat buffer.
 * Replaces ray_caster.py:327-329 (+ torch.optim.Adam's single-tensor update).
 *   scratch (ceil(n/1024)) floats; step_size = lr/(1-beta1^t), inv_sqrt_bc2 =
 *   1/sqrt(1-beta2^t) are computed by the host in double precision.
 */
int ffn_clip_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                  int64_t n, float clip_value, float max_norm, float step_size,
                  float inv_sqrt_bc2, float beta1, float beta2, float eps,
                  float weight_decay, float* scratch, float* grad_norm_out, void* stream);

/* K5t  The training step's K5 + K6 + K5b in one launch: Raycaster.render (ray_caster.py:66-93),
 * ImageDataset.render / .loss (image_dataset.py:224-262) and their autograd for one batch.
 *   logits (R,S,4), t (R,S); gt_colors / gt_alphas (or NULL) / ray_index / the two scales as in
 *   ffn_mse_loss; d_logits (R,S,4) out -- bit-identical to ffn_composite_fwd -> ffn_mse_loss ->
 *   ffn_composite_bwd; partials: 2 * ffn_composite_train_blocks(R) floats out, one
 *   (sum((c-c_gt)^2), sum((a-a_gt)^2)) pair per workgroup, for ffn_loss_from_partials.
 *   nan_flag as in ffn_composite_fwd (may be NULL).  S <= 512, R >= 1. */
int ffn_composite_train_blocks(int num_rays);
int ffn_composite_train(const float* logits, const float* t, int num_rays, int num_samples,
                        const float* gt_colors, const float* gt_alphas, const int64_t* ray_index,
                        float color_scale, float alpha_scale, float* d_logits, float* partials,
                        int32_t* nan_flag, void* stream);

/* Fixed-order sum of K5t's partials into sums (2 floats; may be NULL) and / or the scalar loss
 *   loss = sums[0] / colour_count + alpha_weight * (sums[1] / alpha_count)
 * into loss_out (may be NULL) (image_dataset.py:237-242). */
int ffn_loss_from_partials(const float* partials, int num_blocks, float colour_count,
                           float alpha_count, float alpha_weight, float* sums, float* loss_out,
                           void* stream);

/* The scalar loss from K6's two sums (possibly all-reduced over the ranks in between):
 *   loss = sums[0] / colour_count + alpha_weight * (sums[1] / alpha_count)
 * (image_dataset.py:237-242: colour_count = 3 * rays, alpha_count = rays); one launch instead
 * of four scalar tensor ops per optimisation step. */
int ffn_loss_value(const float* sums, float colour_count, float alpha_count, float alpha_weight,
                   float* loss_out, void* stream);

/* ------------------------------------------------------------------------------------
 * K8  image assembly (ray_sampler.py:191-196): zeros, scatter, (x*255) truncated to u8.
 *   colors (n,3); pixel_index (n) int64 pixel id inside the frame; image (H*W*3) u8
 * A byte is (uint8)(int)(float32(c) * 255.0f): ONE float32 multiply, truncated; defined for
 * 0 <= c < 256/255.  The whole image is cleared first, also for n == 0; unlisted pixels stay 0.
 * Refused by name, before the clear: width <= 0 or height <= 0, n < 0, n > width * height, a
 * null image, null colors or pixel_index with n > 0.  Pixel ids themselves are not checked.
 */
int ffn_to_image(const float* colors, const int64_t* pixel_index, int64_t n, int width,
                 int height, uint8_t* image, void* stream);

/* ------------------------------------------------------------------------------------
 * K8b  8-bit YCrCb -> RGB, in place on a (pixels,3) u8 frame.  Replaces
 * cv2.cvtColor(pixels, cv2.COLOR_YCrCB2RGB) at ray_sampler.py:197-198 and
 * ray_dataset.py:180-181 (color_space == "YCrCb").  OpenCV's 8-bit fixed-point path
 * (coefficients x 2^14, rounded shift, saturating cast), restated from its documented
 * constants -- cv2 is not available where this library is built: parity unpinned.
 */
int ffn_ycrcb_to_rgb_u8(uint8_t* image, int64_t pixels, void* stream);

/* ------------------------------------------------------------------------------------
 * K4  fused Fourier-feature MLP (sigma + view-dependent RGB), exact-f32 MFMA.
 * Replaces FourierFeatureMLP.forward (fourier_feature_models.py:57-78), NeRF.forward
 * (nerf_model.py:86-124) and their autograd backward.
 *
 * The network is described to the kernels as a short chain of dense steps
 * (ffn_mlp_chain); the same interpreter runs the forward chain and the backward-data
 * chain.  A wavefront owns 32 consecutive samples; activations never leave the CU
 * between layers.  Weights are consumed in an MFMA-operand order produced by
 * ffn_mlp_pack from the natural nn.Linear (out,in) tensors.
 */
#define FFN_MAX_STEPS 16

typedef struct ffn_encoding {
    const float* b;        /* (3,max(F,1)) frequency matrix (device), never NULL      */
    const float* a;        /* (max(F,1)) amplitudes (device), never NULL              */
    int32_t num_freq;      /* F; 0 => features are the raw 3 inputs                  */
    int32_t include_input; /* append x after [cos,sin]                               */
    float scale;           /* pi (FourierFeatureMLP) or 1 (NeRF)                     */
    int32_t width;         /* internal feature count padded to a multiple of 32     */
} ffn_encoding;

/* One dense step.  Its K dimension is [act_groups groups of 8 channels read back from the
 * wave's activation slab (the previous step's output)] followed by [aux_groups generated
 * groups]: Fourier features of encoding enc_id in a forward chain (first layer = features
 * only, hidden layer = activations only, NeRF's skip and view layers = both,
 * nerf_model.py:112-121), or the d_logits columns [lg_col, lg_col+lg_n) in a backward
 * chain (the sigma / rgb heads; 4 groups, only the first is non-zero).  Both counts are
 * multiples of 4.                                                                      */
typedef struct ffn_step {
    int32_t act_groups;
    int32_t aux_groups;
    int32_t enc_id;        /* forward: 0 = position encoding, 1 = view encoding        */
    int32_t lg_col;        /* backward: first d_logits column feeding this step        */
    int32_t lg_n;
    int32_t out_tiles;     /* ceil(out/32): 8, 4, 2 or 1 (wide chains: 16, 8, 4 or 2)  */
    int32_t relu;          /* forward: ReLU on the output                              */
    int32_t dst;           /* forward: 0 = activation slab, 1 = logits [out_col,+out_n)*/
    int32_t out_col;
    int32_t out_n;
    int32_t save_in_slot;  /* slab that receives the act-part INPUT while it is being
                              consumed (forward: H for backward; backward: dZ), or -1.
                              A TRAINING forward chain of <= 256 channels sets it on every
                              step with act_groups > 0 (and save_enc_slot on every step
                              with aux_groups > 0): its K-loop trips save unconditionally */
    int32_t save_out_slot; /* slab that receives the step's output (backward: dZ of the
                              last step; forward: input of a fused head), or -1        */
    int32_t mask_slot;     /* ReLU sign-mask slot: a forward step writes the sign bits of
                              its output there, the backward step that differentiates that
                              layer reads them; -1 = no ReLU                           */
    int32_t save_enc_slot; /* forward: slab that receives the generated encoding features
                              of this step (so the weight gradients read them back instead
                              of regenerating them), or -1                             */
    int32_t head_off;      /* forward: >= 0 fuses a logits head into this step's epilogue:
                              float offset (inside the bias buffer) of 4 bias floats then
                              channels*4 weights [channel][logits column], zero in the
                              columns the head does not write; the step's output is then
                              also stored into slab save_out_slot when training; -1 none */
    int32_t out_slot;      /* split-bf16 kernels only (the f32 kernels ignore it): the slab of the
                              step's output -- its activations in a forward chain, its dZ in a
                              backward chain -- which those kernels save from registers in
                              every step's epilogue; -1 = none                            */
    int64_t w_off;         /* float offset of this step's packed operand weights       */
    int64_t b_off;         /* forward: float offset of the bias (padded to 32*tiles)   */
} ffn_step;

typedef struct ffn_mlp_chain {
    ffn_encoding enc[2];
    ffn_step step[FFN_MAX_STEPS];
    int32_t num_steps;
    int32_t num_slots;                     /* hidden-layer slabs (= sign-mask slots);
                                              entries num_slots.. of the two arrays below
                                              describe the encoding-feature slabs        */
    int32_t bias_floats;                   /* floats in the bias buffer: [fused-head blocks |
                                              per-step padded biases].  The kernels stage its
                                              first 4096 floats in LDS; every head block must lie
                                              inside that copy, a step bias beyond it is read
                                              from global memory                              */
    int32_t wide;                          /* waves per 32-sample block of the exact-f32 chain
                                              kernels.  0: one.  1: TWO waves share a block and a
                                              64 KiB slab (required when some layer is wider than
                                              256 channels: out_tiles may be 16 and must be even,
                                              act_groups <= 64, heads must be fused); the mask
                                              buffer holds 512 uint32 per slot and block.  2: FOUR
                                              waves share a block (one team per workgroup; narrow
                                              chains whose steps have 4 or 8 output tiles, heads
                                              fused; training / backward launches only): 1024
                                              uint32 of masks per slot and block.  The host runs
                                              the short last round of a training launch on the
                                              team kernels (same packs, same slabs)            */
    int32_t slot_channels[FFN_MAX_STEPS];  /* channels of each slab (multiple of 32)  */
    int64_t slot_offset[FFN_MAX_STEPS];    /* sum of channels of the slabs before it  */
} ffn_mlp_chain;

/* Slab ("block") layout, shared by forward, dgrad and wgrad: samples are grouped in blocks
 * of 32; slab `slot` starts at float offset slot_offset[slot]*num_blocks*32 and holds,
 * per block, channels*32 floats as float4s indexed [cq][pos], cq = channel/4,
 * pos = sample_in_block ^ (cq & 15), each float4 = 4 consecutive channels of one sample.
 * The XOR spreads the weight-gradient kernel's transposed reads over distinct sectors. */

/* Gather a natural (rows, cols) matrix into MFMA A-operand order:
 *   dst[((g*tiles + o)*64 + lane)*4 + p] = src[row(32*o + (lane&31)) * ld + col(8*g + 4*(lane>>5) + p)]
 * row_map / col_map (int32, device, may be NULL = identity) translate internal to
 * natural indices; a negative entry or an index outside [0,rows)x[0,cols) yields 0.
 * transpose != 0 swaps the roles (operand rows index src columns).                    */
int ffn_mlp_pack(const float* src, int rows, int cols, int ld, int transpose,
                 const int32_t* row_map, const int32_t* col_map, int groups, int tiles,
                 float* dst, void* stream);

/* The same gather for a whole model in one launch: a device array of jobs, one per operand
 * pack (kind 0: ffn_mlp_pack's formula with row_map = identity) or per bias / fused-head block
 * (kind 1: the strided copy dst[c*dst_cs + r*dst_rs] = src[r*ld + c], r < rows, c < cols).
 * The optimiser step rewrites the weights in place, so a training loop re-packs after every
 * step; this keeps that at one launch. */
typedef struct {
    const float* src;
    float* dst;
    const int32_t* col_map;   /* kind 0: internal K index -> natural column, or NULL */
    int32_t kind, rows, cols, ld, transpose, groups, tiles, dst_rs, dst_cs, reserved;
} ffn_pack_job;
int ffn_mlp_pack_jobs(const ffn_pack_job* jobs, int num_jobs, void* stream);

/* Forward chain.  positions (N,3), views (N,3) or NULL, logits out (N,4).  Training: when
 * `saved` and `masks` are non-NULL, every step writes what the backward pass needs into
 * `saved` (block layout): its input activations (save_in_slot), the encoding features it
 * generated (save_enc_slot), its output when a fused head reads it (save_out_slot); and every
 * ReLU step writes the sign bits of its output into `masks` (num_slots * num_blocks * W
 * uint32, W = 256, or 512 for a wide chain: [slot][block][half][lane][4], bit 31-(16*(tile&1)+r)
 * of word tile/2 = accumulator register r of that lane, tiles counted inside the wave's half;
 * an odd tile count leaves the last word's bits shifted down by 16)
 * for the backward-data chain.  `bias` = bias_floats floats: per step its padded bias, plus
 * the fused heads' blocks (head_off).
 *
 * A launch may cover a SUB-RANGE of a batch's 32-sample blocks (the host splits a batch whose
 * block count leaves a short last round for the persistent grid, and runs that tail on the
 * two-waves-per-block kernels): positions / views / logits / masks are then the sub-range's own
 * arrays (n samples), while the slabs in `saved` are addressed by the batch's block ids --
 * slab_block0 = the launch's first block, slab_blocks = the batch's block count (the slot stride).
 * slab_blocks == 0: the launch is the whole batch. */
int ffn_mlp_forward(const ffn_mlp_chain* chain, const float* packed_w, const float* bias,
                    const float* positions, const float* views, int64_t n, float* logits,
                    float* saved, uint32_t* masks, int64_t slab_block0, int64_t slab_blocks,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * Fused inference render: K2 + K3 + K4 + K5 in one launch.
 * Replaces the body of Raycaster.render_image / batched_render (ray_caster.py:103-159:
 * sampler.sample -> model -> activations -> calculate_blend_weights -> sums, each a pass over
 * HBM-resident (R,S,3)/(R,S,4) arrays) for an eval-mode model: per ray, the t-samples, the
 * positions, the features, every hidden activation and the logits stay on the CU; only the
 * ray id + ray state are read and the composited pixel is written.
 *   rays:      resident sampler state (K1's outputs) + the ids of the rays to render.
 *              t_values == NULL: t_j = near + unit[j] * (far - near) (non-stratified uniform
 *              sampling, ray_sampler.py:380-381, rounded like ffn_sample_t); otherwise the
 *              caller's (R,S) t-values (stratified / opacity-guided samplers).
 *   occupancy: NULL or an occupancy grid (K9): samples in empty cells are not evaluated
 *              (sigma = 0 there: weight 0, transmittance factor 1) -- PSNR-level parity with
 *              the full render, exactly the K9 semantics.
 *   out:       any of color (R,3), alpha (R), depth (R) may be NULL; image != NULL also
 *              writes the u8 pixel (x*255 truncated, ray_sampler.py:193-196) at pixel
 *              ray_id - pixel_offset of an (H*W,3) frame the caller has zeroed.
 * Any forward chain (a wide one runs a pair of wavefronts per ray); num_samples <= 256.
 */
typedef struct ffn_render_rays {
    const float* starts;       /* (num_rays_total,3)                                   */
    const float* directions;   /* (num_rays_total,3), also the view directions          */
    const float* near_far;     /* (2,num_rays_total)                                   */
    int64_t num_rays_total;
    const int64_t* ray_index;  /* (num_rays) int64 ray ids, or NULL: ids ray_base + 0..R-1   */
    int64_t ray_base;
    const uint8_t* valid;      /* NULL, or K1's (num_rays_total) mask: rays with valid == 0
                                  are not traced (zeros in color/alpha/depth, no pixel):
                                  a whole camera renders without a filtered index list  */
    int32_t num_rays;
    int32_t num_samples;
    const float* unit;         /* (num_samples) torch.linspace(0,1,S), or NULL with t_values */
    const float* t_values;     /* (num_rays,num_samples) or NULL                       */
} ffn_render_rays;

typedef struct ffn_occupancy {
    const uint32_t* bits;      /* resolution^3 bits (ffn_occupancy_build)               */
    float box_min[3];
    float box_size[3];
    int32_t resolution;
} ffn_occupancy;

typedef struct ffn_render_out {
    float* color;
    float* alpha;
    float* depth;
    int32_t* nan_flag;         /* as ffn_composite_fwd; may be NULL                    */
    uint8_t* image;
    int64_t pixel_offset;
} ffn_render_out;

int ffn_render_fused_fwd(const ffn_mlp_chain* chain, const float* packed_w, const float* bias,
                         const ffn_render_rays* rays, const ffn_occupancy* occupancy,
                         const ffn_render_out* out, void* stream);

/* Fused live focus sampling: the coarse pass of ray_sampler.py:234-269 (probe the opacity model
 * on n_focus <= 64 points t = linspace(near, far, n_focus) per ray, sigma = softplus of its last
 * output), the CDF of :59-67 and the inverse-transform sampling + merge + sort of :301-357 /
 * :388-392 in ONE launch, per batch ray, with no per-sampler table.  `chain` describes the
 * opacity model (a narrow forward chain; view directions = the ray directions when it takes
 * them).  t_io (R,S): on entry the first S-n_focus entries of each row hold the uniform samples
 * (ffn_sample_t with t_stride = S); on exit all S samples sorted.  u (R,n_focus) as
 * ffn_focus_sample_merge.  Arithmetic identical to ffn_sample_t + ffn_cdf_build_logits +
 * ffn_focus_sample_merge_rows. */
int ffn_focus_fused(const ffn_mlp_chain* chain, const float* packed_w, const float* bias,
                    const float* starts, const float* directions, const float* near_far,
                    int64_t num_rays_total, const int64_t* ray_index, int num_rays,
                    int num_samples, int n_focus, const float* unit_focus, const float* u,
                    float* t_io, void* stream);

/* ------------------------------------------------------------------------------------
 * OPT-IN split-bf16 inference mode of K4 (separately labelled; the exact-f32 entry points above
 * are the parity mode).  Every f32 operand is split into two bf16 parts and every product into
 * three v_mfma_f32_32x32x16_bf16 instructions with f32 accumulation (~2^-16 relative error per
 * product).  The chain is an ffn_mlp_chain whose w_off are offsets (in bf16 elements) into the
 * operand buffer written by ffn_mlp_pack_bf16; bias / fused-head blocks are the f32 buffer of
 * ffn_mlp_forward.  Narrow chains (<= 256 channels), slab-destination steps with fused heads.
 *
 * ffn_mlp_pack_bf16: dst[(((G*tiles + o)*2 + part)*64 + lane)*8 + j] =
 *   part(src[32*o + (lane & 31)][col_map[16*G + 8*(lane >> 5) + j]]), part 0 = bf16(v) rounded to
 *   nearest even, part 1 = bf16(v - part 0); col_map (int32, device, 16*kblocks entries) maps the
 *   operand K order to natural columns (-1 = zero): for activation K blocks the hand-off order
 *   16G + {4h+j | 8+4h+(j-4)}, for encoding K blocks the internal feature order 16G + 8h + j.
 *   transpose = 1 packs src^T (backward data): tile rows walk src's first `cols` columns and
 *   col_map maps K to src's rows. */
int ffn_mlp_pack_bf16(const float* src, int rows, int cols, int ld, const int32_t* col_map,
                      int kblocks, int tiles, int transpose, uint16_t* dst, void* stream);
int ffn_mlp_forward_bf16x3(const ffn_mlp_chain* chain, const uint16_t* packed_w, const float* bias,
                           const float* positions, const float* views, int64_t n, float* logits,
                           void* stream);
/* The same forward pass, leaving what the backward kernels need in the formats of
 * ffn_mlp_forward's training mode (`saved` activation slabs, `masks`): every step saves the
 * encoding features it generates (save_enc_slot), its output (out_slot) and its ReLU sign mask
 * (mask_slot).  OPT-IN ("bf16x3" training precision): the saved values carry the ~1e-6 relative
 * error of the split products. */
int ffn_mlp_forward_bf16x3_train(const ffn_mlp_chain* chain, const uint16_t* packed_w,
                                 const float* bias, const float* positions, const float* views,
                                 int64_t n, float* logits, float* saved, uint32_t* masks,
                                 void* stream);

/* Split-bf16 backward-data chain (OPT-IN "bf16x3" training precision): the chain of
 * ffn_mlp_backward_data with w_off pointing into transposed ffn_mlp_pack_bf16 operands (hidden
 * consumer's K blocks, then -- if the producer feeds a logits head -- two K blocks whose K rows
 * 0..lg_n-1 are the head's rows) and step.out_slot = the slab slot of the step's dZ.
 * Reads the sign masks, writes every dZ slab in the f32 kernels' format. */
int ffn_mlp_backward_data_bf16x3(const ffn_mlp_chain* chain, const uint16_t* packed_wt,
                                 const float* d_logits, int64_t n, const uint32_t* masks,
                                 float* dz, void* stream);

/* ------------------------------------------------------------------------------------
 * OPT-IN f32-ACCURATE split mode of K4 ("bf16x6"; separately labelled, the exact-f32 entry points
 * stay the parity mode and the headline).  Every f32 operand is THREE bf16 parts (hi, mid, lo:
 * 8 + 8 + 8 significand bits = the f32 value exactly) and every f32 product SIX
 * v_mfma_f32_32x32x16_bf16 instructions -- every partial product down to 2^-16 of the leading
 * one (h.l, l.h, m.m, h.m, m.h, h.h, smallest first; the three dropped terms are each below 2^-24
 * of it), f32 accumulation: 12 matrix cycles per K where v_mfma_f32_32x32x2_f32 takes 32, at the
 * error of an f32 dot product (same networks, same tolerances as the exact mode in the tests).
 * Same organisation, chains, slab and mask formats as the bf16x3 entry points (csrc/mlp_bf16_ws.hip:
 * eight waves, one output tile each, two blocks of 32 samples per pass); operands come from
 * ffn_mlp_pack_bf16_parts(parts = 3): dst[(((G*tiles + o)*parts + part)*64 + lane)*8 + j], part p =
 * bf16(v - part 0 - .. - part p-1) (parts = 2 is ffn_mlp_pack_bf16), so every w_off of the bf16x3
 * chain scales by 3/2.  Narrow chains (<= 256 channels per layer) with fused heads; encoding
 * features are the exact-f32 kernels' (polynomial sin / cos, bit for bit).  The weight gradients of
 * this mode are TWO launches over one partial buffer and one reducer table: full units (four
 * 128 x 128 quadrants) and the logits-head units on ffn_mlp_wgrad_units_bf16x6 (three-part operands,
 * below), units with fewer quadrants on the exact-f32 ffn_mlp_wgrad_units, which folds narrow input
 * windows -- both read the slabs these kernels write (host: MlpProgram._plan_wgrad;
 * FFN_BF16X6_WGRAD=f32 keeps every unit on the exact-f32 kernel).
 * FFN_BF16X6_PRODUCTS=9 (environment, measurement only) multiplies out all nine partial products.
 * Two workgroup organisations sit behind these entry points (same packs, same slab / mask / dZ formats;
 * the forward's slabs and masks bit-identical, the backward's dZ within 2e-7 of its largest element: the
 * head term of its step 0 is f32 vector arithmetic in one, six bf16 products in the other): chains whose
 * first step is features-only (16 j K blocks) and whose
 * other steps are 256 -> 256 -- the tiny NeRF / Fourier MLP family -- run the MATRIX WAVES / VECTOR WAVES
 * kernels (csrc/mlp_bf16_mv.hip: four waves that only multiply, eight that only generate features and
 * run epilogues), everything else the two-waves-per-SIMD kernels (csrc/mlp_bf16_ws.hip);
 * FFN_BF16X6_ORG=ws (environment, read per launch) keeps the latter for every chain (A/B).
 * ffn_mlp_bf16x6_organisation answers which one a launch of `chain` takes: 1 = matrix / vector waves,
 * 0 = two waves per SIMD (backward != 0: the backward-data chain).
 * Reference arithmetic being matched: fourier_feature_models.py:57-78, nerf_model.py:86-124. */
int ffn_mlp_bf16x6_organisation(const ffn_mlp_chain* chain, int backward);
int ffn_mlp_pack_bf16_parts(const float* src, int rows, int cols, int ld, const int32_t* col_map,
                            int kblocks, int tiles, int transpose, int parts, uint16_t* dst,
                            void* stream);
int ffn_mlp_forward_bf16x6(const ffn_mlp_chain* chain, const uint16_t* packed_w, const float* bias,
                           const float* positions, const float* views, int64_t n, float* logits,
                           void* stream);
int ffn_mlp_forward_bf16x6_train(const ffn_mlp_chain* chain, const uint16_t* packed_w,
                                 const float* bias, const float* positions, const float* views,
                                 int64_t n, float* logits, float* saved, uint32_t* masks,
                                 void* stream);
int ffn_mlp_backward_data_bf16x6(const ffn_mlp_chain* chain, const uint16_t* packed_wt,
                                 const float* d_logits, int64_t n, const uint32_t* masks,
                                 float* dz, void* stream);

/* Backward-data chain: d_logits (N,4) + ReLU sign masks -> dZ slabs (same slab geometry as
 * `saved`).  packed_wt holds the transposed operand packs. */
int ffn_mlp_backward_data(const ffn_mlp_chain* chain, const float* packed_wt,
                          const float* d_logits, int64_t n, uint32_t* masks, float* dz,
                          int64_t slab_block0, int64_t slab_blocks, void* stream);

/* Weight gradients  dW_l = sum over samples of dZ_l (x) X_l  (autograd of the nn.Linear
 * layers, fourier_feature_models.py:70-78 / nerf_model.py:103-124).  Every operand is a
 * slab: dZ from ffn_mlp_backward_data, X = hidden activations and encoding features saved by
 * ffn_mlp_forward.  A unit is a (<=256 output channels) x (<=256 input channels) block of
 * some dW; segments assign contiguous ranges of 32-sample blocks of a unit to persistent
 * workgroups: workgroup g (256 threads) processes segments seg_start[g] .. seg_start[g+1]
 * (segment.job indexes `units`).  Its four waves own the 128x128 quadrants of the unit that
 * exist (quadrant id = 2*m_half + n_half when both sides are wider than 128 channels,
 * otherwise the half index of the wide side, otherwise 0); when fewer than four exist, wave
 * w takes quadrant w % Q and the (w / Q)-th share of every block's samples.  Each wave
 * writes one partial of ffn_mlp_wgrad_partial_floats() floats into slot segment.slot + w.
 * Segments may be planned for more blocks than ceil(n/32): the kernel clamps blk_end and
 * writes zero partials for segments that lie entirely past the end. */
typedef struct ffn_wgrad_segment {
    int32_t job;
    int32_t slot;
    int64_t blk_begin;
    int64_t blk_end;
} ffn_wgrad_segment;

typedef struct ffn_wgrad_unit {
    int32_t m_slot;    /* dZ slab                        (head unit: first d_logits column) */
    int32_t m_cq0;     /* first channel quad of the output window (head unit: #columns)    */
    int32_t m_quads;   /* valid quads (<= 64, multiple of 8)                           */
    int32_t want_bias; /* != 0: also produce the bias gradient (sum of dZ over samples)
                          in the bias strip of the n-half-0 partials               */
    int32_t n_slot;    /* slab index of the input window                               */
    int32_t n_cq0;     /* first channel quad of the window                             */
    int32_t n_quads;   /* valid quads (<= 64, multiple of 8)                           */
    int32_t kind;      /* 0 = dW block; 1 = logits-head rows: wave w owns channel quads
                          16 w .. 16 w + 15 of the window, partial slot segment.slot + w     */
} ffn_wgrad_unit;

int ffn_mlp_wgrad_units(const ffn_mlp_chain* chain, const ffn_wgrad_unit* units,
                        const ffn_wgrad_segment* segments, const int32_t* seg_start,
                        int num_groups, const float* saved, const float* dz,
                        const float* d_logits, int64_t n, float* partials, void* stream);
/* The same launch with every f32 product as three bf16 matrix products (OPT-IN "bf16x3" training
 * precision): same units, segments, slabs and partial format; ffn_mlp_wgrad_reduce is shared.
 * (Slabs are staged by LDS-DMA in half-block stages, operands converted one contraction step
 * ahead of the matrix instructions: csrc/wgrad_bf16.hip.) */
int ffn_mlp_wgrad_units_bf16x3(const ffn_mlp_chain* chain, const ffn_wgrad_unit* units,
                               const ffn_wgrad_segment* segments, const int32_t* seg_start,
                               int num_groups, const float* saved, const float* dz,
                               const float* d_logits, int64_t n, float* partials, void* stream);
/* Weight-gradient units of the f32-accurate "bf16x6" mode (csrc/wgrad_bf16x6.hip): ffn_mlp_wgrad_units with every f32
 * product as six bf16 matrix products on three-part operands; units, segments, partial format and
 * the reducer are shared with the exact-f32 and the bf16x3 kernels (the logits-head unit stays
 * exact f32).  The dZ window is double buffered; the input window is split just in time, hi parts
 * first, and the products are ordered by the part of it they need. */
int ffn_mlp_wgrad_units_bf16x6(const ffn_mlp_chain* chain, const ffn_wgrad_unit* units,
                               const ffn_wgrad_segment* segments, const int32_t* seg_start,
                               int num_groups, const float* saved, const float* dz,
                               const float* d_logits, int64_t n, float* partials, void* stream);

/* Fixed-order reduction of the partials of each job into the flat natural-layout
 * gradient buffer (nn.Linear weight (out,in) row-major, then bias). */
typedef struct ffn_reduce_job {
    int32_t kind;
    int32_t slot_begin, slot_end;  /* partial slots slot_begin, +stride, ... < slot_end      */
    int32_t m_ch0;                 /* kind 0: first output channel of the patch        */
    int32_t rows;                  /* output rows of the layer                         */
    int32_t n_quad0;               /* first input quad of the panel                    */
    int32_t n_quads;
    int32_t k_base;                /* index of the panel's first quad in col_map space */
    int32_t ld;                    /* leading dimension (= in_features) of dW          */
    int32_t has_bias;              /* this job also carries the bias gradient          */
    int32_t lg_n;
    int32_t slot_stride;           /* distance between consecutive slots of this job   */
    int32_t n_fold;                /* kind 0: 1, or the fold of a narrow input window: the
                                      exact-f32 unit kernel packs a window of <= 16 / <= 8
                                      quads into 2 / 1 column tiles (n_fold 2 / 4; column j of
                                      tile q = quad j % (32/n_fold), component
                                      (j / (32/n_fold)) * (4/n_fold) + q); the split-bf16 unit
                                      kernel does not fold (n_fold 1)                       */
    int32_t reserved;
    int64_t w_grad_off;            /* float offset of dW inside `grads`                */
    int64_t b_grad_off;            /* float offset of db inside `grads`                */
    const int32_t* col_map;        /* internal K index -> natural column, or -1        */
} ffn_reduce_job;

int ffn_mlp_wgrad_reduce(const ffn_reduce_job* jobs, int num_jobs, const float* partials,
                         float* grads, void* stream);

int64_t ffn_mlp_wgrad_partial_floats(void);

/* ---- K9: empty-space skipping for inference (opt-in).  The reference has no
 * counterpart on its render path (its octree ray walker, octree.py:418-501, serves only the
 * lecture visualisations), so parity here is PSNR-level, not sample-level.
 *
 * An occupancy grid is resolution^3 bits (cell (ix,iy,iz) = bit ((iz*G + iy)*G + ix), x fastest)
 * over the box [box_min, box_min + box_size); box_min / box_size are HOST pointers to 3 floats.
 *
 * ffn_occupancy_build: logits (G^3,4) = the model evaluated at the cell centres; a cell is
 *   occupied when softplus(sigma logit) > sigma_threshold; dilate != 0 also marks the 26
 *   neighbours (needs scratch_bits of the same size).
 * ffn_occupancy_count: block_offsets (ceil(n/256) int32) <- exclusive scan of the number of
 *   occupied samples per 256-sample block; *total (device int64) <- their sum.  A sample outside
 *   the box takes the occupancy of the nearest cell (indices clamped); NaN positions count as
 *   occupied.
 * ffn_occupancy_compact: packs the occupied samples (order preserved): out_positions /
 *   out_views (total,3), out_index (total) = their position in the input.
 * ffn_scatter_logits: out (n,4) <- (0,0,0,empty_sigma_logit) everywhere, then
 *   out[index[i]] = packed[i]. */
int ffn_occupancy_build(const float* logits, int resolution, float sigma_threshold, int dilate,
                        uint32_t* scratch_bits, uint32_t* bits, void* stream);
int ffn_occupancy_count(const float* positions, int64_t n, const float* box_min,
                        const float* box_size, int resolution, const uint32_t* bits,
                        int32_t* block_offsets, int64_t* total, void* stream);
int ffn_occupancy_compact(const float* positions, const float* views, int64_t n,
                          const float* box_min, const float* box_size, int resolution,
                          const uint32_t* bits, const int32_t* block_offsets,
                          float* out_positions, float* out_views, int32_t* out_index, void* stream);
int ffn_scatter_logits(const float* packed, const int32_t* index, int64_t m, int64_t n,
                       float empty_sigma_logit, float* out, void* stream);
/* K9g: packed[i] = full[index[i]] for (.,4) rows -- the backward of the scatter (training with
 * empty-space skipping: d_logits of the evaluated samples). */
int ffn_gather_logits(const float* full, const int32_t* index, int64_t m, float* packed,
                      void* stream);

/* ---- K10: dense voxel radiance field (voxels_model.py:35-45): trilinear lookup of a
 * (4,S,S,S) volume at positions/scale in [-1,1]^3 (grid_sample semantics: x = fastest axis,
 * border padding, align_corners = false) + bias (4) -> logits (N,4).  It is the opacity model
 * the README workflows hand to the focus sampler, and the forward pass of voxel training. */
int ffn_voxels_forward(const float* volume, const float* bias, const float* positions, int64_t n,
                       int side, float scale, float* out, void* stream);

/* ---- K10b: the adjoint of K10 -- the backward of Voxels.forward (voxels_model.py:35-45 of the
 * reference: grid_sample(padding_mode="border", align_corners=False) + bias, under autograd).
 *   positions (N,3), d_logits (N,4) (16-byte aligned), side S in [1, 1024], 0 <= N <= 2^30,
 *   finite scale > 0
 *   d_volume (4,S,S,S) out: EVERY entry written (no zeroing by the caller);
 *   d_bias (4) out: the column sums of d_logits
 *   workspace: ffn_voxels_backward_workspace(N, S) bytes (-1 for an invalid shape)
 * Same coordinate formula, clamp, corners and weight products as ffn_voxels_forward; a corner
 * clamped onto lo carries weight 0 and receives nothing.  No float atomics: the same inputs give
 * bit-identical outputs on every call (store-and-sum: per-cell lists in sample-id order, summed
 * per voxel over its 8 cells in a fixed order; lists longer than 16 in chunks of 16). */
int64_t ffn_voxels_backward_workspace(int64_t n, int side);
int ffn_voxels_backward(const float* positions, const float* d_logits, int64_t n, int side,
                        float scale, void* workspace, int64_t workspace_bytes, float* d_volume,
                        float* d_bias, void* stream);

/* ------------------------------------------------------------------------------------
 * K11  per-pixel regression loss of 2-D image regression (csrc/regression.hip).
 * Replaces torch.sigmoid(model(uv)), 0.5 * torch.square(out - y).mean() and their autograd
 * (train_image_regression.py:183-185), and the validation path sigmoid -> PixelDataset.psnr ->
 * PixelDataset.to_image (train_image_regression.py:141-142, pixel_dataset.py:168,189-198).
 *   logits (n,4) of the fused MLP, the first c columns used; target (n,c); 1 <= c <= 4, n >= 1.
 *   partials: ffn_regression_blocks(n) floats, one sum((sigmoid - y)^2) per workgroup.
 * No float atomics: the same inputs give the same bits.  Bad shapes / null pointers are refused
 * before any launch. */
int ffn_regression_blocks(int64_t n);

/* d_logits (n,4) out: ((sigmoid - y) * inv_count) * (1 - sigmoid) * sigmoid in f32 (ATen's
 * autograd order, inv_count = 1 / (n c)) for the first c columns, exactly 0 in the others. */
int ffn_regression_train(const float* logits, const float* target, int64_t n, int c,
                         float inv_count, float* d_logits, float* partials, void* stream);

/* Validation: partials (may be NULL; then target may be NULL) for the PSNR, and / or image
 * (n,c) u8 (may be NULL): (sigmoid * 255) truncated, as to_image's astype(np.uint8).  YCrCb
 * frames go on to ffn_ycrcb_to_rgb_u8. */
int ffn_regression_eval(const float* logits, const float* target, int64_t n, int c,
                        float* partials, uint8_t* image, void* stream);

/* Fixed-order sum of K11's partials: sse_out = sum (may be NULL), loss_out = 0.5 * (sum / count)
 * (may be NULL; count = n c). */
int ffn_regression_loss(const float* partials, int num_blocks, float count, float* sse_out,
                        float* loss_out, void* stream);

/* ------------------------------------------------------------------------------------
 * K11b  linear-output MSE of 1-D signal regression (csrc/regression.hip).
 * Replaces (model(x) - y).square().mean() and its autograd (train_signal_regression.py:81-85,
 * run over the full training set every step at :155-157) and the validation loss (:88-95).
 * No sigmoid and no 0.5 factor.  Same grid, partial layout (ffn_regression_blocks(n) floats) and
 * fixed-order sum as K11; logits (n,4) with the first c columns used, target (n,c), 1 <= c <= 4,
 * n >= 1.  No float atomics; bad shapes / null pointers are refused before any launch. */

/* d_logits (n,4) out: inv_count * (2 * (z - y)) in f32 (ATen's autograd order: MeanBackward's
 * 1 / count, then PowBackward's grad * (2 * r); inv_count = fl(1 / (n c))) for the first c
 * columns, exactly 0 in the others; partials: one sum((z - y)^2) per workgroup. */
int ffn_regression_mse_train(const float* logits, const float* target, int64_t n, int c,
                             float inv_count, float* d_logits, float* partials, void* stream);

/* Validation: partials only, bit-identical to ffn_regression_mse_train's. */
int ffn_regression_mse_eval(const float* logits, const float* target, int64_t n, int c,
                            float* partials, void* stream);

/* Fixed-order sum of the partials: sse_out = sum (may be NULL), loss_out = sum / count (may be
 * NULL; count = n c) -- not K11's 0.5 * (sum / count). */
int ffn_regression_mse_loss(const float* partials, int num_blocks, float count, float* sse_out,
                            float* loss_out, void* stream);

/* ------------------------------------------------------------------------------------
 * K12  sparse octree from a point cloud (csrc/octree.hip).  Node ids as the reference's: root 0,
 * children of i are 8 i + 1 .. 8 i + 8, child index 4 [x >= cx] + 2 [y >= cy] + [z >= cz]; node
 * centres are reached by f32 adds of +-scale / 2^k from the root, as the reference's Node
 * arithmetic does.  Integer decisions only, no float atomics, every result is the same bits on
 * every run.  Flag scans need three scratch arrays: flags (u8, one per element), offsets (i32,
 * one per element) and tile_sums (i32, ffn_octree_scan_tiles(elements)).  Element counts are
 * below 2^31; bad shapes / null pointers are refused before any launch. */
int64_t ffn_octree_scan_tiles(int64_t n);
/* the deepest voxel_depth the int32 path codes hold (3 bits per level below the root) */
int ffn_octree_max_depth(void);

/* Surface points of one render batch (voxelize_model.py:71-77): ray i is kept iff
 * alpha[i] > threshold; out_positions[k] = starts[i] + directions[i] * depth[i] (product and sum
 * rounded separately, as numpy), out_colors[k] = color[i] (channels floats per ray; 0 = none),
 * k = the number of kept rays before i (stable).  Outputs hold n rows; *count (device) = kept. */
int ffn_octree_surface_points(const float* alpha, const float* depth, const float* starts,
                              const float* directions, const float* color, int64_t n,
                              int channels, float threshold, uint8_t* flags, int* offsets,
                              int* tile_sums, float* out_positions, float* out_colors, int* count,
                              void* stream);

/* Path code of every point (octree.py:274-286 applied from the root down, replacing
 * _batch_assign at octree.py:502-508 level by level): p - center rounded to f32
 * (octree.py:760), then depth - 1 child indices, 3 bits each, the root's child in the highest. */
int ffn_octree_path_codes(const float* positions, int64_t n, float center_x, float center_y,
                          float center_z, float scale, int depth, int* codes, void* stream);

/* Tree structure by counting on the SORTED codes (octree.py:762-803): perm[i] = index of the
 * point at sorted position i (a stable sort).  A node is visited iff it is the root or its
 * parent is visited and it holds >= min_leaf_size points; a visited node at depth - 1 is a leaf
 * (the root too when depth == 1 and n >= min_leaf_size); a visited node above with no visited
 * child is a leaf holding all its points.  Out, per sorted position: leaf_sorted (leaf id or
 * -1), count_sorted (points of the node the walk stopped in); per point: leaf_of_point.  Out,
 * per leaf in code (depth-first) order, *num_leaves (device) of them in arrays of n entries:
 * leaf_ids, leaf_start (first sorted position), leaf_count. */
int ffn_octree_structure(const int* sorted_codes, const int64_t* perm, int64_t n, int depth,
                         int64_t min_leaf_size, int64_t* leaf_sorted, int* count_sorted,
                         int64_t* leaf_of_point, uint8_t* flags, int* offsets, int* tile_sums,
                         int64_t* leaf_ids, int64_t* leaf_start, int* leaf_count, int* num_leaves,
                         void* stream);

/* Interior nodes = the distinct proper ancestors of the leaves (the node_ids set of
 * octree.py:778 minus the leaves, octree.py:887).  leaf_ids in code order as K12's structure
 * step leaves them; scratch arrays sized for num_leaves * (depth - 1) elements; node_ids holds as
 * many; unsorted, *num_nodes (device) of them.  depth >= 2. */
int ffn_octree_interior_nodes(const int64_t* leaf_ids, int64_t num_leaves, int depth,
                              uint8_t* flags, int* offsets, int* tile_sums, int64_t* node_ids,
                              int* num_nodes, void* stream);

/* leaf_data[k] = mean of data[perm[leaf_start[k] + j]], j < leaf_count[k] (data[index].mean(0),
 * octree.py:775,802): one wave per leaf, a fixed summation order. */
int ffn_octree_leaf_means(const float* data, int64_t n, int channels, const int64_t* perm,
                          const int64_t* leaf_start, const int* leaf_count, int64_t num_leaves,
                          float* leaf_data, void* stream);

/* OcTree.query (octree.py:513-541): index into the sorted leaf_index of the leaf containing each
 * position, -1 outside the root cube (faces inclusive) or in an empty region.  A tree whose only
 * leaf is the root answers 0 inside the cube. */
int ffn_octree_query(const float* positions, int64_t n, float scale, const int64_t* node_index,
                     int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
                     int64_t* result, void* stream);

/* Centre (num_leaves,3) and depth of every leaf from its id alone (replaces the breadth-first
 * walk of octree.py:564-582 behind leaf_centers / leaf_depths, octree.py:605-613). */
int ffn_octree_leaf_geometry(const int64_t* leaf_index, int64_t num_leaves, float scale,
                             float* centers, int* depths, void* stream);

/* ------------------------------------------------------------------------------------
 * K13  ray walk through the octree (csrc/octree_walk.hip), one lane per ray.  starts and
 * directions (n,3) are in the tree's frame (relative to the root cube's centre, as for
 * ffn_octree_query); directions need not be unit length.  depth = 1 + the deepest leaf's level
 * (1 .. 11).  A REGION is a leaf or a maximal empty cell (a child slot of an interior node that is
 * in neither index).  Entry t of a region = the crossing of its bounding plane, (plane - o) / d in
 * f32, planes from the f32 chain of node centres; progress from region to region is decided on
 * integer cell coordinates of the finest grid (2^(depth-1) per axis) -- no epsilon nudge.  A zero
 * direction component constrains nothing if the start lies inside that slab of the root cube and
 * makes the ray a miss otherwise; NaNs and an all-zero direction are misses.  At most
 * (stops) * depth loop trips per ray for any input. */

/* OcTree.intersect (octree.py:418-501 _trace_ray_path / _batch_intersect, 707-731), the reference's
 * Path layout: t_stops (n,max_length) f32 and leaves (n,max_length) i64.  Stop k = the t at which
 * the ray enters its k-th region along the whole chord through the root cube (negative t when the
 * start is inside) and the region's index into leaf_index, -1 for an empty cell.  At most
 * max_length - 1 stops are written (octree.py:460); the other entries hold the cube's exit t
 * and -1 (octree.py:429-430).  A ray that misses the cube has every leaf -1 (its t_stops are 0).
 * max_length >= 2. */
int ffn_octree_walk(const float* starts, const float* directions, int64_t n, float scale,
                    int depth, const int64_t* node_index, int64_t num_nodes,
                    const int64_t* leaf_index, int64_t num_leaves, int max_length, float* t_stops,
                    int64_t* leaves, void* stream);

/* The same walk (octree.py:418-501) over the whole chord, reduced per ray to the span of the
 * leaves that end after t_min: hit = there is such a leaf; t_in = max(entry of the first one,
 * t_min) - w; t_out = exit of the last one + w, with w = pad finest-cell sides
 * (2 scale / 2^(depth-1)) measured along the ray, pad / |d| in t.  t_in = t_out = 0 without a
 * hit.  pad >= 0. */
int ffn_octree_spans(const float* starts, const float* directions, int64_t n, float scale,
                     int depth, const int64_t* node_index, int64_t num_nodes,
                     const int64_t* leaf_index, int64_t num_leaves, float t_min, float pad,
                     float* t_in, float* t_out, uint8_t* hit, void* stream);

/* ------------------------------------------------------------------------------------
 * K14  first hit of the K13 walk (csrc/octree_walk.hip, a third mode of the same kernel): the render
 * of a voxelized model, whose leaves are opaque surface cells with one colour each.  Replaces the
 * walker of octree.py:418-501 cut at the first leaf, and the leaf-cube view the reference hands to
 * scenepic (voxelize_model.py:90-110).  Arguments up to num_leaves as for K13.
 *
 * The ray's regions are walked in order; the hit is the first LEAF whose exit t is > t_min (the
 * predicate of ffn_octree_spans), and the walk ends there.  Per ray:
 *   leaf   index into leaf_index, -1 without a hit;
 *   t_hit  max(entry t, t_min) -- t_min itself, bit for bit, when it is the larger; 0 on a miss;
 *   face   the face the ray enters the leaf through: 2 * axis + (d[axis] > 0 ? 0 : 1), so that
 *          0 / 2 / 4 have the outward normal -x / -y / -z and 1 / 3 / 5 have +x / +y / +z; axis is
 *          the root cube's entry axis for the chord's first region and the exit axis of the region
 *          before otherwise.  6: the entry lies before t_min (the ray starts inside the leaf, or
 *          t_min lies inside it).  -1: a miss.
 * Rays K13 cannot follow (NaN or infinite components, an all-zero direction, a zero component
 * outside its slab) are misses.  t_min must not be NaN. */

#define FFN_OCTREE_SHADING_FLAT 0   /* color = leaf_data[leaf, :3] */
#define FFN_OCTREE_SHADING_FACES 1  /* color = leaf_data[leaf, :3] * k[face], one f32 multiply */
/* k: one factor per axis pair (x, y, z faces) and 1 for face 6 */
#define FFN_OCTREE_SHADE_X 0.8f
#define FFN_OCTREE_SHADE_Y 1.0f
#define FFN_OCTREE_SHADE_Z 0.6f
#define FFN_OCTREE_FACE_SHADE                                                                 \
    {FFN_OCTREE_SHADE_X, FFN_OCTREE_SHADE_X, FFN_OCTREE_SHADE_Y, FFN_OCTREE_SHADE_Y,          \
     FFN_OCTREE_SHADE_Z, FFN_OCTREE_SHADE_Z, 1.0f}

int ffn_octree_first_hit(const float* starts, const float* directions, int64_t n, float scale,
                         int depth, const int64_t* node_index, int64_t num_nodes,
                         const int64_t* leaf_index, int64_t num_leaves, float t_min, int64_t* leaf,
                         float* t_hit, int8_t* face, void* stream);

/* The same launch, shaded: leaf_data (num_leaves, channels) f32 with channels >= 3, of which the
 * first three are the colour.  color (n,3) = the hit leaf's colour (times k[face] with
 * FFN_OCTREE_SHADING_FACES), the background (bg_r, bg_g, bg_b) on a miss, both bit for bit;
 * alpha (n) = 1 on a hit and 0 otherwise; depth (n) = t_hit.  leaf, t_hit and face are written
 * too where they are not null. */
int ffn_octree_render(const float* starts, const float* directions, int64_t n, float scale,
                      int depth, const int64_t* node_index, int64_t num_nodes,
                      const int64_t* leaf_index, int64_t num_leaves, float t_min,
                      const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
                      int shading, float* color, float* alpha, float* depth_out, int64_t* leaf,
                      float* t_hit, int8_t* face, void* stream);

/* ------------------------------------------------------------------------------------
 * K15  volume render of the K13 walk (csrc/octree_walk.hip, a fourth mode of the same kernel): the
 * render of a BAKED tree, whose leaves hold a colour and a density (ffn_octree_bake).  No
 * counterpart in the reference.  Arguments up to num_leaves as for K13; leaf_data
 * (num_leaves, channels) f32 with channels >= 4: [r, g, b, sigma, ...], sigma per unit of world
 * length.  With channels == 4 a leaf is one aligned 16-byte load (leaf_data 16-byte aligned).
 *
 * Per ray, in f32, every operation rounded on its own (no fused multiply-add):
 *   norm = sqrtf(dx*dx + dy*dy + dz*dz);  T = 1, C = 0, w_best = 0, depth = 0
 *   for every region of the walk that is a leaf with t_exit > t_min (the predicate of
 *   ffn_octree_spans and K14), in walk order:
 *     t0    = max(t, t_min)                      t = the region's entry
 *     L     = (t_exit - t0) * norm
 *     sigma = fmaxf(leaf_data[leaf, 3], 0)       a NaN density counts as 0
 *     a     = 1 - expf(-(sigma * L))
 *     w     = T * a
 *     C    += w * leaf_data[leaf, 0..2]
 *     if w > w_best: w_best = w, depth = t0      strict: the first leaf wins a tie
 *     T     = T * (1 - a)
 *     the walk ends when T <= min_transmittance
 *   color = C + T * (bg_r, bg_g, bg_b);  alpha = 1 - T;  depth (0 when no leaf had w > 0)
 * The density is per world length, so the result does not depend on the length of the directions.
 * A ray that misses the cube, or that K13 cannot follow, gives the background, alpha 0 and depth 0,
 * as K14 does.  t_min must not be NaN; 0 <= min_transmittance < 1.  The trip bound of K13 holds. */
int ffn_octree_render_volume(const float* starts, const float* directions, int64_t n, float scale,
                             int depth, const int64_t* node_index, int64_t num_nodes,
                             const int64_t* leaf_index, int64_t num_leaves, float t_min,
                             const float* leaf_data, int channels, float bg_r, float bg_g,
                             float bg_b, float min_transmittance, float* color, float* alpha,
                             float* depth_out, void* stream);

/* Raw model logits (num_leaves,4) [r, g, b, sigma] -> leaf_data (num_leaves,4) f32
 * [sigmoid(r), sigmoid(g), sigmoid(b), softplus(sigma)] (softplus: beta 1, threshold 20): the
 * activations of the compositing kernels (ray_caster.py:66-74), bit for bit.  Both arrays are
 * 16-byte aligned. */
int ffn_octree_bake(const float* logits, int64_t num_leaves, float* leaf_data, void* stream);

/* ------------------------------------------------------------------------------------
 * K16  density octree from a trained model (csrc/octree.hip; the activations of K16b in
 * csrc/composite.hip).  The finest grid (level depth - 1, 2^(depth-1) cells per axis) is evaluated
 * densely in chunks of consecutive path codes (the codes of ffn_octree_path_codes), the cells with
 * sigma * side > tau become leaves, and siblings that agree are merged bottom-up.  No reference
 * counterpart: voxelize_model.py builds the one-cell shell of the depth renders only. */

/* K16a.  out (count,3): centre of the finest cell of code first_code + i, the f32 chain
 * +-scale / 2^k from 0 as ffn_octree_leaf_geometry makes it for the cell's id, then one f32 add of
 * the cube centre.  0 <= first_code, first_code + count <= 8^(depth-1).  No reference
 * counterpart. */
int ffn_octree_cell_centers(int64_t first_code, int64_t count, float center_x, float center_y,
                            float center_z, float scale, int depth, float* out, void* stream);

/* K16b.  logits (count,4): the model at the centres of K16a.  activated (count,4) = what
 * ffn_octree_bake makes of them (the same device functions, bit for bit); a cell is kept iff
 * activated[i, 3] * side > tau in f32 (strict; a NaN density is not kept).  The kept cells, in code
 * order (stable): codes_out (int32) and data_out (count,4), *total (device) of them in arrays of
 * count entries.  flags / offsets / tile_sums as for ffn_octree_surface_points
 * (ffn_octree_scan_tiles(count) tile sums).  logits, activated and data_out are 16-byte aligned.
 * No reference counterpart. */
int ffn_octree_density_select(const float* logits, int64_t first_code, int64_t count, float tau,
                              float side, int depth, uint8_t* flags, int* offsets, int* tile_sums,
                              float* activated, int* codes_out, float* data_out, int* total,
                              void* stream);

/* K16c.  One coarsening pass over a leaf list sorted by code: codes (n) left-aligned to the finest
 * level (a leaf of level l has zeros below its 3 l bits), levels (n), data (n,4).  Entry i heads a
 * group when its child index at `level` is 0, entries i .. i+7 are all leaves of `level` and entry
 * i+7 is child 7 of the same parent.  The group becomes its parent (level - 1, the head's code,
 * the mean) when |x - mean| <= rgb_tol for the first three channels and <= sigma_tol for the
 * fourth, for all eight; mean = the f32 sum of children 0 .. 7 in that order, times 0.125f, no
 * fused multiply-add.  A NaN in the group: no merge.  Everything else is copied; the output stays
 * sorted; *total (device) entries.  merge and flags hold n bytes; offsets / tile_sums as above.
 * 1 <= level <= depth - 1; tolerances >= 0; data and data_out 16-byte aligned.  Related to, but no
 * replacement of, OcTree.prune (octree.py:629-665), which merges unconditionally. */
int ffn_octree_merge_level(const int* codes, const int* levels, const float* data, int64_t n,
                           int level, int depth, float rgb_tol, float sigma_tol, uint8_t* merge,
                           uint8_t* flags, int* offsets, int* tile_sums, int* codes_out,
                           int* levels_out, float* data_out, int* total, void* stream);

/* ------------------------------------------------------------------------------------
 * K17  backward of the K15 volume render, for fitting a baked tree to images (K17a: a fifth mode
 * of the K13 kernel in csrc/octree_walk.hip; K17b, K17c: csrc/octree_grad.hip).  No counterpart in
 * the reference.  Arguments up to min_transmittance as for ffn_octree_render_volume, with the
 * same taken leaves, t0, L, sigma, a, w and T (the same f32 operations in the same order).  With
 * T_k the transmittance in front of taken leaf k = 1..n, w_k = T_k a_k, C = sum w_k c_k +
 * T_{n+1} bg, and the upstream gradients g_C = d_color[ray] (n,3), g_A = d_alpha[ray] (n):
 *   d c_k     = w_k g_C
 *   d sigma_k = L_k [ g_C . (T_{k+1} c_k - S_k) + g_A T_{n+1} ],   S_k = C - sum_{j<=k} w_j c_j
 * d sigma_k is 0 where the stored density is negative or NaN (it passes where it is exactly 0).
 * Depth has no gradient, leaves after an early end get nothing, and neither do the background,
 * the rays or rays that K13 cannot follow.  d_leaf_data (num_leaves,4) f32, 16-byte aligned:
 * every row is written, the sum of the leaf's contributions in a fixed order without float
 * atomics (the same inputs give the same bits on every call), zeros for a leaf no ray took.
 *
 * C and T_{n+1} come from a first walk (which also counts the taken leaves of every ray), not
 * from the forward's outputs.  The call reads the total number of (ray, taken leaf) entries back
 * ONCE (it synchronises the stream) and stores it in *entries (host, may be null).  The
 * workspace (16-byte aligned, ffn_octree_grad_workspace_bytes(n, num_leaves, max_entries) bytes)
 * holds max_entries of them: with more the call fails, *entries says how many there are, and
 * nothing has been written to d_leaf_data.  n * (3 * 2^(depth-1) + 1) < 2^31. */
int64_t ffn_octree_grad_workspace_bytes(int64_t n, int64_t num_leaves, int64_t max_entries);

int ffn_octree_render_volume_backward(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_data, int64_t* entries,
    void* stream);

/* K17c.  The projection after an optimiser step, in place on leaf_data (num_leaves,4) f32,
 * 16-byte aligned: r, g, b = min(max(x, 0), 1), sigma = max(x, 0); a NaN becomes 0. */
int ffn_octree_project(float* leaf_data, int64_t num_leaves, void* stream);

/* ------------------------------------------------------------------------------------
 * K18  view-dependent colour in a baked tree: spherical harmonics per leaf.  No counterpart in the
 * reference.  B = (degree + 1)^2, degree 1 or 2.  A leaf holds 3 B coefficients k in logit space and
 * a density; its colour for the unit vector u = (x, y, z) is sigmoid(sum_b k[c B + b] Y_b(u)) with
 *   Y_0 = 0.28209479177387814
 *   Y_1 = -0.4886025119029199 y     Y_2 = 0.4886025119029199 z     Y_3 = -0.4886025119029199 x
 *   Y_4 = 1.0925484305920792 xy     Y_5 = -1.0925484305920792 yz
 *   Y_6 = 0.31539156525252005 (2zz - xx - yy)
 *   Y_7 = -1.0925484305920792 xz    Y_8 = 0.5462742152960396 (xx - yy)
 *
 * K18a (csrc/octree_walk.hip, two more modes of the K13 kernel).  ffn_octree_render_volume with
 * that colour: u = direction / norm, not negated, its basis computed once per ray; the dot product
 * is a chain of fused multiply-adds from b = 0, the sigmoid ffn_octree_bake's.  Everything else (t0,
 * L, sigma, a, w, T, the depth, the early end, the background, a miss) is K15's, operation for
 * operation: on the same structure and densities alpha and depth have K15's bits.  A direction of
 * length 0 is a miss like any other and leaks no NaN.  leaf_data is the DEVICE layout, 16-byte
 * aligned: rows of row_stride floats [sigma, k_r0 .. k_r(B-1), k_g0 .., k_b0 .., padding];
 * channels == 3 B + 1 <= row_stride <= 64, row_stride a multiple of 4.  The other arguments as for
 * ffn_octree_render_volume. */
int ffn_octree_render_volume_sh(const float* starts, const float* directions, int64_t n,
                                float scale, int depth, const int64_t* node_index,
                                int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
                                float t_min, const float* leaf_data, int channels, float bg_r,
                                float bg_g, float bg_b, float min_transmittance, float* color,
                                float* alpha, float* depth_out, int degree, int row_stride,
                                void* stream);

/* K18b (csrc/composite.hip).  One view of the projection of a model onto the basis: logits
 * (num_leaves,4), 16-byte aligned, the model at the leaves for ONE view direction; weights (B
 * floats, HOST memory) that view's column of the pseudo-inverse of the basis matrix.  In place on
 * leaf_data (num_leaves, 3 B + 1) f32 in the FILE layout [k_r0 .. k_r(B-1), k_g0 .., k_b0 .., sigma]:
 *   k[c B + b] = k[c B + b] + weights[b] * logits[c]     one multiply, one add, no fused multiply-add
 *   sigma      = sigma + softplus(logits[3]) * inv_views  the softplus of ffn_octree_bake
 * One thread per leaf, no atomics: the same calls in the same order give the same bits. */
int ffn_octree_sh_accumulate(const float* logits, int64_t num_leaves, int degree,
                             const float* weights, float inv_views, float* leaf_data, void* stream);

/* ------------------------------------------------------------------------------------
 * K19  backward of the K18a SH volume render, for fitting SH leaves to images (K19a: two more modes
 * of the K13 kernel in csrc/octree_walk.hip; K19b, K19c: csrc/octree_grad.hip).  No counterpart in
 * the reference.  Arguments up to min_transmittance as for ffn_octree_render_volume_sh (leaf_rows is
 * its DEVICE layout, row_stride floats per row), with the same taken leaves, t0, L, sigma, a, w, T,
 * basis Y(u) and colour c_k = sigmoid(k . Y(u)), operation for operation.  With K17's notation
 * (T_k, w_k, C = sum w_k c_k + T_{n+1} bg, S_k = C - sum_{j<=k} w_j c_j, upstream g_C, g_A), taken
 * leaf k of a ray contributes
 *   d k_cb    = e_kc Y_b(u),   e_kc = (w_k g_c) (c_kc (1 - c_kc))    each product rounded, in f32
 *   d sigma_k = L_k [ g_C . (T_{k+1} c_k - S_k) + g_A T_{n+1} ]      K17's expression and order
 * d sigma_k is 0 where the stored density is negative or NaN (it passes where it is exactly 0);
 * depth, the background and the rays get no gradient.  d_leaf_rows (num_leaves, row_stride) f32,
 * 16-byte aligned, in the layout of leaf_rows [d sigma, d k_r0 .., d k_g0 .., d k_b0 .., padding]:
 * every row is written, the sum of the leaf's contributions in K17b's fixed tree without float
 * atomics (the same inputs give the same bits on every call); rows of leaves no ray took and all
 * padding columns are +0.  An entry of the walk stays 16 + 4 + 4 bytes (e_r, e_g, e_b, d sigma, the
 * leaf, the ray): Y_b(u) is rebuilt from the ray's direction when the entries are summed.
 *
 * The read-back of the entry total, *entries and the workspace protocol are those of
 * ffn_octree_render_volume_backward, with ffn_octree_grad_sh_workspace_bytes(n, num_leaves,
 * max_entries, degree) bytes, which grow by less than 96 bytes per additional entry.  degree is 1 or
 * 2; 3 (degree + 1)^2 + 1 <= row_stride <= 64, a multiple of 4; n * (3 * 2^(depth-1) + 1) < 2^31. */
int64_t ffn_octree_grad_sh_workspace_bytes(int64_t n, int64_t num_leaves, int64_t max_entries,
                                           int degree);

int ffn_octree_render_volume_sh_backward(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_rows, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_rows, int64_t* entries, int degree,
    int row_stride, void* stream);

/* K19c.  The projection after an optimiser step, in place on leaf_rows (num_leaves, row_stride) f32
 * in the device layout, 16-byte aligned: density = max(x, 0) (NaN and -0 become +0); a coefficient
 * that is NaN becomes 0 and is otherwise untouched (it lives in logit space); padding untouched. */
int ffn_octree_project_sh(float* leaf_rows, int64_t num_leaves, int row_stride, int degree,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * K29  a per-ray distortion prior for fitting a tree (csrc/octree_walk.hip: K29a a mode of the K13
 * kernel built as K21a is, K29b three gradient modes; the entries of K29b: csrc/octree_grad.hip).
 * The distortion loss of Mip-NeRF 360 on the piecewise-constant weights of an octree ray; no
 * counterpart in the reference.  For one ray, with the taken leaves k = 1..n of
 * ffn_octree_render_volume in walk order and its t0_k, L_k, sigma_k, a_k, w_k = T_k a_k, T_{k+1}
 * (the same f32 operations in the same order), m_k = (0.5 (t0_k + t_exit_k)) |d| the chord's midpoint
 * as a world length, W_k = sum_{j<k} w_j and M_k = sum_{j<k} w_j m_j:
 *   D = sum_k [ (2 w_k) (m_k W_k - M_k) + (w_k w_k) (L_k / 3) ]
 *     = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 L_i      (the leaves are disjoint and ordered)
 * in f32, summed front to back.  Lengths are world lengths; the background's share takes no part.
 *
 * K29a.  Arguments up to min_transmittance as for ffn_octree_leaf_weights (rows of `stride` floats of
 * which only rows[leaf, sigma_offset] is read; stride >= 1, 0 <= sigma_offset < stride).
 * distortion (n) f32: D per ray, +0 for a ray that takes no leaf, that misses the cube or that K13
 * cannot follow.  Nothing is written per leaf, no atomics: the same inputs give the same bits. */
int ffn_octree_distortion(const float* starts, const float* directions, int64_t n, float scale,
                          int depth, const int64_t* node_index, int64_t num_nodes,
                          const int64_t* leaf_index, int64_t num_leaves, float t_min,
                          const float* rows, int stride, int sigma_offset, float min_transmittance,
                          float* distortion, void* stream);

/* K29b.  ffn_octree_render_volume_backward / ffn_octree_render_volume_sh_backward with the term
 * folded into their two walks: the arguments of the parents in their order, then dist_scale and
 * ray_distortion.  Only densities receive a gradient (m and L are geometry, colours do not enter):
 *   G_k         = 2 [ (m_k W_k - M_k) + (M_tot - M_{k+1}) - m_k (W_tot - W_{k+1}) ] + (2/3) (w_k L_k)
 *   dD/dsigma_k = L_k [ T_{k+1} G_k - (2 D - sum_{j<=k} w_j G_j) ]        (sum_j w_j G_j = 2 D)
 * and every entry's d sigma becomes (parent's d sigma) + dist_scale * dD/dsigma_k: one f32 multiply,
 * one f32 add, one rounding each; 0 where the stored density is negative or NaN, as in the parent.
 * The first walk also leaves W_tot, M_tot and D per ray (12 n bytes behind the parent's workspace
 * layout, which is otherwise unchanged: ffn_octree_grad_dist_workspace_bytes(n, num_leaves,
 * max_entries, degree) with degree 0 for plain rows is the parent's size plus those bytes, rounded
 * up to 256) and, where ray_distortion (n) f32 is not null, D there: the bits of
 * ffn_octree_distortion on the same rays and densities, for plain rows and for SH rows.  The colour
 * columns, the entry list, the per-leaf sums, *entries and the workspace protocol are the parents'.
 * dist_scale is the caller's weight / number of rays; finite and >= 0, refused by name before
 * anything else.  No float atomics: the same inputs give the same bits on every call. */
int64_t ffn_octree_grad_dist_workspace_bytes(int64_t n, int64_t num_leaves, int64_t max_entries,
                                             int degree);

int ffn_octree_render_volume_backward_dist(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_data, int channels, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_data, int64_t* entries,
    float dist_scale, float* ray_distortion, void* stream);

int ffn_octree_render_volume_sh_backward_dist(
    const float* starts, const float* directions, int64_t n, float scale, int depth,
    const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index, int64_t num_leaves,
    float t_min, const float* leaf_rows, float bg_r, float bg_g, float bg_b,
    float min_transmittance, const float* d_color, const float* d_alpha, void* workspace,
    int64_t workspace_bytes, int64_t max_entries, float* d_leaf_rows, int64_t* entries, int degree,
    int row_stride, float dist_scale, float* ray_distortion, void* stream);

/* ------------------------------------------------------------------------------------
 * K20  a total-variation prior between leaves that touch across a face (csrc/octree_tv.hip).  No
 * counterpart in the reference.
 *
 * K20a.  neighbors (num_leaves, 6) int32, directions -x, +x, -y, +y, -z, +z.  A leaf's id gives its
 * level d and its cell (ix, iy, iz) on the 2^d grid (child index 4 [x] + 2 [y] + [z], as K12).  One
 * cell along the axis: outside [0, 2^d) the answer is -1; otherwise that cell's path is followed from
 * the root (id = 8 id + 1 + child) with K12j's binary searches.  An id in leaf_index answers with its
 * position in leaf_index (a leaf of equal size or coarser); an id in neither index is empty space,
 * -1; an id that is still an interior node at level d means finer leaves on the other side, -1: they
 * hold the adjacency from their side.  A root-only tree has no neighbours.  Integers only. */
int ffn_octree_neighbors(const int64_t* node_index, int64_t num_nodes, const int64_t* leaf_index,
                         int64_t num_leaves, int32_t* neighbors, void* stream);

/* K20b + K20c.  The plan, made once per tree by the caller, all arrays int32 on the device:
 * (i, dir) is an EDGE when j = neighbors[i][dir] >= 0 and (level(j) < level(i) or dir is a +
 * direction): every touching pair once.  Edges are numbered in (i, dir) order: edge_i, edge_j
 * (num_edges each).  Edge e has the incidences 2 e = (leaf edge_i[e], +) and 2 e + 1 = (leaf
 * edge_j[e], -); inc_leaf / inc_code (2 num_edges each) hold the incidences' leaves and numbers
 * stably sorted by leaf, seg_lo / seg_hi (num_leaves each) leaf l's range [lo, hi) in that order
 * (hi == lo without an incidence), seg_base[l] = seg_lo[l] / 16 + (leaves with an incidence before
 * l), longest = max (hi - lo).  num_edges <= 6 num_leaves, 2 num_edges < 2^31.
 *
 * rows (num_leaves, stride) f32, 16-byte aligned, stride a multiple of 4 in 4 .. 64: [r, g, b, sigma]
 * or the device layout of K18a.  lambda: stride floats in HOST memory, finite and >= 0 (0 for
 * padding columns).  eps > 0.  With d = rows[i][c] - rows[j][c] over the edges (i, j):
 *   R          = (1 / E) sum_e sum_c lambda_c (sqrt(d^2 + eps^2) - eps)         (Charbonnier)
 *   dR/drows[i][c] += (lambda_c / E) d / sqrt(d^2 + eps^2),   dR/drows[j][c] -= the same
 * in f32, in this order: scale_c = lambda_c / (float)E on the host; d = a - b; s = sqrtf(fmaf(d, d,
 * eps * eps)); the term (s - eps) * scale_c; the derivative (d / s) * scale_c.  No fused
 * multiply-add but the one written; sqrt and division are IEEE.  There is no geometric weight for
 * the face's area or the distance of the centres.
 *
 * *value (device) = R: a thread adds its four columns ((x + y) + z) + w, a workgroup of 256 (edge,
 * quad) threads its terms in a fixed shuffle / LDS tree, one workgroup the partials in index order.
 * d_rows (num_leaves, stride), 16-byte aligned, may be null (the energy alone): leaf l's row is the
 * sum of its incidences' signed derivatives in the sorted order, in runs of 16 and runs of 16 partial
 * sums (K17b's tree: no thread adds more than 16 terms), every row written, +0 for a leaf without
 * an incidence and for a column of weight 0; with accumulate != 0, d_rows = d_rows + that sum, one
 * add per element.  No float atomics and no read-back: the same inputs give the same bits.
 * num_edges == 0: *value = 0, d_rows zero (untouched with accumulate).  The indices of a plan are
 * held against num_leaves and num_edges where they are used: a plan of another tree gives wrong
 * sums, not an access outside the buffers.  workspace: 16-byte aligned,
 * ffn_octree_tv_workspace_bytes(num_leaves, num_edges, stride) bytes (-1: bad shape). */
int64_t ffn_octree_tv_workspace_bytes(int64_t num_leaves, int64_t num_edges, int stride);

int ffn_octree_tv(const float* rows, int64_t num_leaves, int stride, const int32_t* edge_i,
                  const int32_t* edge_j, int64_t num_edges, const int32_t* inc_leaf,
                  const int32_t* inc_code, const int32_t* seg_lo, const int32_t* seg_hi,
                  const int32_t* seg_base, int64_t longest, const float* lambda, float eps,
                  float* value, float* d_rows, int accumulate, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * K21  refining a fitted tree: which leaves the rays see, and a rebuild from a decision per leaf.
 * No counterpart in the reference (its prune merges the deepest level into its parents).
 *
 * K21a (csrc/octree_walk.hip, a tenth mode of the K13 kernel).  Arguments up to num_leaves and t_min
 * as for ffn_octree_render_volume.  leaf_data (num_leaves, stride) f32 rows of which only the density
 * leaf_data[leaf, sigma_offset] is read: stride 4 and offset 3 for [r, g, b, sigma], stride 16 / 28
 * and offset 0 for the device layout of K18a; stride >= 1, 0 <= sigma_offset < stride, no alignment
 * asked.  Per ray, K15's operations in K15's order on the same taken leaves (t_exit > t_min):
 *     t0 = max(t, t_min);  L = (t_exit - t0) * norm;  sigma = fmaxf(density, 0);
 *     a = 1 - expf(-(sigma * L));  w = T * a;  T = T * (1 - a);  ends when T <= min_transmittance
 * so w has the bits ffn_octree_render_volume composites with.  For every taken leaf with w > 0:
 *     weights[leaf] = max(weights[leaf], bits of w)
 * weights (num_leaves) uint32 holds f32 bit patterns, monotone for w >= 0, so the maximum is an
 * integer atomic maximum: exact, and the same bits for the same rays in any order, in one call or
 * split over many.  The caller zeroes weights (all bits 0 = +0.0f) or lets calls fold into it;
 * nothing is written per ray, and a leaf no ray takes with w > 0 keeps what it held.  A negative
 * or NaN density weighs 0; a ray that misses the cube, or that K13 cannot follow, touches nothing.
 * t_min must not be NaN; 0 <= min_transmittance < 1.  The trip bound of K13 holds. */
int ffn_octree_leaf_weights(const float* starts, const float* directions, int64_t n, float scale,
                            int depth, const int64_t* node_index, int64_t num_nodes,
                            const int64_t* leaf_index, int64_t num_leaves, float t_min,
                            const float* leaf_data, int stride, int sigma_offset,
                            float min_transmittance, uint32_t* weights, void* stream);

/* K21b (csrc/octree.hip), in two calls around one read-back of the new leaf count.
 * action (num_leaves) uint8 per leaf IN PATH-CODE ORDER: 0 drop, 1 keep, 2 split into the eight
 * children, child order 4 bx + 2 by + bz (the order stays code order).  Leaf i owns the slots
 * 8 i .. 8 i + 7: a keep flags slot 8 i, a split all eight, any other value none.
 * ffn_octree_refine_count: flags / offsets (8 num_leaves each) and tile_sums
 * (ffn_octree_scan_tiles(8 num_leaves)) as for ffn_octree_surface_points; *total (device) = the new
 * leaf count.  8 num_leaves < 2^31, which holds the new count below 2^31 too.
 * ffn_octree_refine_scatter: with the flags and offsets of the first call and out_leaves = *total,
 * output leaf o of slot 8 i + k gets ids_out[o] = leaf_ids[i] (keep) or 8 leaf_ids[i] + 1 + k
 * (split), parent[o] = i, and rows_out[o] = rows[i] bit for bit (rows (num_leaves, channels),
 * channels >= 0, null when 0; moved 16 bytes at a time when channels is a multiple of 4 and both
 * arrays are 16-byte aligned, word by word otherwise).  Nothing beyond out_leaves entries is
 * written.  No atomics.  Whether a split leaf is too deep for K13 is the caller's check. */
int64_t ffn_octree_max_points(void);   /* the most elements one K12 flag scan holds: 2^31 - 2048 */

int ffn_octree_refine_count(const uint8_t* action, int64_t num_leaves, uint8_t* flags, int* offsets,
                            int* tile_sums, int* total, void* stream);

int ffn_octree_refine_scatter(const uint8_t* action, const uint8_t* flags, const int* offsets,
                              const int64_t* leaf_ids, const float* rows, int64_t num_leaves,
                              int channels, int64_t out_leaves, int64_t* ids_out, float* rows_out,
                              int32_t* parent, void* stream);

/* FFN_OCTREE_FACE_SHADE as the kernel was compiled with it, into table[7] (host memory). */
void ffn_octree_face_shade(float* table);

/* K22 (csrc/mesh.hip): surface samples of a textured triangle mesh, one thread per sample.  Replaces
 * the reference's host-side sampler, octree.py:42-136 (_sample_regular_barys,
 * _barycentric_interpolation, _sample_barycentric_point_cloud after the counts are drawn) and
 * utils.py:197-241 (interpolate_bilinear) with the / 255 of octree.py:849.
 * vertices (num_vertices,3) f32, triangles (num_triangles,3) i32, uvs (num_vertices,2) f32, offsets
 * (num_triangles + 1) i32: the exclusive prefix sum of the per-triangle sample counts, offsets[0] = 0
 * and offsets[num_triangles] = n.  texture (height, width, channels) u8, channels >= 3, row index
 * growing with v.  positions (n,3), colors (n,3) f32; sample_uvs (n,2) f32 or null (not written).
 * Sample s, every operation one rounded f32 operation in this order (no fma):
 *     f: offsets[f] <= s < offsets[f + 1] (triangles of count 0 are skipped);  number = s - offsets[f] + 1
 *     A = (1,0), B = (0,1), C = (0,0);  for i = 0 .. 15, d = (number >> 2 i) & 3:
 *         d = 0: (A,B,C) = ((B+C)/2, (A+C)/2, (A+B)/2)      d = 1: (A, (A+B)/2, (A+C)/2)
 *         d = 2: ((B+A)/2, B, (B+C)/2)                      d = 3: ((C+A)/2, (C+B)/2, C)
 *     p = ((A + B) + C) / 3 (IEEE division);  (b0, b1, b2) = (p.x, p.y, 1 - (p.x + p.y))
 *     value = (x0 b0 + x1 b1) + x2 b2 per component of the triangle's three positions and UVs
 *     col = u width, row = v height;  j0 = floor(col), i0 = floor(row);  dj = col - j0, di = row - i0;
 *     j0, i0, j0 + 1, i0 + 1 clamped to the image after that;  per channel 0 .. 2
 *     (((1-di)(1-dj) t00 + (1-di) dj t01) + di (1-dj) t10) + di dj t11, then / 255 (IEEE division)
 * The rounds are exact (multiples of 2^-16); d is the reference's digit while number < 2^24, which
 * the caller checks, as it checks the vertex ids (0 <= id < num_vertices: the kernel clamps an id,
 * so a bad one reads a wrong vertex, not foreign memory), the offsets and finite UVs.  A texel index
 * is clamped in f32, so any u, v (NaN and infinities included) reads inside the texture.
 * n <= ffn_octree_max_points(); height, width <= 2^24; height * width * channels < 2^31.  No
 * atomics, no LDS, no dependence on the launch shape: the same inputs give the same bits. */
int ffn_mesh_sample(const float* vertices, int64_t num_vertices, const int32_t* triangles,
                    int64_t num_triangles, const float* uvs, const int32_t* offsets, int64_t n,
                    const uint8_t* texture, int height, int width, int channels, float* positions,
                    float* colors, float* sample_uvs, void* stream);

/* K23 (csrc/carve.hip): space carving, an octree's finest cells from the images' silhouettes, one
 * thread per cell.  No reference counterpart: nothing in the reference builds a tree from a dataset
 * alone (octree.py builds from a mesh, voxelize_model.py from a trained model's depth renders).
 * images (cameras, height, width, 4) u8 RGBA, 4-byte aligned; mask (cameras, height, width) u8, a
 * pixel is background where it is 0; proj (cameras, 3, 4) f32 row-major, world -> homogeneous
 * pixel, finite (the caller checks).  The cells first_code .. first_code + count - 1 of the finest
 * level as for ffn_octree_cell_centers, whose centre p (the cube centre included) cell i takes, bit
 * for bit.  Per cell, camera c = 0 .. cameras-1 in that order, every operation one rounded f32
 * operation (no fma):
 *     x = ((P00 p.x + P01 p.y) + P02 p.z) + P03, likewise y (row 1) and w (row 2)
 *     !(w > 0): not seen (NaN too).  fu = x / w + 0.5f, fv = y / w + 0.5f (IEEE divisions)
 *     seen iff fu >= 0 && fu < width && fv >= 0 && fv < height;  col = (int)fu, row = (int)fv
 *     seen += 1;  mask[c, row, col] == 0: misses += 1, and misses > max_misses ends the loop, the
 *     cell is carved;  otherwise, if the pixel's own alpha >= alpha_u8, its r, g, b are added to
 *     three uint32 sums and colored += 1
 * A cell is kept iff it was not carved and seen >= min_views.  Its row is [r, g, b, sigma0],
 * r = (float)sum_r / (float)(255 colored) (IEEE division), 0.5f for all three when colored == 0.
 * cameras <= ffn_octree_carve_max_cameras() = 65793, so that 255 cameras is exact in f32.
 * The kept cells in code order (stable): codes_out (int32) and data_out (count,4), *total (device)
 * of them, in arrays of count entries.  flags / offsets / tile_sums as for
 * ffn_octree_density_select, whose scan and scatter this shares; rows (count,4) f32 is scratch;
 * rows and data_out are 16-byte aligned.  visited (count) int32 or null: how many cameras the
 * loop of cell i looked at before it ended.  1 <= alpha_u8 <= 255; max_misses, min_views >= 0;
 * height, width <= 2^24.  No atomics; the same inputs give the same bits. */
int ffn_octree_carve_max_cameras(void);
int ffn_octree_carve_select(const uint8_t* images, const uint8_t* mask, const float* proj,
                            int cameras, int height, int width, int64_t first_code,
                            int64_t count, float center_x, float center_y, float center_z,
                            float scale, int depth, int alpha_u8, int max_misses, int min_views,
                            float sigma0, uint8_t* flags, int* offsets, int* tile_sums,
                            float* rows, int* visited, int* codes_out, float* data_out,
                            int* total, void* stream);

/* K27 (csrc/carve_box.hip): one level of a conservative, coarse-to-fine space carve, one thread
 * per candidate cell of level `level` (0 = the root cube, depth - 1 = the finest).  No reference
 * counterpart.  images / proj / cameras / height / width / the cube / depth / alpha_u8 / max_misses
 * / min_views / sigma0 as for ffn_octree_carve_select.  sat (cameras, height + 1, width + 1) int32:
 * sat[c][r][q] = the foreground pixels of camera c's (grown) mask in rows < r and columns < q, so
 * height * width < 2^31.  candidates: int32 path codes of level `level`, in [0, 8^level) (only
 * their low 3 level bits are read; no memory is indexed by a code).  expand == 0: candidate i is
 * candidates[i], count entries.  expand == 1 (level >= 1): candidate i is
 * (candidates[i >> 3] << 3) | (i & 7), the children of count / 8 parents of level - 1, count a
 * multiple of 8; the children are never written out.  Per (candidate, camera c = 0 .. cameras-1
 * in that order), every operation one rounded f32 operation (no fma):
 *     q0 = the cell's centre as ffn_octree_cell_centers makes it for depth = level + 1, h = scale
 *     halved `level` times;  q1 .. q8 = (q0.x -+ h, q0.y -+ h, q0.z -+ h)
 *     each point: x, y, w as K23;  in front iff w > 0;  fu = x / w + 0.5f, fv = y / w + 0.5f;  a
 *     non-finite fu or fv of a point in front: the camera is undecided;  col = (int)floorf(fu
 *     clamped to +-2^30), row likewise
 *     [c0, c1] x [r0, r1] = min / max over the points in front, widened by
 *     pad = 1 + (depth - 1 - level) pixels on every side
 *     inside iff all nine in front, not undecided, 0 <= c0, c1 <= width - 1, 0 <= r0,
 *     r1 <= height - 1;  miss iff inside and sat counts no foreground pixel in the rectangle
 *     seen iff some point in front and (undecided or some point not in front or the rectangle
 *     meets the image)
 *     misses > max_misses ends the loop, the cell is rejected
 * A camera that does not see the whole cell never refutes it.  A candidate survives iff it was not
 * rejected and, at the finest level only, seen >= min_views.  Containment: the padded rectangle of
 * a child lies inside its parent's (the pad shrinks by one pixel per level, which covers the f32
 * rounding of the projection as long as that stays below half a pixel), so a cell that survives
 * at max_misses implies that its parent survives, and testing only the children of survivors
 * gives the set that testing every finest cell gives.  At the finest level a survivor's row is
 * [r, g, b, sigma0] with K23's colour from q0's own projection (in front and on the image, the pixel
 * votes iff its own alpha >= alpha_u8; 0.5f without a vote): a cell K23 keeps too has K23's row
 * bit for bit.  Below the finest level rows are not written and data_out is undefined.
 * The survivors in candidate order (stable): codes_out (int32) and data_out (count,4), *total
 * (device) of them, in arrays of count entries.  flags / offsets / tile_sums / rows / visited as
 * for ffn_octree_carve_select.  Refused by name before any launch: level outside 0 .. depth - 1,
 * count outside 1 .. ffn_octree_max_points(), cameras outside 1 .. ffn_octree_carve_max_cameras(),
 * height or width outside 1 .. 2^24 or height * width >= 2^31, alpha_u8 outside 1 .. 255, negative
 * max_misses or min_views, a null or misaligned buffer.  No atomics; the same inputs give the same
 * bits. */
int ffn_octree_carve_box_level(const uint8_t* images, const int32_t* sat, const float* proj,
                               int cameras, int height, int width, const int32_t* candidates,
                               int64_t count, int expand, int level, float center_x,
                               float center_y, float center_z, float scale, int depth,
                               int alpha_u8, int max_misses, int min_views, float sigma0,
                               uint8_t* flags, int* offsets, int* tile_sums, float* rows,
                               int* visited, int* codes_out, float* data_out, int* total,
                               void* stream);

/* K24 (csrc/octree_walk.hip, an eleventh mode of the K13 kernel): which cameras see a leaf through
 * the tree as it stands, and the sum of what they see there.  No counterpart in the reference.
 * One lane per (leaf, camera) pair, the camera in blockIdx.y; no ray is ever stored.
 * leaf_centers (num_leaves,3) f32 as ffn_octree_leaf_geometry writes them, relative to the root
 * cube's centre; scale .. leaf_index as for ffn_octree_walk; leaf_data / stride / sigma_offset as
 * for ffn_octree_leaf_weights (only the density is read).  images (cameras, height, width, 4) u8
 * RGBA, 4-byte aligned.  camera_blocks (cameras, 16) f32: P' (3x4 row-major, cube-relative point ->
 * homogeneous pixel), the eye relative to the cube's centre, one float of padding.  Pair (leaf l
 * with centre p, camera c), every operation one rounded f32 operation (no fma):
 *     x = ((P00 p.x + P01 p.y) + P02 p.z) + P03, likewise y (row 1) and w (row 2)
 *     !(w > 0): no vote (NaN too).  fu = x / w + 0.5f, fv = y / w + 0.5f (IEEE divisions)
 *     no vote unless fu >= 0 && fu < width && fv >= 0 && fv < height;  the pixel is
 *     images[c, (int)fv, (int)fu], one aligned 4-byte load;  no vote if its alpha < alpha_u8
 *     o = eye, d = p - o (the centre lies at t = 1), norm = sqrtf(d.x^2 + d.y^2 + d.z^2)
 *     the K13 walk with t_min = 0 and T = 1; per leaf with t_exit > 0, in order:
 *         leaf l itself: the pair is visible, the walk ends
 *         t0 = max(t, 0);  L = (t_exit - t0) * norm;  sigma = fmaxf(density, 0);
 *         a = 1 - expf(-(sigma * L));  T = T * (1 - a);  T <= min_transmittance: occluded, ends
 *     a walk that ends without meeting l (a miss of the cube, the trip bound of K13) is not visible
 * A visible pair adds the pixel's r, g, b and 1 to votes[l] = [sum_r, sum_g, sum_b, count] (uint32),
 * as two 64-bit integer atomic adds of two fields each: exact, the same bits for the same pairs in
 * any order, in one call or split over many.  votes (num_leaves,4) is 16-byte aligned; the caller
 * zeroes it or lets calls fold into it, and keeps the cameras that fold into one buffer at or below
 * ffn_octree_carve_max_cameras(), so that a sum stays below 2^24, the count below 2^17 and
 * 255 count exact in f32 (the colour is (float)sum / (float)(255 count), as K23).
 * 1 <= num_leaves <= 2^31, 1 <= depth <= 11, cameras >= 1 (launched 65535 at a time),
 * 1 <= height, width <= 2^24, 1 <= alpha_u8 <= 255, 0 <= min_transmittance < 1, stride >= 1,
 * 0 <= sigma_offset < stride; each refused by name before any launch. */
int ffn_octree_visible_votes(const float* leaf_centers, int64_t num_leaves, float scale, int depth,
                             const int64_t* node_index, int64_t num_nodes,
                             const int64_t* leaf_index, const float* leaf_data, int stride,
                             int sigma_offset, const uint8_t* images, const float* camera_blocks,
                             int cameras, int height, int width, int alpha_u8,
                             float min_transmittance, uint32_t* votes, void* stream);

/* K28a (csrc/octree_walk.hip, a twelfth mode of the K13 kernel): K24's votes with their second
 * moments, so that one walk gives a per-leaf colour variance as well as a mean.  No counterpart in
 * the reference.  Arguments, checks, pairs and the walk are ffn_octree_visible_votes', operation for
 * operation; only the write-back differs.  A visible pair adds to
 *     moments[l] = [sum_r, sum_g, sum_b, count, sq_r, sq_g, sq_b, 0]   (eight uint32, 32 bytes)
 * with sq_c = c * c of the pixel's byte, as FOUR 64-bit integer atomic adds of two fields each:
 * [sum_r, sum_g] and [sum_b, count], exactly K24's two words, then [sq_r, sq_g] and [sq_b, 0].
 * The first four fields are K24's votes bit for bit.  Exact, the same bits for the same pairs in
 * any order, in one call or split over many, as long as no carry crosses a field: a square is at
 * most 255^2 = 65025 and 65025 C < 2^32 holds for C <= 66051, so the caller keeps the cameras that
 * fold into one buffer AT OR BELOW 66051 (the sums and the count are then far below 2^32 too; the
 * eighth field stays 0).  The f32 colour (float)sum / (float)(255 count) of K24 is exact in both
 * operands only up to ffn_octree_carve_max_cameras() cameras.  moments (num_leaves,8) is 16-byte
 * aligned; the caller zeroes it or lets calls fold into it.  Limits and refusals as for
 * ffn_octree_visible_votes (cameras launched 65535 at a time; each bad argument refused by name
 * before any launch). */
int ffn_octree_visible_moments(const float* leaf_centers, int64_t num_leaves, float scale,
                               int depth, const int64_t* node_index, int64_t num_nodes,
                               const int64_t* leaf_index, const float* leaf_data, int stride,
                               int sigma_offset, const uint8_t* images, const float* camera_blocks,
                               int cameras, int height, int width, int alpha_u8,
                               float min_transmittance, uint32_t* moments, void* stream);

/* K25(csrc/occupancy.hip, beside K9a / K9b): the occupancy grid of K9 from an octree's leaves, the
 * leaves' boxes rasterised into the bits.  No counterpart in the reference.
 * leaf_index (num_leaves) sorted int64 ids, scale as for ffn_octree_leaf_geometry; center, box_min,
 * box_size are HOST pointers to 3 floats (the root cube's centre; the grid's box as for
 * ffn_occupancy_count).  Every operation below is one rounded f32 operation (no fma).
 *   Leaf: centre c and depth d by the chain of ffn_octree_leaf_geometry, h = scale 2^-d (exact);
 *     per axis lo = (c - h) + center, hi = (c + h) + center.
 *   Grid coordinate: f(x) = (x - box_min) * inv with inv = (float)G / box_size -- the very number
 *     the K9 lookup truncates for a sample at x.
 *   Cells: per axis the leaf covers the half-open interval [f(lo), f(hi)) of grid coordinates and
 *     marks every cell [i, i + 1) that meets it: i0 = clamp(floor(f(lo)), 0, G - 1),
 *     i1 = max(i0, clamp(ceil(f(hi)) - 1, 0, G - 1)).  A leaf with !(f(hi) > 0) or !(f(lo) < G) on
 *     any axis lies outside the box and marks nothing.  Half-open in GRID coordinates: a leaf
 *     whose + face falls on a cell boundary (every leaf, when the box is the root cube and G a
 *     power of two) does not mark the neighbour beyond it.
 *   Density: with leaf_data (num_leaves, stride) given and use_threshold != 0 a leaf whose
 *     leaf_data[l, sigma_offset] <= sigma_threshold marks nothing; a NaN density marks.
 *     leaf_data NULL: every leaf marks (use_threshold != 0 is then refused).
 * Guarantee: f is monotone, so every f32 point p with f(lo) <= f(p) < f(hi) on all three axes, for
 * a leaf that marks, is reported occupied by the K9 lookup (ffn_occupancy_count / _compact, the
 * fused render).  The points of a leaf left out are within rounding of a + face; `dilate` is the
 * slack for those and for what the tree itself missed.
 * Work: one thread per leaf plans (index ranges; ny nz rows, 0 for a leaf that marks nothing), the
 * row counts are scanned into offsets (tiles of 4096 leaves round the K9d scan; one read-back of
 * their sum, refused from 2^31 - 1 on: "too many rows"), then one thread per row ORs the run [(iz G + iy) G + ix0 .. + ix1] into the
 * grid, one 32-bit mask and at most one integer atomic OR per touched word (<= G / 32 + 2 words a
 * thread).  Integer OR: the same bits in any order, on every call.
 * accumulate == 0: bits (ceil(G^3 / 32) words) is zeroed first.  accumulate != 0: the cells are
 * ORed into what bits holds, so leaf subsets or several trees folded over several calls give the
 * bits of one call -- also with dilation, which distributes over OR.
 * dilate = n >= 0: n passes of the 26-neighbourhood dilation of ffn_occupancy_build over what
 * THIS call rasterised; the result lands in bits for every n.  scratch_bits: NULL for n = 0, else
 * as many words as bits, twice as many with accumulate.
 * Workspace (device): plan 4 int32 per leaf, 16-byte aligned; row_offsets 1 int32 per leaf;
 * tile_sums ceil(num_leaves / 4096) int32; total one int64.  Refused by name before any launch:
 * resolution outside 1 .. 1024, num_leaves outside 1 .. 2^31 - 1, a null pointer, scale or
 * box_size not finite and positive, center or box_min not finite, stride < 1 or sigma_offset
 * outside 0 .. stride - 1, a threshold that is NaN or has no leaf_data, dilate < 0, dilation
 * without scratch. */
int ffn_occupancy_from_octree(const int64_t* leaf_index, int64_t num_leaves, float scale,
                              const float* center, const float* leaf_data, int stride,
                              int sigma_offset, float sigma_threshold, int use_threshold,
                              const float* box_min, const float* box_size, int resolution,
                              int accumulate, int dilate, int32_t* plan, int32_t* row_offsets,
                              int32_t* tile_sums, int64_t* total, uint32_t* scratch_bits,
                              uint32_t* bits, void* stream);

/* K26 (csrc/octree_walk.hip, a sibling of the K13 kernel that shares its device functions): a ray's
 * focus samples drawn from the compositing weights of the octree itself, merged with its uniform
 * samples.  Stands where the reference probes a coarse model at n_focus points per ray
 * (ray_sampler.py:234-269, _determine_cdf) and inverts the CDF of the blend weights
 * (ray_sampler.py:380-392); here the distribution is the tree's own piecewise weights.
 * starts, directions (num_rays_total,3), near_far (2,num_rays_total) as K1 writes them; ray_index
 * (num_rays) int64 ids (an id outside 0 .. num_rays_total - 1 leaves its row unwritten); center_x/y/z
 * the root cube's centre, scale .. num_leaves as for ffn_octree_walk; leaf_rows / stride /
 * sigma_offset as leaf_data for ffn_octree_leaf_weights (only the density is read: stride 4 and
 * offset 3 on plain rows, the K18a device stride and offset 0 on SH rows).  u (num_rays,n_focus) in
 * [0,1], ASCENDING in every row by contract (not checked).  t_uniform: row r's n_uniform ascending
 * uniform samples at t_uniform + r * uniform_stride (K2a's output), or NULL with n_uniform == 0.
 * t_out (num_rays, S), S = n_uniform + n_focus, a buffer of its own; mass_out (num_rays) or NULL.
 * One lane per batch ray r with id i = ray_index[r]; every operation one rounded f32 operation (the
 * file is compiled with -ffp-contract=off):
 *     o = starts[i] - center;  d = directions[i];  near, far = near_far[0,i], near_far[1,i]
 *     norm = sqrtf(dx*dx + dy*dy + dz*dz);  T = 1, c = 0
 *     for every region of the K13 walk that is a leaf, in walk order (t_entry, t_exit its crossings):
 *         t0 = fmaxf(t_entry, near);  t1 = fminf(t_exit, far);  taken iff t1 > t0
 *         L = (t1 - t0) * norm;  sigma = fmaxf(leaf_rows[leaf, sigma_offset], 0)   (NaN counts as 0)
 *         a = 1 - expf(-(sigma * L));  w = T * a;  c_next = c + w;  T = T * (1 - a)
 *     the walk ends at the first region whose t_exit >= far, and once T == 0 exactly
 * Phase 0 walks once: M = c after the last taken leaf.  Phase 1 runs the same code again, so c
 * repeats bit for bit, with a pointer j into the row's targets:
 *     y_j = u_j * M;  in a taken leaf with w > 0, while j < n_focus and y_j < c_next:
 *         f = (y_j - c) / w;  t = fminf(fmaxf(t0 + f * (t1 - t0), t0), t1)
 *         t = fmaxf(t, last emitted);  emit;  ++j
 *     after the walk every remaining target (u == 1, rounding, a NaN, a u out of order) is emitted as
 *     the t1 of the last taken leaf with w > 0 (the end of the mass: every taken leaf after it weighs
 *     exactly 0, so the value does not depend on where the walk ends), through the same maximum
 * The uniform fall-back t_j = near + u_j * (far - near) is what a ray emits instead when M > 0 does
 * not hold or M < min_mass, when it misses the cube or K13 cannot follow it (NaN directions), and
 * when near < far does not hold -- then t_j = near.  mass_out[r] = M (0 for a ray that did not walk).
 * Merge: the lane's ascending emits and the row's uniform samples by two pointers, a uniform sample
 * first where the two are equal: as values and bits row r of t_out is sort(cat(uniform, focus)).
 * A row of u that breaks the contract may give a poorly ordered row; it never gives a write outside
 * the row or an unbounded loop: a lane emits exactly n_focus values and moves each uniform sample
 * once, and its trips are bounded by two K13 walks plus S.  No LDS, no atomics, no S <= 256 limit as
 * in K2d; a row depends on its own ray alone, so the same inputs give the same bits in any batch.
 * Refused by name before any launch: n_focus < 1, n_uniform < 0, a null t_uniform with
 * n_uniform > 0, uniform_stride < n_uniform, depth outside 1 .. ffn_octree_max_depth(), num_leaves
 * < 1, stride < 1 or sigma_offset outside 0 .. stride - 1, a NaN or negative min_mass,
 * num_rays * S >= 2^31, a NaN centre, a null pointer, t_out overlapping t_uniform.  num_rays == 0
 * returns 0 at once. */
int ffn_octree_focus_sample(const float* starts, const float* directions, const float* near_far,
                            int64_t num_rays_total, const int64_t* ray_index, int num_rays,
                            float center_x, float center_y, float center_z, float scale, int depth,
                            const int64_t* node_index, int64_t num_nodes,
                            const int64_t* leaf_index, int64_t num_leaves, const float* leaf_rows,
                            int stride, int sigma_offset, const float* u, int n_focus,
                            const float* t_uniform, int uniform_stride, int n_uniform,
                            float min_mass, float* t_out, float* mass_out, void* stream);

/* ------------------------------------------------------------------------------------
 * K30  a coloured triangle mesh from an octree (csrc/octree_mesh.hip).  No counterpart in the
 * reference, which hands its leaf cubes to scenepic.
 *
 * n = 2^(depth-1) finest cells per axis, side = 2 scale / n.  Vertices sit on the lattice of cell
 * corners c = (i, j, k), 0 <= i, j, k <= n.  The eight samples of a corner are the cells
 * c - 1 + (dx, dy, dz) with bit b = 4 dx + 2 dy + dz (the child digit); mask has bit b set when that
 * cell is solid; cells in empty space or outside the cube are not.  A corner is a vertex when mask is
 * neither 0 nor 255; its key is (i (n+1) + j)(n+1) + k (int64).  Integers wherever the contract is
 * integer, f32 sums in a fixed order (the file is compiled with -ffp-contract=off), no float
 * atomics: the same bits on every call.  Every index read from an input array is held against its
 * range before use.  Bad shapes and null pointers are refused by name before any launch. */
int ffn_octree_mesh_max_depth(void);   /* 21: the deepest tree whose keys an int64 holds */

/* K30a.  Per leaf the opacity over one FINEST side and the flag alpha > threshold (strict):
 *   solid_in (num_leaves) uint8 given: alpha = solid_in ? 1 : 0 (leaf_rows is not read);
 *   else leaf_rows NULL: alpha = 1;
 *   else sigma = leaf_rows[l * stride + sigma_offset], alpha = -expm1f(-(sigma * side)), 0 for a
 *   negative or NaN sigma.
 * 0 < threshold < 1; side finite and positive. */
int ffn_octree_mesh_solid(const float* leaf_rows, int stride, int sigma_offset,
                          const uint8_t* solid_in, int64_t num_leaves, float side, float threshold,
                          uint8_t* solid, float* alpha, void* stream);

/* K30b.  Only corners on the closed surface of a solid leaf can be vertices; a leaf of k =
 * 2^(depth-1-level) cells a side has (k+1)^3 - (k-1)^3 = 6 k^2 + 2 of them.  cand_offsets
 * (num_leaves + 1) int64 is the exclusive scan of that count over the leaves (0 for a leaf that is
 * not solid), made by the caller.  This call handles the candidates first .. first + count - 1, one
 * thread each: the leaf by a binary search of cand_offsets, the corner by a closed form of the
 * remainder (the plane i = 0, the plane i = k, then per i the ring: row j = 0, row j = k, then per j
 * the ends k = 0 and k = k), the eight cells by integer coordinate from the root down with the
 * binary searches of ffn_octree_neighbors (a leaf met on the way covers the cell, the root included;
 * an id in neither index is empty).  A candidate is kept when its mask is active and the first solid
 * sample in bit order lies in the thread's own leaf: every vertex exactly once.  The kept ones in
 * candidate order (the K12b/c scan and a stable scatter): keys (int64), masks (uint8) and samples
 * (.,8) int32 (the eight leaf numbers, -1 for empty), *total (device) of them, in arrays of count
 * entries; the *_scratch arrays have the same shapes.  flags / offsets / tile_sums as for
 * ffn_octree_surface_points.  A candidate whose leaf, id or number does not fit depth is dropped.
 * 1 <= depth <= ffn_octree_mesh_max_depth(); 1 <= count <= ffn_octree_max_points(). */
int ffn_octree_mesh_candidates(const int64_t* node_index, int64_t num_nodes,
                               const int64_t* leaf_index, int64_t num_leaves, const uint8_t* solid,
                               const int64_t* cand_offsets, int64_t first, int64_t count, int depth,
                               uint8_t* flags, int* offsets, int* tile_sums, int64_t* keys_scratch,
                               uint8_t* masks_scratch, int32_t* samples_scratch, int64_t* keys,
                               uint8_t* masks, int32_t* samples, int* total, void* stream);

/* K30c.  Per vertex (keys ascending: the caller sorts them and permutes masks and samples), with
 * a_b = alpha[samples[v, b]] (0 for -1 or a number outside 0 .. num_leaves - 1), p_b = (dx, dy, dz) -
 * 0.5 and every operation one rounded f32 operation:
 *   offset: 0 without surface_nets.  With it, over the 12 sample pairs that differ in one bit -- x
 *     pairs first, then y, then z, within an axis by ascending lower b -- a pair whose mask bits
 *     differ contributes p_b0 + t e_ax, t = (threshold - a_b0) / (a_b1 - a_b0); offset = the sum of
 *     the contributions in that order, divided by their count.
 *   vertices[v] = center + (((float)c - n / 2) + offset) * side, side = 2 scale / n.
 *   corners[v] = c (int32).
 *   normals[v] = -g / |g|, g = sum_b a_b * 2 p_b in bit order, |g| = sqrtf((gx gx + gy gy) + gz gz);
 *     (0, 0, 0) when |g| is 0.
 *   colors[v] = the sum over the solid samples, in bit order, of the three columns
 *     leaf_rows[l * stride + color_offset + c * color_step], divided by their number; with color_sh
 *     != 0 a column k is first turned into 1 / (1 + expf(-(k * Y_00))), Y_00 = 0.28209479, the
 *     band-0 colour of an SH leaf (plain rows: offset 0, step 1; K18a device rows of B bases: offset
 *     1, step B).  leaf_rows and colors are NULL together: no colours. */
int ffn_octree_mesh_vertices(const int64_t* keys, const uint8_t* masks, const int32_t* samples,
                             int64_t num_vertices, const float* alpha, const float* leaf_rows,
                             int64_t num_leaves, int stride, int color_offset, int color_step,
                             int color_sh, int depth, float scale, float center_x, float center_y,
                             float center_z, float threshold, int surface_nets, float* vertices,
                             float* colors, float* normals, int32_t* corners, void* stream);

/* K30d, in two calls around one read-back of the quad count.  Vertex v owns the quad across axis ax
 * (x, y, z) when cell c (bit 7) and cell c - e_ax (bit 7 ^ (4 >> ax)) differ in solidity.
 * ffn_octree_mesh_face_flags: flags / offsets (3 num_vertices each, slot 3 v + ax) and tile_sums
 * (ffn_octree_scan_tiles(3 num_vertices)); *total (device) = the number of quads.
 * ffn_octree_mesh_faces: with those flags and offsets and num_quads = *total, quad o writes the rows
 * 2 o and 2 o + 1 of triangles (2 num_quads, 3) int32: its corners q = c, c + e_u, c + e_u + e_v,
 * c + e_v, (u, v) the next two axes in cyclic order (normal +ax), as written when cell c - e_ax is the
 * solid one and as c, c + e_v, c + e_u + e_v, c + e_u when cell c is, so that the normal points from
 * solid to empty; triangles (q0, q1, q2) and (q0, q2, q3).  The three other corners are found by a
 * binary search of their keys in keys (ascending).  A key that is not found, or an offset outside
 * 0 .. num_quads - 1, is an error: that quad is not written, missing (one int32 on the device) is
 * set, and the call -- which waits for the stream to read it -- returns non-zero.
 * 3 num_vertices <= ffn_octree_max_points(). */
int ffn_octree_mesh_face_flags(const uint8_t* masks, int64_t num_vertices, uint8_t* flags,
                               int* offsets, int* tile_sums, int* total, void* stream);
int ffn_octree_mesh_faces(const int64_t* keys, const uint8_t* masks, const uint8_t* flags,
                          const int* offsets, int64_t num_vertices, int depth, int64_t num_quads,
                          int32_t* triangles, int32_t* missing, void* stream);

/* ------------------------------------------------------------------------------------
 * K31  a z-buffer rasteriser for triangle meshes (csrc/mesh_raster.hip).  No counterpart in the
 * reference.  vertices (num_vertices,3) f32, triangles (num_triangles,3) i32 (an id is clamped into
 * 0 .. num_vertices - 1 as in K22: a bad one reads a wrong vertex, not foreign memory), an image of
 * width x height pixels, pixel (px, py) being the ray through the integer coordinates (px, py).
 * Coverage is decided on integers; every float operation is one rounded f32 operation in the order
 * written (no fma; / and sqrtf are IEEE operations): the same inputs give the same bits on every call
 * and for any split into chunks.  There is NO near-plane clipping: a triangle that crosses w = 0 or
 * leaves the guard band is not drawn, and its status says so.
 * 1 <= width, height <= 16384; 1 <= num_vertices, num_triangles <= (2^31 - 1) / 3; bad shapes and
 * null pointers are refused by name before any launch.
 *
 * K31a, one thread per triangle.  proj: 12 floats in HOST memory, the 3x4 row-major matrix of K23.
 *   per vertex p: x = ((P00 p.x + P01 p.y) + P02 p.z) + P03, likewise y (row 1) and w (row 2);
 *                 sx = x / w, sy = y / w
 *   status[f]: 1 behind: all three w <= 0;  else 2 clipped: some !(w > 0) or some
 *              !(fabsf(s) <= 16384.0f) (NaN and infinities fall here);  else
 *              X = (int)rintf(sx * 256.0f), Y = (int)rintf(sy * 256.0f) (24.8 fixed point) and
 *              A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) in int64: 3 degenerate when A == 0;  else the box
 *              x0 = max(0, ceil(minX / 256)), x1 = min(width - 1, floor(maxX / 256)), likewise y
 *              (integer floor division): 4 off-image when it is empty;  else 0 drawn.
 *   counts[f] (int64) = (x1-x0+1)(y1-y0+1) when drawn, 0 otherwise.
 *   record[f] = 16 int32, 16-byte aligned: X0 Y0 X1 Y1 X2 Y2, the bits of w0 w1 w2, x0 y0 x1 y1, three
 *              zeros.  X and Y are 0 for status 1 and 2; the box is 0 0 -1 -1 unless drawn.
 *
 * K31b, one thread per box pixel s = first .. first + count - 1, 1 <= count <= ffn_octree_max_points().
 * offsets (num_triangles + 1) int64: the exclusive scan of counts, made by the caller.
 *   f: offsets[f] <= s < offsets[f + 1];  k = s - offsets[f];  bw = x1 - x0 + 1;
 *   (px, py) = (x0 + k % bw, y0 + k / bw);  Q = (256 px, 256 py);  sgn = sign(A)
 *   E_i = sgn [(X_k - X_j)(Q_y - Y_j) - (Y_k - Y_j)(Q_x - X_j)], (j, k) = (i+1, i+2) mod 3, in int64
 *   covered iff E_0, E_1, E_2 >= 0: inclusive and two-sided, so a pixel centre on a shared edge
 *   belongs to both triangles and there are no cracks
 *   l_i = (float)E_i / (float)|A|;  q_i = l_i / w_i;  inv_w = (q0 + q1) + q2;  depth_w = 1.0f / inv_w
 *   skipped unless depth_w is finite and > 0;  key = (uint64)bits(depth_w) << 32 | f
 *   zbuf[py width + px] = min(itself, key), an unsigned 64-bit atomic behind a plain load that skips
 *   it when the pixel already holds no more.  zbuf (height width) uint64, all ones where empty (the
 *   caller fills it).  The minimum does not depend on the order: the nearest depth_w wins, the lower
 *   triangle id among equal ones.  A pixel outside the image is never written, whatever the record.
 *
 * K31c, one thread per pixel.  Exactly one of vertex_colors (num_vertices,3) f32 and uvs
 * (num_vertices,2) f32 + texture (tex_height, tex_width, tex_channels) u8 (K22's texture and limits,
 * row index growing with v) is non-null.  eye, background: 3 floats each in HOST memory.
 *   zbuf all ones: color = background, alpha = 0, depth = 0, ids = -1
 *   else f = the low word; E_i, l_i, q_i, depth_w as in K31b (the same bits); b_i = q_i * depth_w
 *   color = (c0 b0 + c1 b1) + c2 b2 per channel, or (u, v) interpolated the same way and looked up
 *   as in ffn_mesh_sample (bilinear, / 255);  alpha = 1;  ids = f
 *   p = (v0 b0 + v1 b1) + v2 b2 per component;  d = p - eye;
 *   depth = sqrtf((d.x d.x + d.y d.y) + d.z d.z): the distance from the eye, OcTree.render's t
 * color (height width, 3), alpha, depth (height width) f32, ids (height width) int32.  No atomics. */
int ffn_mesh_raster_setup(const float* vertices, int64_t num_vertices, const int32_t* triangles,
                          int64_t num_triangles, const float* proj, int width, int height,
                          int32_t* record, uint8_t* status, int64_t* counts, void* stream);
int ffn_mesh_raster_draw(const int32_t* record, const int64_t* offsets, int64_t num_triangles,
                         int64_t first, int64_t count, int width, int height, uint64_t* zbuf,
                         void* stream);
int ffn_mesh_raster_resolve(const uint64_t* zbuf, const int32_t* record, const float* vertices,
                            int64_t num_vertices, const int32_t* triangles, int64_t num_triangles,
                            const float* vertex_colors, const float* uvs, const uint8_t* texture,
                            int tex_height, int tex_width, int tex_channels, const float* eye,
                            const float* background, int width, int height, float* color,
                            float* alpha, float* depth, int32_t* ids, void* stream);

/* ------------------------------------------------------------------------------------
 * K32  the adjoint of K31c's colour interpolation (csrc/mesh_raster_grad.hip).  No counterpart in
 * the reference.  K31's colour is (c_v0 b0 + c_v1 b1) + c_v2 b2 with b_i from the geometry alone:
 * the image is a linear map of the vertex colours, and these two launches are its transpose, for
 * the per-vertex colours only (the textured path's transpose is K33, the geometry has no gradient).  No
 * float atomics and no LDS; every float operation is one rounded f32 operation in the order
 * written: the same inputs give the same bits on every call.  Limits as in K31: 1 <= width, height
 * <= 16384; 1 <= num_vertices, num_triangles <= (2^31 - 1) / 3; bad shapes and null pointers are
 * refused by name before any launch.
 *
 * K32a, one wavefront (64 lanes) per triangle f.  record (num_triangles,16) int32, 16-byte aligned,
 * from K31a; ids (height width) int32 from K31c; d_color (height width,3) f32.
 *   the box x0 y0 x1 y1 of record[f];  bw = x1 - x0 + 1;  n = bw (y1 - y0 + 1)
 *   a box that is empty, not inside the image, or has n > 2^28 contributes nothing: a pixel outside
 *   the image is never read, whatever the record
 *   box pixel k = 0 .. n - 1 is (px, py) = (x0 + k % bw, y0 + k / bw), p = py width + px; it is
 *   SELECTED iff ids[p] == f.  ids is compared and never used as an index.  A pixel that is not
 *   selected is skipped by selection, not multiplied by zero: d_color[p] is not read
 *   a selected pixel: E_i, l_i, q_i, depth_w as in K31b (the same bits); b_i = q_i * depth_w;
 *     t[3 i + j] = b_i * d_color[p][j] (one rounded product each), t[9 + i] = b_i
 *   segment s holds k = 64 s .. 64 s + 63, lane l the pixel k = 64 s + l; a lane that is not selected
 *   or past n holds +0.0f; the 64 lane values are folded by x += shfl_xor(x, off), off = 32, 16, 8,
 *   4, 2, 1 -- an IEEE add commutes bit for bit, so this is the fold of halves a[:h] + a[h:2h],
 *   h = 32 .. 1;  acc = 0.0f, then acc = acc + segment_s for s = 0, 1, .. in order
 * face_sums (num_triangles,12) f32 = the twelve acc.  Every row is written; the row of a triangle
 * that is not drawn, or wins no pixel, is +0.
 *
 * K32b, one thread per vertex v.  corner_order (3 num_triangles) int32: the corners 3 f + i stably
 * sorted by vertex id; vertex_starts (num_vertices + 1) int32: the rows of v are
 * corner_order[vertex_starts[v] .. vertex_starts[v + 1] - 1] (CSR; the range is clamped into the
 * array).  From 0.0f and in that order, for the corner 3 f + i:
 *   g[j] = g[j] + face_sums[f][3 i + j], j = 0 .. 2;  w = w + face_sums[f][9 + i]
 * a corner outside 0 .. 3 num_triangles - 1 is skipped.  grad (num_vertices,3) = g and weight
 * (num_vertices) = w, or with accumulate != 0 out = out + value, one add each. */
int ffn_mesh_raster_face_sums(const int32_t* record, const int32_t* ids, const float* d_color,
                              int64_t num_triangles, int width, int height, float* face_sums,
                              void* stream);
int ffn_mesh_vertex_gather(const float* face_sums, const int32_t* corner_order,
                           const int32_t* vertex_starts, int64_t num_triangles,
                           int64_t num_vertices, float* grad, float* weight, int accumulate,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * K33  K31c's textured colour as a sparse matrix and its two products (csrc/mesh_texture.hip).  No
 * counterpart in the reference.  K31c's textured colour is a bilinear blend of four texels whose
 * indices and weights come from the geometry, the camera and the UVs alone: the image is a linear
 * map of the texture with four entries (taps) per covered pixel.  K33a makes the taps, K33b applies
 * them to a float texture and K33c their transpose to an image.  No float atomics and no LDS; every
 * float operation is one rounded f32 operation in the order written: the same inputs give the same
 * bits on every call.  Every index read from an input array is held against its range before it is
 * used: foreign ids, taps or orders give wrong numbers, never an access outside the buffers.
 * Limits: 1 <= width, height <= 16384 and 1 <= num_pixels <= 2^28; 1 <= num_vertices,
 * num_triangles <= (2^31 - 1) / 3; 1 <= tex_height, tex_width <= 2^24 and num_texels =
 * tex_height tex_width <= (2^31 - 1) / 3; bad shapes and null pointers are refused by name before
 * any launch.  tap_texel and tap_weight are 16-byte aligned.
 *
 * K33a, one thread per pixel p.  record (num_triangles,16) int32, 16-byte aligned, from K31a; ids
 * (height width) int32 from K31c; triangles (num_triangles,3) int32; uvs (num_vertices,2) f32.
 *   f = ids[p] outside 0 .. num_triangles - 1: the pixel is uncovered, tap_texel[p][0..3] = -1 and
 *   tap_weight[p][0..3] = +0
 *   else E_i, l_i, q_i, depth_w as in K31b (the same bits); b_i = q_i * depth_w; the vertex ids
 *   clamped into 0 .. num_vertices - 1; u = (u0 b0 + u1 b1) + u2 b2, v likewise; then the index and
 *   weight arithmetic of ffn_mesh_sample's lookup: col = u tex_width, row = v tex_height,
 *   fj = floorf(col), fi = floorf(row), dj = col - fj, di = row - fi (before clamping),
 *   j0 = clamp(fj), j1 = clamp(fj + 1) into 0 .. tex_width - 1 (as floats; NaN clamps to 0), i0 and
 *   i1 likewise, w00 = (1 - di)(1 - dj), w01 = (1 - di) dj, w10 = di (1 - dj), w11 = di dj
 * tap_texel (height width,4) int32 = i tex_width + j in the order 00, 01, 10, 11 (i0 j0, i0 j1,
 * i1 j0, i1 j1); tap_weight (height width,4) f32 the weights in that order.
 *
 * K33b, one thread per pixel p.  texture (num_texels,3) f32, plain floats (no / 255); background: 3
 * floats in HOST memory.
 *   tap_texel[p][0] < 0: color[p] = background, alpha[p] = 0
 *   else term_k = tap_weight[p][k] * texture[tap_texel[p][k]][ch], or +0.0f by selection when the
 *   texel is outside 0 .. num_texels - 1 (it is not read);
 *   color[p][ch] = ((term_0 + term_1) + term_2) + term_3;  alpha[p] = 1
 * color (num_pixels,3), alpha (num_pixels) f32.
 *
 * K33c, one thread per texel t.  sorted_texels (4 num_pixels) int32, ascending, and tap_order
 * (4 num_pixels) int32: the tap slots 4 p + k stably sorted by tap_texel, made by the caller (the -1
 * slots sort first and belong to no texel).  d_color (num_pixels,3) f32.
 *   the row of t is [lower_bound(t), lower_bound(t + 1)) of sorted_texels (binary searches; both
 *   ends lie in 0 .. 4 num_pixels whatever the array holds).  From 0.0f and in that order, for the
 *   slot s = tap_order[at] and w = tap_weight[s]:
 *     skipped by selection, not multiplied by zero, when s is outside 0 .. 4 num_pixels - 1 or
 *     !(w > 0.0f): a NaN weight, or a zero weight over a non-finite d_color, reaches no texel
 *     else g[ch] = g[ch] + w * d_color[s / 4][ch], ch = 0 .. 2;  wsum = wsum + w
 * grad (num_texels,3) = g and weight (num_texels) = wsum, or with accumulate != 0 out = out +
 * value, one add each.  The loop is linear in the length of the row. */
int ffn_mesh_texture_taps(const int32_t* record, const int32_t* ids, const int32_t* triangles,
                          int64_t num_triangles, const float* uvs, int64_t num_vertices,
                          int tex_height, int tex_width, int width, int height,
                          int32_t* tap_texel, float* tap_weight, void* stream);
int ffn_mesh_texture_gather(const int32_t* tap_texel, const float* tap_weight,
                            const float* texture, int64_t num_texels, const float* background,
                            int64_t num_pixels, float* color, float* alpha, void* stream);
int ffn_mesh_texture_grad(const int32_t* sorted_texels, const int32_t* tap_order,
                          const float* tap_weight, const float* d_color, int64_t num_pixels,
                          int64_t num_texels, float* grad, float* weight, int accumulate,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * K34  analytic edge antialiasing behind K31, its transposes in the image and in the vertex
 * positions, and a smoothness term for vertex displacements (csrc/mesh_aa.hip).  No counterpart in
 * the reference; the method is nvdiffrast's (Laine et al. 2020).  K31's image is piecewise constant in
 * the positions.  Here two 4-neighbour pixels whose ids differ are blended by how far the silhouette
 * edge between their centres reaches, a smooth function of the edge's two vertices.  Decisions are
 * made on integers; every float operation is one rounded f32 operation in the order written (no fma;
 * / is the IEEE division; -x is the sign flip); no float atomics and no LDS: the same inputs give the
 * same bits on every call.  Every index read from an input array is held against its range before it
 * is used.  Limits as in K31: 1 <= width, height <= 16384, and width height <= 2^28 (the 4 width
 * height entries index in an int32); 1 <= num_vertices, num_triangles <= (2^31 - 1) / 3; bad shapes
 * and null pointers are refused by name before any launch.  record is 16-byte, zbuf and entry_grad
 * are 8-byte aligned.
 *
 * Notation.  Pixel p = py width + px, centres at integer coordinates.  A PAIR is two 4-neighbours:
 * slot (p, axis) pairs p with q = p + 1 (axis 0, only when px + 1 < width) or q = p + width (axis 1,
 * only when py + 1 < height).  record (num_triangles,16) from K31a, zbuf (height width) uint64 from
 * K31b (all ones where empty), ids (height width) int32 from K31c.  opposite (3 num_triangles) int32:
 * for corner 3 f + i the vertex across edge i of triangle f (edge i joins the corners j = (i+1) mod 3
 * and k = (i+2) mod 3, K31b's numbering) when exactly one other triangle shares the undirected edge,
 * else -1 (boundary and non-manifold edges).  proj: 12 floats in HOST memory, as in K31a.
 *
 * The pair decision of (p, q), the same function in every kernel:
 *   inactive when ids[p] == ids[q].  near = q when zbuf[q] < zbuf[p] (unsigned), else p; far the other.
 *   attempt(near -> far); when it fails and ids[far] >= 0, attempt(far -> near); the first success
 *   decides; with none the pair is inactive.
 *   attempt(a -> b): f = ids[a]; fails when f is outside 0 .. num_triangles - 1.  X, Y, A, sgn =
 *     sign(A) from record[f]; fails when A == 0.  E_i(Q_a), E_i(Q_b), i = 0 .. 2, as in K31b (int64,
 *     sgn applied), Q = 256 (x, y) of the pixel.  Fails when some E_i(Q_a) < 0, and when no
 *     E_i(Q_b) < 0.  For every i with E_i(Q_b) < 0: D_i = E_i(Q_a) - E_i(Q_b) (int64, > 0),
 *     alpha_i = (float)E_i(Q_a) / (float)D_i.  i* = the smallest alpha_i, the lowest i among equal
 *     ones (a later i replaces the best only when its alpha is less).
 *     o = opposite[3 f + i*].  o < 0 passes.  Else o is clamped to num_vertices - 1 and projected as
 *     in K31a: x, y, w, sx = x / w, sy = y / w; fails when !(w > 0) or !(fabsf(sx) <= 16384.0f) or
 *     !(fabsf(sy) <= 16384.0f); O = ((int)rintf(sx * 256.0f), (int)rintf(sy * 256.0f));
 *     side = sgn [(X_k - X_j)(O_y - Y_j) - (Y_k - Y_j)(O_x - X_j)] in int64, E_i* at O; passes iff
 *     side >= 0 (the neighbour folds back onto f's own side), fails otherwise (an interior edge).
 *   On success alpha = alpha_i*, D = D_i*;  s = alpha - 0.5f;  s >= 0: target = b, source = a (f
 *   reaches past the midpoint into b's pixel); else target = a, source = b;  m = fabsf(s).
 *
 * K34a, one thread per pixel p.  The channels c are r, g, b of color (height width,3) and alpha
 * (height width), K31c's.  out_c = in[p]_c; then for the pairs left (slot (p - 1, 0)), right
 * (slot (p, 0)), up (slot (p - width, 1)), down (slot (p, 1)) that exist, in that order, each active
 * one whose target is p:  out_c = out_c + m * (in[source]_c - in[p]_c).  out_color (height width,3),
 * out_alpha (height width).  A pixel in no active pair is copied bit for bit.
 *
 * K34b, one thread per pixel p.  g_color, g_alpha: the gradient in K34a's outputs.
 *   image: d_c = g[p]_c; the same four pairs in the same order; an active pair with target p:
 *   d_c = d_c - m * g[p]_c; with source p: d_c = d_c + m * g[target]_c.  A g at a pixel that is
 *   neither p nor the target of one of p's pairs is not read.  d_color (height width,3), d_alpha.
 *   entries: the thread owns the slots (p, 0) and (p, 1); slot (p, axis) has the entries
 *   e = 4 p + 2 axis + {0, 1}.  Inactive or non-existent: entry_vertex[e] = num_vertices,
 *   entry_grad[e] = (+0, +0), both entries.  Active, with t = target:
 *     delta_c = in[source]_c - in[t]_c;
 *     G = ((g[t]_r delta_r + g[t]_g delta_g) + g[t]_b delta_b) + g[t]_a delta_a;
 *     d_alpha_pair = s >= 0 ? G : -G;   V_j, V_k = (float)(X, Y) of the corners j, k of f;
 *     C = ((float)Q_a.x + alpha * (float)(Q_b.x - Q_a.x), likewise y);  c_j = C - V_j, c_k = C - V_k;
 *     r = (sgn > 0 ? d_alpha_pair : -d_alpha_pair) / (float)D;   r256 = 256.0f * r;
 *     entry 0: vertex triangles[f][k], (r256 * c_j.y, -(r256 * c_j.x));
 *     entry 1: vertex triangles[f][j], (-(r256 * c_k.y), r256 * c_k.x);  ids clamped as in K31.
 *   These are d loss / d (sx, sy) of the two vertices: alpha's derivative in V_k is
 *   (sgn / D)(c_j.y, -c_j.x), in V_j it is -(sgn / D)(c_k.y, -c_k.x), and the snap V = 256 s is
 *   passed straight through.  entry_vertex (4 height width) int32, entry_grad (4 height width,2)
 *   f32; every entry is written on every call.
 *
 * K34c, one thread per vertex v.  sorted_vertex (4 num_pixels) int32: entry_vertex stably sorted,
 * ascending; order (4 num_pixels) int32: the entries in that order; both made by the caller (the
 * sentinel num_vertices sorts behind every vertex and belongs to none).  The run of v is
 * [lower_bound(v), lower_bound(v + 1)) of sorted_vertex (binary searches; both ends lie in
 * 0 .. 4 num_pixels whatever the array holds).  From 0.0f and in that order, e = order[at]:
 * gx = gx + entry_grad[e][0], gy = gy + entry_grad[e][1]; an e outside 0 .. 4 num_pixels - 1 is
 * skipped.  v projected as in K31a to x, y, w, sx = x / w, sy = y / w.  !(w > 0): the row is +0.
 * Else, per component c of the position, with P the rows of proj:
 *   grad[v][c] = ((gx * (P0c - sx * P2c)) + (gy * (P1c - sy * P2c))) / w
 * grad (num_vertices,3) = the row, or with accumulate != 0 out = out + row, one add each.  The loop
 * is linear in the run: a vertex on a long silhouette is one thread's loop, K33c's limit.
 *
 * K34d, one thread per vertex v.  values (num_vertices,3) f32; neighbor_starts (num_vertices + 1)
 * int32 and neighbors (num_neighbors) int32: a CSR with every undirected edge listed once per end
 * (the range of a row is clamped into the array).  From 0.0f and in the row's order, per component:
 * acc_c = acc_c + (x[v]_c - x[n]_c); an n outside 0 .. num_vertices - 1 is skipped.
 * out[v]_c = scale * acc_c, or with accumulate != 0 out = out + scale * acc.  With scale = 1 this
 * is the gradient of 1/2 sum_edges |x_i - x_j|^2.  0 <= num_neighbors < 2^31. */
int ffn_mesh_aa_forward(const int32_t* record, const uint64_t* zbuf, const int32_t* ids,
                        const int32_t* opposite, const float* vertices, int64_t num_vertices,
                        int64_t num_triangles, const float* proj, const float* color,
                        const float* alpha, int width, int height, float* out_color,
                        float* out_alpha, void* stream);
int ffn_mesh_aa_backward(const int32_t* record, const uint64_t* zbuf, const int32_t* ids,
                         const int32_t* opposite, const float* vertices, int64_t num_vertices,
                         const int32_t* triangles, int64_t num_triangles, const float* proj,
                         const float* color, const float* alpha, const float* g_color,
                         const float* g_alpha, int width, int height, float* d_color,
                         float* d_alpha, int32_t* entry_vertex, float* entry_grad, void* stream);
int ffn_mesh_aa_vertex_grad(const int32_t* sorted_vertex, const int32_t* order,
                            const float* entry_grad, int64_t num_pixels, const float* vertices,
                            int64_t num_vertices, const float* proj, float* grad, int accumulate,
                            void* stream);
int ffn_mesh_laplacian(const float* values, const int32_t* neighbor_starts,
                       const int32_t* neighbors, int64_t num_vertices, int64_t num_neighbors,
                       float scale, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K35  the interior half of the geometry gradient behind K31: colour through the barycentric
 * weights (csrc/mesh_interp_grad.hip).  No counterpart in the reference; the method is nvdiffrast's
 * (Laine et al. 2020).  K34 gives a gradient to the vertices of silhouette edges; here every pixel a
 * triangle wins gives one to the triangle's three corners, for the per-vertex colours only (the
 * textured path has none).  Which triangle wins a pixel is held fixed and the snap to 1/256 pixel is
 * passed straight through.  The edge functions are int64; every float operation is one rounded f32
 * operation in the order written (no fma; / is the IEEE division; -x is the sign flip); no float
 * atomics and no LDS: the same inputs give the same bits on every call.  Every index read from an
 * input array is held against its range before it is used.  Limits as in K31: 1 <= width, height <=
 * 16384; 1 <= num_vertices, num_triangles <= (2^31 - 1) / 3; bad shapes and null pointers are refused
 * by name before any launch.  record is 16-byte aligned.
 *
 * K35a, one wavefront (64 lanes) per triangle f, K32a's organisation.  record (num_triangles,16)
 * int32 from K31a; ids (height width) int32 from K31c; d_color (height width,3) f32: the gradient of
 * a loss in K31c's colour (under antialiasing, K34b's d_color); colors (num_vertices,3) f32;
 * triangles (num_triangles,3) int32, ids clamped into 0 .. num_vertices - 1 as in K31.
 *   the box, n, the box pixels k and the SELECTED ones (ids[p] == f) exactly as in K32a: a box that
 *   is empty, not inside the image, or has n > 2^28 contributes nothing; a pixel that is not selected
 *   is skipped by selection, d_color[p] is not read
 *   per triangle: X, Y, A, sgn = sign(A), w_i from record[f]; c_i = colors[triangles[f][i]];
 *     for edge i with j = (i+1) mod 3, k = (i+2) mod 3:  dx_i = sgn (-(Y_k - Y_j)), dy_i = sgn (X_k - X_j)
 *     (int64);  n_i = ((256.0f * (float)dx_i) / (float)|A|, (256.0f * (float)dy_i) / (float)|A|): the
 *     gradient of lambda_i per pixel
 *   a selected pixel: E_i as in K31b (int64, sgn applied); lambda_i = (float)E_i / (float)|A|;
 *     q_i = lambda_i / w_i;  depth_w = 1.0f / ((q0 + q1) + q2);  b_i = q_i * depth_w (the bits of K31c);
 *     C_ch = (c0_ch b0 + c1_ch b1) + c2_ch b2;  g = d_color[p];
 *     a_i = (g_r * (ci_r - C_r) + g_g * (ci_g - C_g)) + g_b * (ci_b - C_b);
 *     r_i = (a_i * depth_w) / w_i: d loss / d lambda_i;
 *     G = ((r0 * n0.x + r1 * n1.x) + r2 * n2.x, likewise y): d loss / d (the sample point, in pixels);
 *     t[3 j] = -(lambda_j * G.x), t[3 j + 1] = -(lambda_j * G.y): d loss / d (sx, sy) of corner j;
 *     t[3 j + 2] = -(r_j * q_j): d loss / d w_j
 *   segments of 64 box pixels, the fold x += shfl_xor(x, off), off = 32 .. 1, and acc = acc + segment_s
 *   from 0.0f in the order of s, as in K32a
 * face_grads (num_triangles,9) f32 = the nine acc.  Every row is written; the row of a triangle that
 * is not drawn, or wins no pixel, is +0.
 *
 * K35b, one thread per vertex v.  corner_order (3 num_triangles) and vertex_starts (num_vertices + 1)
 * int32: K32b's CSR, the range of a row clamped into the array.  From 0.0f and in that order, for the
 * corner 3 f + i:  gx = gx + face_grads[f][3 i], gy = gy + face_grads[f][3 i + 1],
 * gw = gw + face_grads[f][3 i + 2]; a corner outside 0 .. 3 num_triangles - 1 is skipped.  v projected
 * as in K31a to x, y, w, sx = x / w, sy = y / w (proj: 12 floats in HOST memory).  !(w > 0): the row
 * is +0.  Else, per component c of the position, with P the rows of proj:
 *   grad[v][c] = ((gx * (P0c - sx * P2c)) + (gy * (P1c - sy * P2c))) / w + gw * P2c
 * grad (num_vertices,3) = the row, or with accumulate != 0 out = out + row, one add each: this is how
 * it joins K34c's result in one buffer.  The loop is linear in the valence. */
int ffn_mesh_interp_face_grads(const int32_t* record, const int32_t* ids, const float* d_color,
                               const float* colors, int64_t num_vertices, const int32_t* triangles,
                               int64_t num_triangles, int width, int height, float* face_grads,
                               void* stream);
int ffn_mesh_interp_vertex_grad(const float* face_grads, const int32_t* corner_order,
                                const int32_t* vertex_starts, int64_t num_triangles,
                                const float* vertices, int64_t num_vertices, const float* proj,
                                float* grad, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K36  rays against a triangle mesh: a tree over the triangles, the nearest or farthest hit of every
 * ray, the shading of the hits (csrc/mesh_cast.hip).  No counterpart in the reference.  What K13/K14
 * are for octrees: K31 needs a pinhole camera and refuses every triangle that reaches w <= 0; a cast
 * has no camera plane and answers for any ray.  Every float operation is one rounded f32 operation in
 * the order written (no fma; / is the IEEE division); no atomics, no LDS, no scratch: the same inputs
 * give the same bits on every call.  tests/mesh_cast_reference.py restates all of it in numpy f32.
 * Every index read from an input array is held against its range before it is used: vertex ids are
 * clamped into 0 .. num_vertices - 1 as in K22/K31, the entries of order into 0 .. num_triangles - 1.
 * Limits: 1 <= num_vertices, num_triangles <= (2^31 - 1) / 3; 1 <= num_rays < 2^31; 1 <= leaf_size
 * <= 64; levels is the smallest number with leaf_size 2^(levels - 1) >= num_triangles (at most 31) and
 * is refused when it is not; bad shapes and null pointers are refused by name before any launch.
 * nodes and boxes are 8-byte aligned.
 *
 * Conventions: dot(a,b) = (a.x b.x + a.y b.y) + a.z b.z;  cross(a,b).x = a.y b.z - a.z b.y, cyclically.
 *
 * The box of a triangle with the (clamped) vertices a, b, c: lo = min(a,b,c) - pad, hi = max(a,b,c) +
 * pad per axis, pad >= 0 one finite f32.  A triangle with a non-finite coordinate gets the EMPTY box
 * lo = +inf, hi = -inf.  A box is empty iff lo.x > hi.x; an empty box is never entered and its triangle
 * never hit (the slab test below would take it for the whole line, hence the explicit clause).
 *
 * The slab test of a box and a ray (o, d): inv = 1.0f / d per axis; t0 = (lo - o) inv, t1 = (hi - o)
 * inv; near_a = fminf(t0, t1), far_a = fmaxf(t0, t1) (a NaN operand is dropped, numpy's fmin / fmax);
 * tn = fmaxf(fmaxf(near_x, near_y), near_z), tf = fminf(fminf(far_x, far_y), far_z).
 *
 * The triangle test (Moeller-Trumbore, two-sided): e1 = b - a, e2 = c - a, p = cross(d, e2), det =
 * dot(p, e1), k = 1.0f / det, s = o - a, u = dot(p, s) k, q = cross(s, e1), v = dot(d, q) k, t = dot(q,
 * e2) k.  Triangle f is HIT iff det != 0, u >= 0, v >= 0, u + v <= 1, t is finite, t > t_min, its box is
 * not empty and tn <= t <= tf for its own box.  The last clause makes a tree exact: every operation of
 * the slab test is monotone, so a box built by min / max alone over other boxes has a [tn, tf] that
 * contains theirs bit for bit, and a culled node cannot hide a hit.  The answer for a ray is the
 * minimum of (t, f) over the hit triangles, lexicographically; in farthest mode the maximum t, ties to
 * the lower f.  It does not depend on order (any permutation), leaf_size or the keys.
 *
 * K36a, one thread per triangle.  boxes (num_triangles,6) f32 = lo, hi.  keys (num_triangles) int32:
 * per axis centre = (lo + hi) 0.5f, cell = (centre - grid) grid_scale, q = (int)fminf(fmaxf(cell,
 * 0.0f), 1023.0f); key = the bits of q.x, q.y, q.z interleaved, x lowest (30 bits); 2^30 for an empty
 * box.  The caller sorts key << 32 | f (torch.sort: plumbing, as in K12 and K30) into order.
 *
 * K36b, one thread per node of a level, `levels` launches from the leaves up.  nodes (2^levels - 1, 6)
 * f32, level l (2^l nodes) from row 2^l - 1: no pointers.  Leaf j of the last level: fminf / fmaxf
 * from the empty box over boxes[order[p]], j leaf_size <= p < min((j + 1) leaf_size, num_triangles).
 * Node j of a level above: fminf of the lo, fmaxf of the hi of nodes 2 j and 2 j + 1 of the next level.
 * Every row is written.
 *
 * K36c, one lane per ray; starts, directions (num_rays,3) f32.  The walk is depth first, left child
 * first, on (level, index) alone, every node visited at most once, the loop bounded by 2^levels - 1
 * trips.  A node is entered iff its box is not empty, tn <= tf, tf > t_min and (nearest) tn <= t_best,
 * (farthest) tf >= t_best; t_best is +inf (-inf) until a triangle is hit.  Per ray: hit (num_rays)
 * int32 = f, or -1; t, u, v (num_rays) f32 of that triangle, all 0 for a miss.  A NaN or infinite
 * ray misses.  t_min is not NaN; farthest is 0 or 1.
 *
 * K36d, one thread per ray, hit, t, u, v as K36c writes them (a hit outside 0 .. num_triangles - 1 is
 * a miss).  b0 = (1.0f - u) - v, b1 = u, b2 = v.  Either vertex_colors (num_vertices,3): colour =
 * (c0 b0 + c1 b1) + c2 b2 per channel; or uvs (num_vertices,2) and texture (tex_height, tex_width,
 * tex_channels) uint8, the row index growing with v: the UV interpolated the same way and put through
 * K22's lookup.  color (num_rays,3), alpha (num_rays) = 1, depth (num_rays) = t; a miss gets the
 * background, 0 and 0. */
int ffn_mesh_cast_boxes(const float* vertices, int64_t num_vertices, const int32_t* triangles,
                        int64_t num_triangles, float pad, float grid_x, float grid_y, float grid_z,
                        float grid_scale, float* boxes, int32_t* keys, void* stream);
int ffn_mesh_cast_tree(const float* boxes, const int32_t* order, int64_t num_triangles,
                       int leaf_size, int levels, float* nodes, void* stream);
int ffn_mesh_cast(const float* nodes, const float* boxes, const int32_t* order,
                  const float* vertices, int64_t num_vertices, const int32_t* triangles,
                  int64_t num_triangles, int leaf_size, int levels, const float* starts,
                  const float* directions, int64_t num_rays, float t_min, int farthest,
                  int32_t* hit, float* t, float* u, float* v, void* stream);
int ffn_mesh_cast_shade(const int32_t* hit, const float* t, const float* u, const float* v,
                        int64_t num_rays, const int32_t* triangles, int64_t num_triangles,
                        const float* vertex_colors, const float* uvs, int64_t num_vertices,
                        const uint8_t* texture, int tex_height, int tex_width, int tex_channels,
                        float background_r, float background_g, float background_b, float* color,
                        float* alpha, float* depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FFN_HIP_H */
