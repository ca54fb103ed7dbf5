/*
 * isdf_hip.h -- C ABI of the MI355X-native iSDF training hot path.
 *
 * The reference (facebookresearch/iSDF) is pure Python/PyTorch and has no FFI;
 * its seam for this path is the Python method `Trainer.step`
 * (isdf/modules/trainer.py:951-1016) and the two methods it calls,
 * `Trainer.sample_points` (:683-766) and `Trainer.sdf_eval_and_loss` (:768-868).
 * This header is what a ctypes binding inside those methods binds to; the
 * reference-side binding (graft(trainer)) is shown in INTEGRATION.md and lives in
 * isdf_amd/hot_path.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are
 *     DEVICE pointers unless a parameter name ends in `_host`.
 *   - The caller owns every buffer (torch allocates them); the library keeps
 *     no state between calls and never allocates, frees or synchronises.
 *   - All work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - Return value: 0 on success, a negative ISDF_E* code otherwise; never
 *     throws.  isdf_error_string() names the code.
 *   - Points are stored ray-major: point n = ray * S + s, S = n_strat + n_surf.
 */
#ifndef ISDF_HIP_H
#define ISDF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISDF_ABI_VERSION 8

enum {
  ISDF_OK = 0,
  ISDF_EINVAL = -1,       /* bad argument / null pointer / size mismatch      */
  ISDF_EUNSUPPORTED = -2, /* configuration the kernels are not built for      */
  ISDF_EWORKSPACE = -3,   /* caller workspace too small                       */
  ISDF_EHIP = -4,         /* a HIP runtime call failed (see hipGetLastError)  */
  ISDF_ECOLLECTIVE = -5   /* the caller's collective library refused the call */
};

/* ---- network description ------------------------------------------------
 * Mirrors SDFMap(PostionalEncoding) (isdf/modules/fc_map.py:63-111,
 * isdf/modules/embedding.py:24-111).  Parameters live in ONE flat fp32 buffer
 * in `named_parameters()` order:
 *   in_layer.0.{weight[Hd,E],bias[Hd]}, mid1.i.0.{weight[Hd,Hd],bias}, i<B,
 *   cat_layer.0.{weight[Hd,Hd+E],bias}, mid2.i.0.{...}, out_alpha.{weight[1,Hd],bias[1]}
 * (the host mirror re-points the nn.Module parameters at views of it).       */
typedef struct isdf_net_cfg {
  int32_t hidden;        /* Hd: hidden_feature_size (replicaCAD.json:58): any value <= 512 (widths other than 256 / 512 run zero-padded
                            on the 256- / 512-wide tile kernels; parameters, moments and gradients keep the reference's shapes) */
  int32_t blocks;        /* B : hidden_layers_block (replicaCAD.json:57)       */
  int32_t n_freqs;       /* n_embed_funcs + 1 (embedding.py:36); E = 42*n+3    */
  int32_t has_transform; /* 0: PE transform is None (live modes)    */
  float scale_input;     /* embedding.scale_input                              */
  float scale_output;    /* model.scale_output (fc_map.py:109)                 */
  float bounds_T[12];    /* rows of inv_bounds_transform[:3,:4] (row-major)    */
  int32_t fwd_operand;   /* MFMA operands of the forward and first-backward
                            GEMMs (the second-order passes: bwd_operand):
                            0 bf16; 1 fp16; 2 "fp16x2" = fp16 with a compensated
                            forward -- layers >= cat_layer also multiply the
                            fp16 residual of their weights, the layers past it
                            the fp16 residual of their input too -- which is
                            what meets the reference's fp32 sdf to 1e-3
                            (fc_map.py:94-111); 3 "fp16x2_full" =
                            the same compensation in EVERY forward layer, the
                            embedding included (exact-forward instrument: sdf
                            ~1e-6 and d sdf/dx < 1e-3 of the reference;
                            hidden 256 with a padded embedding of 256 only,
                            other shapes ISDF_EUNSUPPORTED).  isdf_shadow_bytes
                            grows by one forward set for modes 2 and 3.        */
  int32_t bwd_operand;   /* ABI 5: MFMA operands of the SECOND-order passes (adjoint of the input-gradient sweep, reverse sweep
                            with the injected term, the dW contraction) and storage type of the tensors spilled between them:
                            0 bf16 (range-safe for any loss-adjoint magnitude; rounds 1-3), 1 fp16 (needs fwd_operand >= 1;
                            11 instead of 8 significand bits in every weight-gradient operand: total_loss.backward(),
                            trainer.py:981, to ~1e-3 instead of ~4e-3; the adjoints of the shipped configs sit well inside
                            fp16's range)                                                                    */
  int32_t spill_operand; /* ABI 6: storage of two of the four tensor families the training step parks in HBM between its sweeps and for
                            the dW contraction -- P = d sdf / d z (below the top layer) and GB = the adjoint entering each layer in
                            the upward sweep, i.e. the operands of the SECOND-order product of total_loss.backward() (the eikonal /
                            normal terms' share of the gradient, trainer.py:814-830,981):
                            0 auto: e4m3 when n_freqs <= 6, hidden <= 256 and bwd_operand is fp16 (replicaCAD.json / scanNet.json), else 16-bit;
                            1 the 16-bit bwd_operand type (rounds 1-5); 2 OCP e4m3 (hidden <= 256 only), one byte per element: P / 2^-10, GB / s_G with a
                            per-POINT scale s_G (GB is linear in the point's loss adjoint); 3 e4m3 for GB only.  e4m3 halves 11 of the 23 tensors a step
                            stores and 21 of the 50 it reads back; at six octaves it moves the worst weight gradient by 2e-4 of the
                            reference's, with nine or more octaves the second-order term carries most of the first layers' gradient
                            and e4m3 costs ~1e-2 there -- which is why `auto` keeps those nets on 16 bits.            */
} isdf_net_cfg;

int isdf_abi_version(void);
const char* isdf_error_string(int code);

/* ISDF_OK if the tile kernels are instantiated for this network shape, ISDF_EUNSUPPORTED otherwise (call it when
 * the network is built -- trainer.py:419-439 -- rather than at the first step) */
int isdf_check_net(const isdf_net_cfg* net);

/* number of fp32 parameters (460033 for the default net) */
int64_t isdf_param_count(const isdf_net_cfg* net);
/* bytes of the packed 16-bit MFMA-operand copies of the weights ("shadow") */
int64_t isdf_shadow_bytes(const isdf_net_cfg* net);
/* bytes of scratch isdf_train_step / isdf_sdf_eval need for up to max_points */
int64_t isdf_workspace_bytes(const isdf_net_cfg* net, int64_t max_points, int32_t train);
/* number of floats in the flat reduction buffer written by isdf_train_step:
 *   [ grad(n_params) | loss_sums(8) | block_loss(F*64) | block_cnt(F*64) ]    */
int64_t isdf_reduce_floats(const isdf_net_cfg* net, int32_t n_frames);
/* first float of the reduction buffer that is complete when isdf_step_out.split_event is recorded: the message's SUFFIX
 * [isdf_reduce_split_floats, isdf_reduce_floats + extra_floats) = weight gradients of the layers from the cat layer up, the out
 * layer, loss sums, bins and the caller's tail; the PREFIX [0, isdf_reduce_split_floats) = layers below the cat layer
 * follows with the call's last launch.  (New: the reference has no collective, README.md:102; SURVEY 8e "overlap the
 * all-reduce of early-finished layers' dW".)                                                                       */
int64_t isdf_reduce_split_floats(const isdf_net_cfg* net);

/* Rebuild the packed operand copies from the fp32 parameters (after loading a
 * checkpoint; isdf_adamw does it itself after every update).                  */
int isdf_pack_weights(const isdf_net_cfg* net, const float* params, void* shadow, void* stream);

/* ---- K1: ray / point sampler ---------------------------------------------
 * Replaces sample.sample_pixels + get_batch_data + sample_along_rays
 * (isdf/modules/sample.py:11-178) and transform.origin_dirs_W
 * (isdf/geometry/transform.py:36-41).  dirs_C is computed from the intrinsics
 * (transform.py:13-33) instead of gathered from a [H,W,3] table.             */
typedef struct isdf_sample_args {
  /* keyframe store (data_util.FrameData, isdf/datasets/data_util.py:11-81)   */
  const float* depth_batch;   /* [K,H,W]                                       */
  const float* normal_batch;  /* [K,H,W,3] or NULL (do_normal false)           */
  const float* T_WC_batch;    /* [K,4,4]                                       */
  const int32_t* frame_idx;   /* [F] window -> keyframe index (trainer.py:965) */
  const int32_t* normal_idx;  /* [F] keyframe index used for normals; the
                                 reference passes the un-windowed normal_batch
                                 (trainer.py:956,969): pass 0..F-1
                                 to reproduce, frame_idx to fix                */
  int32_t n_frames;           /* F                                             */
  int32_t n_rays;             /* rays per frame (sample.n_rays)                */
  int32_t H, W;
  float fx, fy, cx, cy;
  int32_t n_strat, n_surf;    /* sample.n_strat_samples / n_surf_samples       */
  float min_depth;            /* sample.depth_range[0]                         */
  float dist_behind_surf;
  /* random inputs.  rng_mode 0 ("injected", parity): the caller supplies the
   * draws the reference would make, in the reference's own shapes:
   *   draw_h/draw_w [F*n_rays] int64  (torch.randint, sample.py:15-16)
   *   draw_u [R,n_strat] (torch.rand, sample.py:123), draw_n [R,n_surf-1]
   *   (torch.normal(0,0.1) on the CPU generator, sample.py:160-162), both
   *   indexed by COMPACTED ray.  rng_mode 1: in-kernel Philox4x32-10 keyed by
   *   (seed, offset): counter (drawn ray, 0) for the pixel, one call per four
   *   consecutive-by-64 output points for the along-ray draws (surface
   *   offsets: Box-Muller on the two 16-bit halves of a word); deterministic
   *   for a given (seed, offset, configuration), not stream-compatible with
   *   torch, and the mapping may change between ABI versions.                 */
  int32_t rng_mode;
  const int64_t* draw_h;
  const int64_t* draw_w;
  const float* draw_u;
  const float* draw_n;
  uint64_t seed, offset;
  /* ABI 5 -- the window INLINE: with n_inline == n_frames (1..ISDF_MAX_INLINE_FRAMES) the kernel takes the window's keyframe
   * indices from these kernel arguments and ignores frame_idx / normal_idx (which may then be NULL): no device copy of a window
   * that select_keyframes (trainer.py:652-674) re-draws on the host every step, and no dependent index load in front of the
   * depth gather.  0 = use the device arrays.                                                                            */
  int32_t n_inline;
  int32_t frame_idx_inline[8];
  int32_t normal_idx_inline[8];
  int32_t reserved_inline;
} isdf_sample_args;
#define ISDF_MAX_INLINE_FRAMES 8

typedef struct isdf_sample_out {
  int32_t* n_valid;      /* [1]  R = rays kept (depth != 0, normal not NaN)    */
  int64_t* indices_b;    /* [F*n_rays] first R entries valid (ordered)         */
  int64_t* indices_h;
  int64_t* indices_w;
  float* depth_sample;   /* [F*n_rays]                                         */
  float* dirs_C_sample;  /* [F*n_rays,3]                                       */
  float* norm_sample;    /* [F*n_rays,3] or NULL                               */
  float* T_WC_sample;    /* [F*n_rays,4,4] or NULL (reference materialises it) */
  float* dirs_W_sample;  /* [F*n_rays,3] world-frame ray direction             */
  float* z_vals;         /* [F*n_rays,S]                                       */
  float* pc;             /* [F*n_rays,S,3]                                     */
} isdf_sample_out;

/* ONE launch: pixel draw (or injected draws), gather of depth + normal, validity, ORDER-PRESERVING
 * compaction across workgroups (decoupled look-back), then per compacted ray the stratified + surface z
 * values and world points.  scan_ws: device scratch of isdf_sample_scan_bytes(F*n_rays) bytes that must be
 * ZERO when first used and is otherwise private to this entry point (it re-arms itself at the end of every
 * launch; launches sharing one scan_ws must be stream-ordered).                                            */
int64_t isdf_sample_scan_bytes(int64_t max_rays);
int isdf_sample_rays(const isdf_sample_args* a, const isdf_sample_out* o, void* scan_ws,
                     int64_t scan_ws_bytes, void* stream);

/* ---- fused PE + MLP (+ input gradient) inference --------------------------
 * Replaces SDFMap.forward and fc_map.gradient (fc_map.py:94-111,12-22) for
 * arbitrary points.  noise: pre-scaled additive term on the raw output
 * (fc_map.py:106-108) or NULL.  sdf_grad may be NULL.                          */
int isdf_sdf_eval(const isdf_net_cfg* net, const float* params, const void* shadow,
                  const float* pts, int64_t n_points, const float* noise,
                  float* sdf, float* sdf_grad, void* workspace, int64_t workspace_bytes,
                  void* stream);

/* ---- training step (everything between sampling and the optimiser) --------
 * Replaces Trainer.sdf_eval_and_loss + total_loss.backward()
 * (trainer.py:768-868,981; loss.py:13-240).                                   */
typedef struct isdf_loss_cfg {
  int32_t bounds_method;  /* 0 "ray" (loss.py:13-22), 1 "pc" (loss.py:56-89)   */
  int32_t loss_type;      /* 0 L1, 1 L2 (loss.py:138-143)                      */
  float trunc_weight, trunc_distance, eik_weight, eik_apply_dist, grad_weight;
  int32_t orien_loss;
} isdf_loss_cfg;

typedef struct isdf_step_args {
  const int32_t* n_valid;     /* [1] device: R (from the sampler)              */
  int32_t max_rays;           /* capacity of the per-ray arrays (F*n_rays)     */
  int32_t S;                  /* samples per ray                               */
  int32_t n_frames, H, W;     /* for the 8x8 block-loss bins (loss.py:208-240);
                                 H and W must be multiples of 8 (ISDF_EINVAL otherwise, as
                                 the reference's .view raises)                    */
  const float* pc;            /* [max_rays,S,3]                                */
  const float* z_vals;        /* [max_rays,S]                                  */
  const float* depth_sample;  /* [max_rays]                                    */
  const float* dirs_C_sample; /* [max_rays,3]                                  */
  const float* dirs_W_sample; /* [max_rays,3]                                  */
  const float* norm_sample;   /* [max_rays,3] (may be NULL when grad_weight=0) */
  const int64_t* indices_b;   /* [max_rays]                                    */
  const int64_t* indices_h;
  const int64_t* indices_w;
  const float* noise;         /* [max_rays,S] pre-scaled, or NULL              */
  float noise_std;            /* used when noise == NULL and noise_std != 0:   */
  uint32_t reserved0;         /* in-kernel Philox N(0,1) * noise_std keyed by  */
  uint64_t noise_seed;        /* (noise_seed, noise_offset, point)             */
  uint64_t noise_offset;      /* (fc_map.py:106-108)                            */
  const float* pc_bounds;     /* [max_rays,S]   bounds_method "pc" only        */
  const float* pc_grad_vec;   /* [max_rays,S,3] bounds_method "pc" only        */
  /* caller-owned tail of the reduction message (data parallel): reduce_buf may be
   * followed by `extra_floats` floats that ride in the same all-reduce; the step
   * writes extra_value into slot extra_slot and 0 into the others (one slot per
   * rank: after the SUM all-reduce every rank holds every rank's value -- the
   * host mirror carries the ranks' step times this way, no second collective) */
  int32_t extra_floats;
  int32_t extra_slot;
  float extra_value;
  int32_t reserved1;
} isdf_step_args;

typedef struct isdf_step_out {
  float* reduce_buf;    /* [isdf_reduce_floats]: SUMS (not means) so that ranks
                           can be all-reduced and scaled once      */
  float* sdf;           /* optional [max_rays,S]  debug / parity outputs       */
  float* sdf_grad;      /* optional [max_rays,S,3]                             */
  float* tot_loss_mat;  /* optional [max_rays,S]                               */
  void** prof_events;   /* optional HOST array of 4 hipEvent_t recorded on `stream`:
                           [0] before the chain kernel, [1] after it, [2] after
                           the dW kernel, [3] after the reductions (bench.py)    */
  float* host_mailbox;  /* optional PINNED HOST memory (device-mapped, >= 8 floats): the
                           step's last launch also stores loss_sums[8] there, so the
                           `losses` of Trainer.step (trainer.py:1016; loss.py:187-200)
                           need no device->host copy command -- they are valid after the
                           caller's closing stream synchronisation (metrics.py:27-30)   */
  void* split_event;    /* optional hipEvent_t, isdf_train_step only (data parallel): the closing reduction runs as TWO
                           launches and this event is recorded on `stream` between them -- the suffix of reduce_buf
                           (isdf_reduce_split_floats) is final at the event, so its all-reduce can run on a second stream
                           beside the second launch.  Same arithmetic, same values as the one-launch form.            */
} isdf_step_out;

/* layout of loss_sums inside reduce_buf (after the n_params gradient floats) */
enum { ISDF_LS_SDF = 0, ISDF_LS_GRAD = 1, ISDF_LS_EIK = 2, ISDF_LS_TOTAL = 3, ISDF_LS_COUNT = 4 };

int isdf_train_step(const isdf_net_cfg* net, const isdf_loss_cfg* loss, const float* params,
                    const void* shadow, const isdf_step_args* a, const isdf_step_out* o,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* Single-GPU form of the same step with the optimiser fused in: what
 * `total_loss.backward(); self.optimiser.step(); self.optimiser.zero_grad()` do in
 * Trainer.step (isdf/modules/trainer.py:981-983) as ONE call.  After the dW kernel a single
 * launch sums the gradient, applies AdamW to params / exp_avg / exp_avg_sq in place,
 * refreshes the packed operand copies in `shadow`, and finalises the loss sums and block
 * bins.  reduce_buf is written exactly as by isdf_train_step (the gradient is the SUM over
 * points; AdamW divides by the point count).  Bit-identical to isdf_train_step followed by
 * isdf_adamw(count_ptr = &loss_sums[ISDF_LS_COUNT]).  Data-parallel runs use the two-call
 * form because the gradient all-reduce sits between the reduction and the update.          */
typedef struct isdf_optim_args {
  float* params;        /* [n_params] fp32 master weights, updated in place               */
  float* exp_avg;       /* [n_params] AdamW first moment                                   */
  float* exp_avg_sq;    /* [n_params] AdamW second moment                                  */
  void* shadow;         /* packed operand copies (isdf_shadow_bytes), refreshed in place   */
  float lr, beta1, beta2, eps, weight_decay;
  float grad_scale;     /* multiplies the mean gradient (1.0 for the reference's loss)     */
  int32_t step;         /* 1-based optimiser step (bias correction)                        */
  int32_t reserved;
  /* optional: loss.frame_avg (loss.py:208-240) of this step written by the same launch, i.e. what
   * isdf_frame_avg would return: loss_approx [F,8,8] and frame_avg[frame_avg_index ?
   * frame_avg_index[f] : f] -- pass the keyframe store's frame_avg_losses and the window's keyframe
   * indices to get `self.frames.frame_avg_losses[idxs] = frame_avg_loss` (trainer.py:979) for free.
   * Both or neither of loss_approx / frame_avg.                                                    */
  float* loss_approx;
  float* frame_avg;
  const int32_t* frame_avg_index;
  /* ABI 5: the same index list inline (frame_avg_inline_n == n_frames, 1..ISDF_MAX_INLINE_FRAMES; frame_avg_index is then
   * ignored and may be NULL), for the host-drawn window of every step (see isdf_sample_args.n_inline)                       */
  int32_t frame_avg_inline_n;
  int32_t frame_avg_index_inline[8];
  int32_t reserved_inline;
} isdf_optim_args;

int isdf_train_step_adamw(const isdf_net_cfg* net, const isdf_loss_cfg* loss, const isdf_step_args* a,
                          const isdf_step_out* o, const isdf_optim_args* opt, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* Second half of the DATA-PARALLEL step: after isdf_train_step has written this rank's SUMS to reduce_buf
 * and ONE all-reduce(sum) over reduce_buf has made them global, this single launch does what
 * `self.optimiser.step()` and `self.frames.frame_avg_losses[idxs] = frame_avg_loss` do upstream (trainer.py:979-982):
 * AdamW on gradient = grad_sum * grad_scale / reduced count, refresh of the packed operand copies, and (when
 * opt->loss_approx / opt->frame_avg are given) loss.frame_avg (loss.py:208-240) from the reduced bins.
 * isdf_train_step + all-reduce + isdf_train_step_finish == isdf_train_step_adamw on the union batch
 * (tests/test_dp_gpu.py).                                                                                          */
int isdf_train_step_finish(const isdf_net_cfg* net, const isdf_optim_args* opt, const float* reduce_buf,
                           int32_t n_frames, int32_t extra_floats, float* host_mailbox, void* stream);

/* THE collective of the data-parallel step, enqueued on the step's OWN stream between isdf_train_step and
 * isdf_train_step_finish: in-place sum of buf[0..count) over the communicator's ranks.  The library does not link a
 * collective library: the caller passes the address of RCCL's `ncclAllReduce` (from the RCCL build its communicator was
 * created with -- torch ships its own) and the communicator (ncclComm_t).  Stream order replaces the two cross-stream
 * event hand-offs of a framework-issued collective (torch.distributed.all_reduce runs on a side stream: +36 us per step
 * at world size 1 in round 5, profiles/r05_bench_forced_dp_world1.json).  The caller must not have another collective of
 * the same communicator in flight on a different stream.  Returns ISDF_ECOLLECTIVE (with the library's code in
 * isdf_error_string's text) if RCCL refuses the call.  Reference: none (the reference is single-process).  */
typedef int (*isdf_nccl_allreduce_fn)(const void* sendbuf, void* recvbuf, size_t count, int datatype, int op,
                                      void* comm, void* stream);
int isdf_allreduce_sum_f32(isdf_nccl_allreduce_fn nccl_all_reduce, void* comm, float* buf, int64_t count, void* stream);
/* extra_floats / host_mailbox (optional, pinned host memory of 8 + extra_floats floats): the same launch stores the
 * REDUCED loss_sums[8] followed by the message's caller-owned tail there (isdf_step_args.extra_floats).
 * extra_floats > 0 without a host_mailbox is ISDF_EINVAL (the tail would be dropped silently).                    */

/* nearest-surface-point bounds (bounds_method "pc", loss.py:56-89): for every sample point the distance to
 * the nearest SURFACE sample (sign from z vs depth) and the unit vector from it.  surf_pts == NULL: the
 * surface set is this batch's own pc[:, 0, :] (what the single-process reference uses, loss.py:58-61).
 * Data parallel: surf_pts [n_surf,3] is the all-gathered surface set of all ranks' rays, so each
 * rank sees the surface the single-process run with the global batch would see; slots of dropped rays may
 * hold any far-away sentinel (e.g. 1e18).                                                                    */
int isdf_bounds_pc(const int32_t* n_valid, int32_t max_rays, int32_t S, const float* pc,
                   const float* z_vals, const float* depth_sample, const float* surf_pts,
                   int64_t n_surf, float* bounds, float* grad_vec, void* stream);

/* per-frame 8x8 block-loss averages from the (all-reduced) bins (loss.py:208-240): loss_approx [F,8,8] and
 * frame_avg_loss[frame_avg_index ? frame_avg_index[f] : f] -- pass the keyframe store's frame_avg_losses and
 * the window's keyframe ids to get `self.frames.frame_avg_losses[idxs] = frame_avg_loss` (trainer.py:979)
 * without the separate index_put; frame_avg_index NULL: dense [F] output.                                  */
int isdf_frame_avg(const float* reduce_buf, int64_t n_params, int32_t n_frames,
                   float* loss_approx, float* frame_avg_loss, const int32_t* frame_avg_index,
                   void* stream);

/* ---- per-frame ingest and keyframe test ("next" tier) ------------
 * isdf_estimate_normals: transform.pointcloud_from_depth_torch +
 * estimate_pointcloud_normals (transform.py:169-196,215-270) as run by
 * Trainer.get_data (trainer.py:553-557): depth [H,W] (0 = invalid) -> camera-frame
 * unit normals [H,W,3] (NaN where the 8-neighbour stencil has no valid pair).   */
int isdf_estimate_normals(const float* depth, int32_t H, int32_t W, float fx, float fy, float cx,
                          float cy, float* normals, void* stream);

/* isdf_render_depth: the keyframe test of Trainer.is_keyframe (trainer.py:597-609):
 * per ray sort the S samples by z, render.sdf_render_depth (render.py:12-35), and
 * count rays with |view - depth| / depth < kf_dist_th.  n_valid (device) or, when
 * NULL, n_rays_host rays; depth_sample / below_count may be NULL (render only).  */
int isdf_render_depth(const int32_t* n_valid, int64_t n_rays_host, int64_t max_rays, int32_t S,
                      const float* z_vals, const float* sdf, const float* depth_sample,
                      float kf_dist_th, float* view_depth, int32_t* below_count, void* stream);

/* ---- fused flat AdamW + operand-copy refresh -------------------------------
 * Replaces torch.optim.AdamW.step (trainer.py:435-439,982): decoupled weight
 * decay on all parameters, bias-corrected moments.  grad_scale multiplies the
 * summed gradient; count_ptr (device, optional) divides it further by
 * *count_ptr (the all-reduced number of loss elements).                        */
int isdf_adamw(const isdf_net_cfg* net, float* params, float* exp_avg, float* exp_avg_sq,
               const float* grad_sum, const float* count_ptr, float grad_scale,
               float lr, float beta1, float beta2, float eps, float weight_decay,
               int32_t step, void* shadow, void* stream);

/* ---- mesh reconstruction (ABI 8) -------------------------------------------
 * Marching cubes over a dense fp32 volume, the isosurface step of
 * Trainer.mesh_rec (trainer.py:1500-1542; draw3D.marching_cubes_trimesh,
 * draw3D.py:111-160).  An INDEXED mesh: one vertex per sign-changing grid edge.
 *   - corner inside iff value < level (a value equal to level is outside);
 *   - a cell with a non-finite corner emits no triangle, an edge with a
 *     non-finite end no vertex (so no face references a missing vertex);
 *   - grid point (i,j,k) owns its +i, +j, +k edges; vertices are ordered by the
 *     owner's linear index, then axis (i < j < k); faces by cell linear index,
 *     then table order: the output is bit-reproducible (no atomics decide it);
 *   - vertex = a + t (b - a), t = (level - f(a)) / (f(b) - f(a)), in index
 *     coordinates; normal = the central-difference gradient (one-sided at the
 *     borders) interpolated with the same t and normalised: it points toward
 *     increasing value, and the right-hand normal of every face agrees;
 *   - has_transform: positions go through index_to_world (rows of a 3x4
 *     affine), normals through the inverse transpose of its 3x3 part and are
 *     renormalised (a singular 3x3 part: ISDF_EINVAL).                         */
typedef struct isdf_mc_args {
  const float* volume;        /* [D0][D1][D2] row-major: vol[i][j][k]                    */
  int32_t D0, D1, D2;         /* each >= 2, D0*D1*D2 <= 2^31 - 1                         */
  float level;
  int32_t has_transform;
  float index_to_world[12];   /* rows of the 3x4 affine (used iff has_transform)         */
} isdf_mc_args;

#define ISDF_MC_MAX_TRIS 5    /* triangles per cell; isdf_mc_tables' row width is 3x this */

/* workspace bytes of isdf_marching_cubes for a D0 x D1 x D2 volume (ISDF_EINVAL outside the bounds above) */
int64_t isdf_mesh_ws_bytes(int32_t D0, int32_t D1, int32_t D2);

/* counts: device int64[2] = (vertices, faces), ALWAYS written.  verts / normals
 * [max_verts][3] fp32 and faces [max_faces][3] int32 (vertex ids) are written
 * only when the whole mesh fits (vertices <= max_verts, faces <= max_faces);
 * otherwise read counts and call again with larger buffers.  normals may be
 * NULL.  Four launches on `stream`; the workspace needs no initialisation.   */
int isdf_marching_cubes(const isdf_mc_args* args, int64_t* counts, float* verts, float* normals,
                        int64_t max_verts, int32_t* faces, int64_t max_faces, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* HOST-only copy of the tables the kernels use (launches nothing; either
 * pointer may be NULL): edge_corners_host int32[12][2] -- edge e runs along
 * axis e / 4 from corner [e][0] to corner [e][1], corner c sitting at offset
 * (c & 1, c >> 1 & 1, c >> 2 & 1) -- and tri_table_host int8[256][3 *
 * ISDF_MC_MAX_TRIS]: the edge triples of case c (bit c set = corner c inside),
 * -1 padded.                                                                  */
int isdf_mc_tables(int32_t* edge_corners_host, int8_t* tri_table_host);

/* ---- rendered views -----------------------------------------------------
 * The depth / normal renders of Trainer.render_depth_vis, render_normals_vis and
 * latest_frame_vis (trainer.py:1225-1280,1055-1147) for B views at once: per ray
 * of an H x W raster, S stratified samples (sample.stratified_sample +
 * sample_along_rays, sample.py:77-178, no surface samples), the network
 * (isdf_sdf_eval), the first crossing (render.sdf_render_depth, render.py:12-35,
 * as isdf_render_depth without a depth sample) and, optionally, camera-frame
 * normals at the rendered depth (render.render_normals, render.py:38-57:
 * n_C = inverse(R_WC) (-g / (|g| + 1e-4)), the GENERAL 3x3 inverse, and a ray of
 * depth 0 is evaluated at the camera origin).  Ray r = i * W + j of view b.
 * The depth range of a ray has three sources (range_mode):
 *   ISDF_RANGE_SCALAR   [min_depth, max_depth] for every ray: the coarse pass of
 *                       latest_frame_vis (trainer.py:1091-1099); the bin limits
 *                       are torch.linspace(min, max, S + 1) and bin_length is the
 *                       caller's double (max - min) / S rounded to fp32;
 *   ISDF_RANGE_DEPTH    [min_depth, resize(src_depth[b]) + depth_offset]:
 *                       render_depth_vis (trainer.py:1237-1252; depth_offset 0.8),
 *                       resize = OpenCV INTER_LINEAR from src_H x src_W to H x W
 *                       (src = (dst + 0.5) * src_n / dst_n - 0.5, clamped at the
 *                       borders, no antialiasing);
 *   ISDF_RANGE_UPSAMPLE [d - depth_offset, d + depth_offset], d = the bilinear
 *                       align_corners=True upsample of src_depth[b] (the previous
 *                       pass's [src_H, src_W] depth) to H x W: the fine pass of
 *                       latest_frame_vis (trainer.py:1105-1119; depth_offset 0.1).
 * For the last two the limits are linspace(0, 1, S + 1) * (max - min) + min and
 * bin_length = (max - min) / S in fp32 (sample.py:94-105); z = limit + u * bin_length. */
enum { ISDF_RANGE_SCALAR = 0, ISDF_RANGE_DEPTH = 1, ISDF_RANGE_UPSAMPLE = 2 };

typedef struct isdf_render_args {
  int32_t n_views;           /* B >= 0 (0: the call is a no-op)                                    */
  int32_t H, W;              /* view raster, R = H * W rays per view                               */
  int32_t n_samples;         /* S >= 1 (unused when depth_in is given)                             */
  const float* T_WC;         /* [B,4,4] camera-to-world poses (frames.T_WC_batch / T_WC_track)     */
  const float* dirs_C;       /* [R,3] camera-frame ray directions (trainer.dirs_C_vis[_up])        */
  int32_t range_mode;        /* ISDF_RANGE_*                                                        */
  float min_depth;           /* SCALAR / DEPTH: trainer.min_depth                                   */
  float max_depth;           /* SCALAR: trainer.max_depth                                           */
  float bin_length;          /* SCALAR: (max_depth - min_depth) / S                                 */
  float depth_offset;        /* DEPTH: 0.8 (trainer.py:1244); UPSAMPLE: 0.1 (trainer.py:1113-1114)   */
  int32_t src_H, src_W;      /* DEPTH / UPSAMPLE: raster of src_depth                               */
  int32_t rng_mode;          /* 0: draw_u [B,R,S] injected (torch.rand(R, S) per view, sample.py:123);
                                1: in-kernel Philox4x32-10 keyed by seed, counter (render counter),
                                view and ray; not stream-compatible with torch                       */
  const float* src_depth;    /* DEPTH: [B,src_H,src_W] keyframe depth; UPSAMPLE: [B,src_H,src_W]   */
  const float* draw_u;       /* rng_mode 0                                                          */
  uint64_t seed, counter;    /* rng_mode 1                                                          */
  const float* depth_in;     /* [B,R] or NULL: the depth is GIVEN (render_normals_vis) -- no samples,
                                no render; normals_out is then required                              */
} isdf_render_args;

/* workspace bytes of isdf_render_views for n_views x (H * W) rays x n_samples (ISDF_EINVAL on bad sizes).
 * After a call that renders, the workspace BEGINS with z_vals [B,R,S] f32 followed by pc [B,R,S,3] f32
 * (the samples of that call, for parity checks).                                                         */
int64_t isdf_render_ws_bytes(const isdf_net_cfg* net, int32_t n_views, int32_t H, int32_t W, int32_t n_samples);

/* depth_out [B,R] (or NULL), normals_out [B,R,3] (or NULL); at least one of them.  Launches on `stream`:
 * samples, forward, first crossing (unless depth_in), then points, forward with input gradient and the
 * camera-frame rotation (if normals_out).  The workspace needs no initialisation.                        */
int isdf_render_views(const isdf_net_cfg* net, const float* params, const void* shadow, const isdf_render_args* args,
                      float* depth_out, float* normals_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- evaluation against ground truth ---------------------------------------
 * The arithmetic of Trainer.eval_sdf, eval_object_sdf and eval_traj_cost after the network (trainer.py:1831-1866,
 * 1993-2003,2026-2050) in ONE pass over the points: the ground-truth SDF by trilinear interpolation of an axis-aligned
 * volume -- what sdf_util.eval_sdf_interp(handle_oob='mask') gets from scipy's linear RegularGridInterpolator
 * (sdf_util.py:151-216) --, the validity mask, and every sum the three methods divide.
 *   grid coordinate u = (p - origin) / spacing per axis; in bounds iff 0 <= u <= n - 1 on every axis (faces INCLUSIVE);
 *   valid = in bounds and (gt != 0 or not exclude_zero_gt)   (trainer.py:1835 excludes zeros, :1993-2003 does not).
 * record: ISDF_METRICS_RECORD doubles on the device,
 *   [0] valid points  [1] in-bounds points  [2] sum |sdf - gt|
 *   [3..8]  per bin of metrics.binned_losses (limits -inf, 0, 0.1, 0.2, 0.5, 1, +inf, strict on both sides) sum |sdf - gt|
 *   [9..14] per bin the number of points
 *   [15 + 3e ..] for epsilon 1, 1.5, 2 (e = 0, 1, 2): sum |chomp(sdf) - chomp(gt)|, sum chomp(sdf), sum chomp(gt)
 *                (metrics.chomp_cost, metrics.py:95-104), all over the valid points.
 * The record is bit-identical from run to run on the same inputs (per-block partial sums combined in block order).
 * gt_out [n] (optional): the interpolated value, oob_fill where the point is out of bounds; valid_out [n] u8 (optional).
 * workspace: ISDF_SDF_METRICS_WS_BYTES, no initialisation needed.  n = 0 writes a record of zeros.               */
typedef struct isdf_gt_volume {
  const float* values;        /* [nx][ny][nz] row-major fp32 on the device                  */
  int32_t nx, ny, nz;         /* each >= 2, nx * ny * nz <= 2^31 - 1                         */
  int32_t reserved;
  float spacing[3];           /* > 0: transform[i][i] of the grid (sdf_util.py:151-159)      */
  float origin[3];            /* transform[i][3]: world position of grid point (0, 0, 0)     */
} isdf_gt_volume;

#define ISDF_METRICS_RECORD 24
#define ISDF_METRICS_MAX_BLOCKS 1024
#define ISDF_SDF_METRICS_WS_BYTES (ISDF_METRICS_MAX_BLOCKS * ISDF_METRICS_RECORD * 8)

int isdf_sdf_metrics(const isdf_gt_volume* vol, const float* pts, const float* sdf, int64_t n, int32_t exclude_zero_gt,
                     float oob_fill, double* record, float* gt_out, uint8_t* valid_out, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* The arithmetic of eval_pts.fixed_pts_eval after the network (eval_pts.py:96-299) in ONE pass over n points, for the two
 * nested regions it reports ("vis": every visible point, "vox": the part another mapper also covers): the |sdf - gt| figures
 * of isdf_sdf_metrics per region, and the mean cosine distance between the predicted gradient and the central-difference
 * gradient of the ground truth (eval_pts.eval_grad(..., delta, is_gt_sdf=True), eval_pts.py:68-93).
 * flags [n] u8 (optional): bit 1 = in the vis sdf set, 2 = vox sdf set, 4 = vis gradient set, 8 = vox gradient set.  NULL: every
 * point is in both sdf sets and in no gradient set.  Bits 4 and 8 are honoured only when grad_sets != 0.
 * Ground truth from exactly one of: `vol` (trilinear lookup; its grid spacing and origin are read from the DOUBLES of this
 * struct, not from vol's fp32 fields), or `gt_in` [n] doubles on the device (every point counts as in bounds, no lookup; the
 * full-volume leg, whose ground truth comes from a file).  gt_in excludes gradient sets.
 * ALL arithmetic is double -- grid coordinate, in-bounds test (faces inclusive), trilinear blend, sums -- on the fp32 points
 * widened: the reference evaluates these in float64.
 * records: 2 x ISDF_REGION_RECORD doubles on the device, vis then vox:
 *   [0..23]  the fields of isdf_sdf_metrics over the set's points with valid = in bounds (zero-valued ground truth is KEPT, as
 *            eval_pts.sub_eval keeps it); the bins compare the double ground truth with the double limits
 *   [24]     points in the set's gradient set
 *   [25]     sum of 1 - cos over those whose ground-truth gradient is finite, cos = x.y / (max(|x|, 1e-6) * max(|y|, 1e-6))
 *            (torch.nn.CosineSimilarity(dim=1, eps=1e-6)) with the fp32 predicted gradient x widened
 *   [26]     points of [24] whose ground-truth gradient is not finite (one of its six lookups at p +- delta e_i is out of
 *            bounds or == 0): the reference's mean is then NaN
 * The records are bit-identical from run to run (per-block partial records combined in block order, a grid that depends on n
 * alone, no float atomics).  workspace: ISDF_REGION_METRICS_WS_BYTES, no initialisation needed.  n = 0 writes zero records.
 * ISDF_EINVAL: no ground-truth source, or both; grad_sets without sdf_grad; grad_sets together with gt_in; delta <= 0 or
 * not finite; a spacing <= 0.                                                                                          */
typedef struct isdf_region_args {
  const float* pts;           /* [n,3] fp32                                              */
  const float* sdf;           /* [n]   fp32, the prediction                              */
  const float* sdf_grad;      /* [n,3] fp32 or NULL                                      */
  const uint8_t* flags;       /* [n] or NULL                                             */
  const isdf_gt_volume* vol;  /* or NULL (host pointer, read before the call returns)    */
  const double* gt_in;        /* [n] on the device, or NULL                              */
  int64_t n;
  int32_t grad_sets;          /* != 0: flag bits 4 and 8 select gradient points          */
  int32_t reserved;
  double spacing[3];          /* of vol's grid, > 0 (ignored with gt_in)                 */
  double origin[3];
  double delta;               /* > 0: half the central-difference step (0.01)            */
} isdf_region_args;

#define ISDF_REGION_RECORD 27
#define ISDF_REGION_METRICS_WS_BYTES (ISDF_METRICS_MAX_BLOCKS * 2 * ISDF_REGION_RECORD * 8)

int isdf_region_metrics(const isdf_region_args* args, double* records, void* workspace, int64_t workspace_bytes, void* stream);

/* Exact nearest-neighbour distances, the KD-tree queries of metrics.accuracy / completion (metrics.py:48-59), by brute
 * force: dist[q] = min over t of |query[q] - target[t]| for query [n,3] and target [m,3] (m >= 1), fp32 on the device.
 * The squared distance is (dx*dx + dy*dy) + dz*dz of the coordinate DIFFERENCES, each operation rounded to fp32, and
 * dist its correctly rounded square root.  index (optional, int32 [n]): the nearest target, the lowest index on ties.
 * dist_sum: one double on the device, the sum of dist in a fixed order (bit-identical run to run).  dist may be NULL.
 * workspace: ISDF_NN_WS_BYTES(n), no initialisation needed; after the call it BEGINS with one 64-bit key per query,
 * (bits of the squared distance) << 32 | index (index 0xffffffff when none was asked for), for parity checks.
 * n = 0 writes dist_sum = 0.                                                                                      */
#define ISDF_NN_WS_BYTES(n) (8 * (int64_t)(n) + 8 * (((int64_t)(n) + 255) / 256) + 256)

int isdf_nn_distance(const float* query, int64_t n, const float* target, int64_t m, float* dist, int32_t* index,
                     double* dist_sum, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- SDF slice images ---------------------------------------------------------
 * What Trainer.compute_slices, obj_slices_vis and get_sdf_grid_pc do after the network (trainer.py:1593-1595,1603,
 * 1617-1621,1629,1796-1807,1453-1461), in ONE pass over n points on the device:
 *   colour      ScalarMappable.to_rgba(v, alpha=1., bytes=False), then (.. * 255).astype(np.uint8)[..., :3], through a
 *               caller-supplied table: x = ((v - vmin) / range) * (float)n_colors, every operation rounded to fp32 (a true
 *               division); NaN -> bad, x < 0 -> under, x == n_colors -> n_colors - 1, x > n_colors -> over, else (int)x.
 *               Equal to matplotlib on every fp32 value when fp32 holds vmin and vmax - vmin exactly (the reference's tables:
 *               -2, 2 and -0.5, 0.5); with other limits matplotlib subtracts and divides in double before it rounds, and a value
 *               within a few fp32 roundings of a bin edge can land in the neighbouring bin.
 *   ground truth sdf_util.eval_sdf_interp(gt_sdf_interp, pc, handle_oob='fill') (sdf_util.py:183-216): the trilinear value of
 *               isdf_sdf_metrics (the same device function), oob_fill out of bounds.
 *   CHOMP cost  metrics.chomp_cost(sdf, epsilon=chomp_eps) (metrics.py:95-104) of a float32 array, in numpy's order:
 *               -s + eps/2; (1/(2 eps)) * ((s - eps) * (s - eps)) where s > 0; 0 where s > eps.
 * Every output is optional (NULL): pred_rgb u8 [n,3] and pred_cost f32 [n] of sdf [n]; gt_out f32 [n], gt_rgb u8 [n,3] and
 * gt_cost f32 [n] of the volume at pts [n,3].  cmap is needed by the colours, vol and pts by the ground-truth outputs, sdf by the
 * predicted ones, chomp_eps > 0 by the costs; a call with no output, or an output without its input, is ISDF_EINVAL.
 * n = 0 is a no-op.  No workspace, no atomics; the same inputs give the same bytes.                                          */
typedef struct isdf_colormap {
  const uint32_t* lut;  /* device [n_colors + 3], entry = R | G<<8 | B<<16;
                           entries n_colors, n_colors+1, n_colors+2 = under, over, bad */
  int32_t n_colors;     /* N >= 1 (<= ISDF_COLORMAP_MAX_COLORS: the table is staged in LDS) */
  float vmin;           /* (float)norm.vmin */
  float range;          /* (float)(norm.vmax - norm.vmin), > 0 */
} isdf_colormap;

#define ISDF_COLORMAP_MAX_COLORS 16381

int isdf_slice_images(const float* pts, const float* sdf, int64_t n, const isdf_colormap* cmap, const isdf_gt_volume* vol,
                      float oob_fill, float chomp_eps, uint8_t* pred_rgb, float* gt_out, uint8_t* gt_rgb, float* pred_cost,
                      float* gt_cost, void* stream);

/* The points of a plane raster, instead of an index_select on the trainer's grid_pc (trainer.py:1569-1576) or the
 * linspace / meshgrid of obj_slices_vis (trainer.py:1785-1793): pts_out [H,W,3] fp32 on the device,
 *   p[i][j] = (origin + (float)i * du) + (float)j * dv,   each operation rounded to fp32.
 * origin, du, dv: three floats each in HOST memory (read before the call returns).  H * W = 0 is a no-op;
 * H * W <= 2^31 - 1.                                                                                           */
int isdf_plane_points(const float* origin, const float* du, const float* dv, int32_t H, int32_t W, float* pts_out,
                      void* stream);

/* ---- visibility against posed depth frames ---------------------------------------
 * "Is a world point in front of a posed depth frame, inside its image, and no more than trunc metres behind the surface?" --
 * the use_projection=True branch of geometry.frustum.is_visible_torch (frustum.py:87-133), the project's one definition of the
 * visible region (Trainer.eval_object_sdf, trainer.py:1976-1981; the masks of the slice figures, eval/figs/slices.py:274) -- for
 * every pair of F frames and n points in ONE pass; nothing of size F * n is kept unless `mask` is asked for.
 * T_CW is CAMERA-FROM-WORLD (the caller inverts its poses; the reference uses torch.linalg.inv).  Per pair, with a_rc the
 * frame's matrix, every operation rounded to fp32, no fused multiply-add, IEEE division:
 *   xc = ((a00*x + a01*y) + a02*z) + a03, yc and zc alike from rows 1 and 2 (row 3 is not read)
 *   u = (fx*xc + cx*zc) / zc,  v = (fy*yc + cy*zc) / zc
 *   inside  = u > 0 && u < (float)W && v > 0 && v < (float)H          (NaN and +-inf compare false)
 *   pixel   = ((int)v, (int)u), truncated as .long() truncates
 *   visible = inside && zc > 0 && zc < depth[f][row][col] + trunc     (a pixel of 0 or NaN has no case of its own)
 * Equal to a numpy float32 model of these lines on every pair, and to the reference wherever float32 decides as float64 does.
 * count [n] int32: the frames that see the point.  mask [F,n] u8 (optional): 1 where frame f sees point i.  n_seen (optional):
 * one int64, the points with count > 0.  None needs initialisation, all are integers combined by integer adds: the same inputs
 * give the same bytes.  n = 0 or F = 0 writes zeros and reads neither pts nor depth.  Up to two memsets and two launches on
 * `stream` (one more launch per further 2^30 points), no workspace.
 * ISDF_EINVAL: n < 0 or n > 2^38; F < 0; H or W < 1 or H * W > 2^31 - 1; F * n beyond int64; an intrinsic or trunc that is not
 * finite; count NULL with n > 0; pts, T_CW or depth NULL with n > 0 and F > 0.                                              */
int isdf_visible_points(const float* pts, int64_t n, const float* T_CW, const float* depth, int32_t F, int32_t H, int32_t W,
                        float fx, float fy, float cx, float cy, float trunc, int32_t* count, uint8_t* mask, int64_t* n_seen,
                        void* stream);

/* ---- narrow-band selection for surface extraction -----------------------------------
 * Which points of a D0 x D1 x D2 lattice a scalar field has to be evaluated at so that isdf_marching_cubes of the result
 * equals isdf_marching_cubes of the dense grid: coarse to fine, strides coarse, coarse / 2, ..., 2.  A cell of stride s has its
 * corners on the stride-s lattice, the far ones clipped to the last index of each axis (ragged grids and grids smaller than one
 * coarse cell work); with (di, dj, dk) its clipped extents and a_rc the affine (the identity without has_transform),
 *   w_r = fma(a_r2, dk, fma(a_r1, dj, a_r0 * di)),   d = sqrt(fma(w_2, w_2, fma(w_1, w_1, w_0 * w_0)))        (fp32).
 * A cell is KEPT iff a corner value is not finite, or its corners are not all on one side of level (inside iff value < level,
 * as marching cubes has it), or max over the corners of |f - level| <= slack * d, compared in fp32.  Every cell of stride
 * `coarse` is tested; the children (2c .. 2c + 1 per axis) of kept cells are tested at the next stride.  At the end every
 * lattice point of [2c - 1, 2c + 3] per axis around a kept stride-2 cell c, clipped to the grid, is evaluated: the cell and
 * the one-point halo that the central-difference normals of marching cubes read.  Everything else stays NaN, and marching
 * cubes skips it.  If the field is L-Lipschitz in world units and slack >= L, no sign-changing cell is lost and the mesh is the
 * dense one bit for bit.
 *
 * The caller drives the levels, since the field is evaluated in between (for the network: isdf_sdf_eval):
 *   begin;  for s = coarse, ..., 2:  select(s) -> n, emit(s), values = field(points), update(s);
 *   select(1) -> n, emit(1), values = field(points), update(1);  leaks.
 * The volume marks "not evaluated" with one NaN bit pattern (0x7fe15df0); a field value with these very bits is stored as the
 * default NaN.  No atomic decides a position and all counts are integer sums: two runs give the same bytes.  The workspace
 * needs no initialisation; it carries the kept flags from level to level, so one workspace serves one volume at a time.
 * Every call: ISDF_EINVAL for a NULL args / volume / counts, a dimension < 2 or D0*D1*D2 > 2^31 - 1, coarse not a power of two
 * >= 2, slack negative or not finite, level or the affine not finite, a stride that is not a power of two in [1, coarse];
 * ISDF_EWORKSPACE for a workspace that is NULL or too small.                                                              */
typedef struct isdf_band_args {
  int32_t D0, D1, D2;         /* lattice points per axis, volume[i][j][k] row-major          */
  int32_t coarse;             /* coarsest stride, a power of two >= 2                        */
  float level, slack;
  int32_t has_transform;
  int32_t reserved;
  float index_to_world[12];   /* rows of the 3x4 affine (used iff has_transform)             */
  const float* points;        /* optional device [D0*D1*D2][3]: emit gathers from it instead of applying the affine */
} isdf_band_args;

/* up(x) = x rounded up to 256, c_a(s) = ceil((D_a - 1) / s), nb = ceil(D0*D1*D2 / 256):
 *   sum over s = 2, 4, ..., coarse of up(c_0(s) * c_1(s) * c_2(s))  +  up(8 * nb)  +  up(16 * nb)  +  256
 * (the kept flags per stride, the per-block sums and their offsets).  ISDF_EINVAL for dims / coarse outside the bounds above. */
int64_t isdf_band_ws_bytes(int32_t D0, int32_t D1, int32_t D2, int32_t coarse);

/* volume [D0][D1][D2] <- "not evaluated" everywhere.  One launch. */
int isdf_band_begin(const isdf_band_args* args, float* volume, void* stream);

/* counts[0] (device int64[2]) <- the points stride `stride` needs that are not evaluated yet: the corners of its candidate cells,
 * or for stride 1 the cells and halos of the kept stride-2 cells.  Two launches. */
int isdf_band_select(const isdf_band_args* args, int32_t stride, const float* volume, int64_t* counts, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* After select at the same stride with the volume unchanged, n = the count it reported: index_out [n] int32 <- the points'
 * linear indices, ascending in the stride's lattice order; pts_out [n][3] <- their positions: points[index] if args->points,
 * else per row r  fma(a_r2, k, fma(a_r1, j, fma(a_r0, i, a_r3)))  -- the chain of isdf_grid_points.  Nothing is written at
 * or past n.  n = 0 is a no-op.  One launch. */
int isdf_band_emit(const isdf_band_args* args, int32_t stride, const float* volume, int32_t* index_out, float* pts_out, int64_t n,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* volume[index[t]] <- values[t] for t < n (indices outside the volume are ignored); then, stride > 1: every cell of the stride
 * is tested, its kept flag stored, counts <- (candidates, kept).  Stride 1 only scatters; counts may be NULL.  Up to three
 * launches. */
int isdf_band_update(const isdf_band_args* args, int32_t stride, float* volume, const int32_t* index, const float* values, int64_t n,
                     int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* counts[0] <- the unit cells with eight evaluated finite corners not all on one side of level that lie in no kept stride-2
 * cell.  They are halo cells, marching cubes will mesh them, and they say the surface left the band: slack was too small.
 * Two launches. */
int isdf_band_leaks(const isdf_band_args* args, const float* volume, int64_t* counts, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* pts_out [D0*D1*D2][3] <- index_to_world (rows of a 3x4 affine, HOST memory, read before the call returns) applied to every
 * lattice point with the chain documented at emit: the dense grid whose values the band's agree with bit for bit. */
int isdf_grid_points(int32_t D0, int32_t D1, int32_t D2, const float* index_to_world, float* pts_out, void* stream);

/* ---- frame-to-map pose alignment ---------------------------------------------------
 * One linearisation of "where was this depth frame really taken?" against the map: the depth pixels of a posed frame are
 * back-projected under the pose guess, the caller evaluates its field (sdf and d sdf / dx, e.g. isdf_sdf_eval) at those world
 * points, and the point-to-SDF residuals, their SE(3) Jacobians and the 6 x 6 normal equations are summed per pose.  Reference:
 * none (the reference takes its poses from a tracker or from robot kinematics and never corrects them).
 *
 * Pixel lattice of a pose: every stride-th row and column from 0: n_pix = ceil(H / stride) * ceil(W / stride) pixels, row-major.
 * B poses per call; pose b reads depth frame frame_of_pose[b], or frame b when frame_of_pose is NULL (then B <= F).
 * A pixel is VALID iff its depth z is finite, != 0, >= min_depth and <= max_depth (max_depth may be +inf).
 *
 * Points (fp32, every operation rounded on its own, no fused multiply-add, IEEE division; c, r the pixel's column and row):
 *   xc = (z * (c - cx)) / fx,  yc = (z * (r - cy)) / fy,  zc = z                       (pointcloud_from_depth_torch, transform.py:189-190)
 *   x_w[i] = ((R[i][0]*xc + R[i][1]*yc) + R[i][2]*zc) + t[i]       with T_WC = [R | t], rows of 4
 *   an invalid pixel gets t itself: finite, so the field call behind it is harmless, and the pixel is never counted.
 *
 * System (ALL arithmetic in double on the fp32 inputs widened; huber and trunc are fp32 and widened too): r = sdf; a point is USED
 * iff its pixel is valid and |r| <= trunc; weight w = 1 if |r| <= huber, else huber / |r|; Huber cost rho = r^2 / 2 if |r| <= huber,
 * else huber * (|r| - huber / 2); Jacobian J = [g, (x - t) x g] (g = grad, x the point): the twist (v, omega) about the camera
 * centre under the update R <- exp(omega^) R, t <- t + v.  Per pose one record of ISDF_POSE_RECORD doubles:
 *   [0] used points   [1] valid pixels   [2] sum w r^2   [3] sum rho   [4..9] sum w r J
 *   [10..30] upper triangle of sum w J J^T, row-major ((0,0) .. (0,5), (1,1) .. (5,5))   [31] sum |r| over the used points
 * Summed in a fixed order (per thread a grid-stride share in ascending order, lanes by shuffle, the four waves in wave order, one
 * partial record per block, the blocks in block order) on a grid that depends on n_pix alone: a pose's record repeats bit for bit
 * from run to run and does not depend on which other poses share the call.
 *
 * T_WC [B][12] (rows of the 3 x 4 pose) and frame_of_pose [B] are HOST arrays, read and checked before the call returns; they
 * travel to the kernels as launch arguments.  Every call: ISDF_EINVAL for a NULL args / depth / T_WC / output / input, B, F, H, W
 * or stride < 1, B > ISDF_POSE_MAX_POSES, H * W > 2^31 - 1, an intrinsic that is not finite, fx or fy == 0, min_depth > max_depth
 * (or either NaN), a pose entry that is not finite, a frame_of_pose entry outside [0, F), B > F without frame_of_pose; the
 * system also for huber or trunc <= 0 or not finite.  ISDF_EWORKSPACE for a workspace that is NULL or too small.  Nothing is
 * launched by a refused call.                                                                                          */
typedef struct isdf_pose_args {
  int32_t B, F, H, W;            /* poses; depth frames and their size                          */
  int32_t stride, reserved;      /* pixel lattice step (>= 1)                                   */
  float fx, fy, cx, cy;
  float min_depth, max_depth;
  const float* depth;            /* device [F][H][W]                                            */
  const float* T_WC;             /* HOST [B][12]                                                */
  const int32_t* frame_of_pose;  /* HOST [B], or NULL: pose b reads frame b                     */
} isdf_pose_args;

#define ISDF_POSE_RECORD 32
#define ISDF_POSE_MAX_BLOCKS 64       /* partial records per pose                               */
#define ISDF_POSE_MAX_POSES 65536

/* workspace bytes of the system call for B poses: B * ISDF_POSE_MAX_BLOCKS * ISDF_POSE_RECORD * 8 (ISDF_EINVAL for B outside
 * [1, ISDF_POSE_MAX_POSES]).  No initialisation needed. */
int64_t isdf_pose_ws_bytes(int32_t B);

/* pts_out [B * n_pix][3] <- the world point of every lattice pixel of every pose.  One launch per 32 poses. */
int isdf_pose_points(const isdf_pose_args* args, float* pts_out, void* stream);

/* records [B][ISDF_POSE_RECORD] (device doubles) <- the sums above from pts [B * n_pix][3], sdf [B * n_pix], grad [B * n_pix][3]
 * (device fp32; validity is re-derived from the depth).  One launch per 32 poses and one closing launch. */
int isdf_pose_system(const isdf_pose_args* args, const float* pts, const float* sdf, const float* grad, float huber, float trunc,
                     double* records, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- planning against the map: batched trajectory optimisation -----------------------
 * One iteration of covariant (CHOMP-style) gradient descent on B trajectories at once: the caller evaluates its field (sdf and
 * d sdf / dx, e.g. isdf_sdf_eval) at the query points of the trajectories, and one launch turns those values into the cost, its
 * gradient, the preconditioned step and the query points of the next iteration.  Reference: none (the reference scores a recorded
 * camera path with metrics.chomp_cost, metrics.py:95-104; it never moves one).
 *
 * B trajectories of T waypoints x[b][t] (world frame, fp32); waypoints 0 and T-1 are fixed, 1 .. T-2 are INTERIOR.  The robot
 * is S body spheres that translate with the waypoint: offset o_s, radius r_s.  No rotation, no kinematics.
 *
 * Query points (fp32, one add per coordinate): q[b][t][s] = x[b][t] + o_s, layout [B][T][S][3].
 *
 * Everything else in double on the fp32 inputs widened (eps, w_obs, w_smooth, eta, max_step, tol are fp32 and widened too),
 * every operation rounded on its own, no fused multiply-add, products and sums in the order written:
 *   sample (t, s), every t, s ascending: BAD iff sdf or one of the three grad values is not finite; a bad sample adds its number
 *     of non-finite values to [8] and nothing else.  Otherwise clearance d = sdf - r_s and
 *       d < 0:          c = -d + eps * 0.5              c' = -1
 *       0 <= d <= eps:  c = ((d - eps) * (d - eps)) / (2 * eps)   c' = (d - eps) / eps
 *       d > eps:        c = 0                           c' = 0                      (metrics.chomp_cost, as eval.hip restates it)
 *   per waypoint: C_t = sum_s c, G_t = sum_s c' * g (g = grad), C_0 = C_{T-1} = 0
 *   velocity, interior t: v_t = (x_{t+1} - x_{t-1}) * 0.5, sigma_t = sqrt((v0 v0 + v1 v1) + v2 v2), vh_t = v_t / sigma_t (0 where
 *     sigma_t == 0; vh_0 = vh_{T-1} = 0)
 *   F_obs = sum_{t=1}^{T-2} C_t * sigma_t          F_smooth = (0.5 * (T-1)) * sum_{t=0}^{T-2} |x_{t+1} - x_t|^2
 *   gradient, interior t (the exact gradient of w_obs F_obs + w_smooth F_smooth in x_t; rows 0 and T-1 are 0):
 *     grad_t = w_obs * (sigma_t * G_t + (C_{t-1} vh_{t-1} - C_{t+1} vh_{t+1}) * 0.5) + (w_smooth * (T-1)) * ((2 x_t - x_{t-1}) - x_{t+1})
 *   step: Delta = -(1 / eta) K^-1 grad per coordinate, K = (T-1) tridiag(-1, 2, -1) over the n = T-2 interior waypoints, by the
 *     closed-form inverse through two ordered prefix sums (i = 1 .. n):
 *       P_i = sum_{j <= i} j grad_j,  Q_i = sum_{j > i} (n+1-j) grad_j  (j ascending / descending),
 *       y_i = ((n+1-i) P_i + i Q_i) / (n+1),  Delta_i = -(y_i / (eta * (T-1)))
 *     m = max_t sqrt((D0 D0 + D1 D1) + D2 D2); kappa = 1 if m <= max_step, else max_step / m (max_step may be +inf)
 *     x_t <- (float)((double)x_t + kappa * Delta_t)
 *
 * State, one int32 per trajectory, in/out: 0 moving, 1 converged, 2 invalid.  On entry with state 0: a bad sample anywhere
 * in the trajectory -> state 2, x untouched; else m < tol -> state 1, x untouched (a converged trajectory's record describes
 * exactly the x it leaves); else the step is applied.  On entry with any other state: x is untouched bit for bit, the state is
 * kept, the record is written with [6] = [7] = 0.
 *
 * Record, ISDF_TRAJ_RECORD doubles per trajectory:
 *   [0] F_obs   [1] F_smooth   [2] min d over the samples that are not bad (+inf if none)   [3] samples with d < 0
 *   [4] samples with d < eps   [5] sum_t |grad_t|^2   [6] m   [7] kappa as applied (0 where no step was taken)
 *   [8] non-finite values among sdf and grad   [9] state after the call   [10] path length sum_t |x_{t+1} - x_t|   [11..15] 0
 * Sums: thread k of 256 takes waypoints k, k + 256, .. in ascending order, lanes by shuffle, the four waves in wave order: an
 * order that depends on T and S alone.  A trajectory's record and its new x repeat bit for bit from run to run and do not
 * depend on which other trajectories share the call.  x must be finite (device data, not checked).
 *
 * offsets [S][3] and radii [S] are HOST arrays, read and checked before the call returns; they travel as launch arguments.
 * Every call: ISDF_EINVAL for a NULL args / x / offsets / radii / output / input (state may be NULL for isdf_traj_points only),
 * B outside [1, ISDF_TRAJ_MAX_TRAJ], T outside [3, ISDF_TRAJ_MAX_WAYPOINTS], S outside [1, ISDF_TRAJ_MAX_SPHERES],
 * B * T * S > 2^31 - 1, an offset that is not finite, a radius that is negative or not finite; the step also for eps, eta or
 * max_step <= 0 or NaN, eps or eta infinite, w_obs, w_smooth or tol negative or not finite.  Nothing is launched by a refused
 * call.                                                                                                                */
#define ISDF_TRAJ_RECORD 16
#define ISDF_TRAJ_MAX_WAYPOINTS 1024
#define ISDF_TRAJ_MAX_SPHERES 32
#define ISDF_TRAJ_MAX_TRAJ 65536

typedef struct isdf_traj_args {
  int32_t B, T, S, reserved;
  float eps, w_obs, w_smooth, eta, max_step, tol;
  float* x;              /* device [B][T][3]; isdf_traj_step updates it in place */
  int32_t* state;        /* device [B]; may be NULL for isdf_traj_points          */
  const float* offsets;  /* HOST [S][3] */
  const float* radii;    /* HOST [S]    */
} isdf_traj_args;

/* q_out [B][T][S][3] <- the query points of x.  One launch. */
int isdf_traj_points(const isdf_traj_args* args, float* q_out, void* stream);

/* One iteration from sdf [B][T][S] and grad [B][T][S][3] (device fp32) at the query points of x: records
 * [B][ISDF_TRAJ_RECORD] (device doubles), grad_out [B][T][3] (device doubles, or NULL) <- grad, x and state updated in place,
 * q_out (or NULL) <- the query points of the x the call leaves, for every trajectory, frozen ones included.  One launch. */
int isdf_traj_step(const isdf_traj_args* args, const float* sdf, const float* grad, double* records, float* q_out, double* grad_out,
                   void* stream);

/* ---- planning for articulated robots: trajectory steps in joint space ------------------
 * isdf_traj_step for a robot that has joints: a serial kinematic chain with collision spheres on its links -- an arm, a free-
 * flying rigid body (three prismatic and three revolute joints), a mobile base with yaw.  The caller evaluates its field at the
 * query points, one launch turns the values into the cost, its exact gradient pulled back through the chain's Jacobian, the
 * preconditioned and projected step, and the query points of the next iteration.  Reference: none.
 *
 * The chain (HOST arrays, read and checked before the call returns; they travel as launch arguments): J joints, joint j = 1 .. J
 * of kind 0 (revolute) or 1 (prismatic), with a fixed transform X_j (3x4 row-major, [R | t]) from the previous link's frame and a
 * unit axis u_j in its own frame; base (3x4) is the world pose of link 0.  S spheres: sphere s sits on link l_s in [0, J] at the
 * local centre o_s with radius r_s.  A sphere on link 0 does not move: it counts in the cost and pulls on no joint.  Optional
 * limits lo_j <= hi_j (fp32, +-inf: none; a NULL array: none for every joint).  Branches and closed loops are not described.
 *
 * B trajectories of T configurations theta[b][t][j] (fp32); rows 0 and T-1 are fixed, 1 .. T-2 are INTERIOR.
 *
 * Everything in double on the fp32 inputs widened, every operation rounded on its own, no fused multiply-add, products and
 * sums in the order written; dot(a, b) = (a0 b0 + a1 b1) + a2 b2, a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 * Frames of one configuration (R: 3x3, rows R_0 R_1 R_2; t: 3), link by link:
 *   (R, t) = base.  For j = 1 .. J:  A = R X_j.R with A[r][c] = dot(R_r, column c of X_j.R);  p_j[r] = dot(R_r, X_j.t) + t[r];
 *     a_j[r] = dot(A_r, u_j)   (the joint's world axis; p_j is its world origin)
 *     revolute:  s = sin(theta_j), c = cos(theta_j), k = 1 - c,
 *       M = [ c + k (u0 u0)       k (u0 u1) - s u2    k (u0 u2) + s u1 ]
 *           [ k (u1 u0) + s u2    c + k (u1 u1)       k (u1 u2) - s u0 ]
 *           [ k (u2 u0) - s u1    k (u2 u1) + s u0    c + k (u2 u2)    ],  R <- A M with R[r][c] = dot(A_r, column c of M), t <- p_j
 *     prismatic: R <- A, t[r] <- p_j[r] + theta_j * a_j[r]
 *   Query points, layout [B][T][S][3]: q[s][r] = (float)(dot(R_r, o_s) + t[r]) under the frame of link l_s.
 *
 * The step, from q (the fp32 query points the field was evaluated at), sdf and grad:
 *   sample (t, s), every t, s ascending: BAD iff sdf or one of the three grad values is not finite; a bad sample adds its number
 *     of non-finite values to [8] and nothing else (its c, c' and r are 0).  Otherwise d = sdf - r_s and c, c' as for
 *     isdf_traj_step; c = c' = 0 at t = 0 and t = T-1.
 *   body-point velocity, interior t: v = (q_{t+1,s} - q_{t-1,s}) * 0.5, sigma = sqrt((v0 v0 + v1 v1) + v2 v2), h = v / sigma (0
 *     where sigma == 0; h = 0 at t = 0 and t = T-1)
 *   F_obs = sum_{t=1}^{T-2} (sum_s c_{t,s} * sigma_{t,s})      F_smooth = (0.5 * (T-1)) * sum_{t=0}^{T-2} sum_j (theta_{t+1,j} - theta_{t,j})^2
 *   workspace force, interior t, sample not bad: r = (sigma * c') * g + (c_{t-1,s} * h_{t-1,s} - c_{t+1,s} * h_{t+1,s}) * 0.5
 *   per link l = 1 .. J, s ascending over the spheres with l_s = l, from 0:  R_l = sum r,  M_l = sum q_{t,s} x r
 *   suffix sums over the links, j = J-1 down to 1:  Rs_J = R_J, Rs_j = Rs_{j+1} + R_j;  Ms_J = M_J, Ms_j = Ms_{j+1} + M_j
 *   revolute:  o_j = dot(a_j, Ms_j - p_j x Rs_j)       prismatic:  o_j = dot(a_j, Rs_j)       (a_j, p_j at waypoint t)
 *   grad_t[j] = w_obs * o_j + (w_smooth * (T-1)) * ((2 theta_{t,j} - theta_{t-1,j}) - theta_{t+1,j}); rows 0 and T-1 are 0.  This
 *     is the exact gradient of w_obs F_obs + w_smooth F_smooth in theta_t with q, sigma and h as functions of theta.
 *   step: y = K^-1 grad per joint exactly as for isdf_traj_step (the same two ordered prefix sums), Delta = -(y / (eta * (T-1))),
 *     z0 = theta + Delta, z = min(max(z0, lo_j), hi_j), Delta' = z - theta; the entry is CUT iff z != z0
 *     m = max_{t,j} |Delta'| (the infinity norm: radians and metres are not mixed into a 2-norm);
 *     kappa = 1 if m <= max_step, else max_step / m;  theta <- (float)((double)theta + kappa * Delta')
 *     A theta inside [lo, hi] stays inside; one outside is moved towards the interval.
 * State and its rules: those of isdf_traj_step.  Record, ISDF_TRAJ_RECORD doubles per trajectory: [0] .. [9] as for
 * isdf_traj_step with the definitions above, [10] the joint-space path length sum_t sqrt(sum_j (theta_{t+1,j} - theta_{t,j})^2)
 * (j ascending), [11] the number of cut entries (0, as [6], for a trajectory that did not enter as moving), [12..15] 0.  [5] =
 * sum_t (sum_j grad_t[j]^2), j ascending.  Sums over t: thread k of 256 takes waypoints k, k + 256, .. in ascending order, lanes
 * by shuffle, the four waves in wave order.  A trajectory's record and its new theta repeat bit for bit from run to run and do not
 * depend on which other trajectories share the call.  theta must be finite (device data, not checked).
 *
 * ISDF_ARM_MAX_WAYPOINTS: the step keeps 2 J doubles per waypoint in LDS (the gradient that becomes the step, and the prefix
 * sums), 16 J T bytes: 48 KB at 8 joints and 384 waypoints, which fits the 64 KB a workgroup gets without an opt-in.
 * ISDF_ARM_MAX_TRAJ: the smallest power of two at which B * T * S can pass 2^31 - 1 at all.
 *
 * Every call: ISDF_EINVAL for a NULL args / theta / base / X / kinds / axes / links / centres / radii / output / input (lo and
 * hi may be NULL; state may be NULL for isdf_arm_points only), B outside [1, ISDF_ARM_MAX_TRAJ], T outside [3,
 * ISDF_ARM_MAX_WAYPOINTS], J outside [1, ISDF_ARM_MAX_JOINTS], S outside [1, ISDF_ARM_MAX_SPHERES], B * T * S > 2^31 - 1, a
 * kind outside {0, 1}, a link outside [0, J], an axis whose fp32 (u0 u0 + u1 u1) + u2 u2 is further than 1e-5 from 1, an entry
 * of X, base or the centres that is not finite, a radius that is negative or not finite, lo_j > hi_j or a NaN limit; the step
 * also for the parameters isdf_traj_step refuses.  Nothing is launched by a refused call.                                  */
#define ISDF_ARM_MAX_JOINTS 8
#define ISDF_ARM_MAX_SPHERES 64
#define ISDF_ARM_MAX_WAYPOINTS 384
#define ISDF_ARM_MAX_TRAJ 131072

typedef struct isdf_arm_args {
  int32_t B, T, J, S;
  float eps, w_obs, w_smooth, eta, max_step, tol;
  float* theta;            /* device [B][T][J]; isdf_arm_step updates it in place */
  int32_t* state;          /* device [B]; may be NULL for isdf_arm_points          */
  const float* base;       /* HOST [12]    */
  const float* X;          /* HOST [J][12] */
  const int32_t* kinds;    /* HOST [J]     */
  const float* axes;       /* HOST [J][3]  */
  const int32_t* links;    /* HOST [S]     */
  const float* centres;    /* HOST [S][3]  */
  const float* radii;      /* HOST [S]     */
  const float* lo;         /* HOST [J], or NULL */
  const float* hi;         /* HOST [J], or NULL */
} isdf_arm_args;

/* q_out [B][T][S][3] <- the query points of theta.  One launch. */
int isdf_arm_points(const isdf_arm_args* args, float* q_out, void* stream);

/* One iteration from q [B][T][S][3], sdf [B][T][S] and grad [B][T][S][3] (device fp32; q: the points the field was evaluated
 * at): records [B][ISDF_TRAJ_RECORD] (device doubles), grad_out [B][T][J] (device doubles, or NULL) <- grad, theta and state
 * updated in place, q_out (or NULL; it may be q itself) <- the query points of the theta the call leaves, for every trajectory,
 * frozen ones included.  One launch, one workgroup per trajectory. */
int isdf_arm_step(const isdf_arm_args* args, const float* q, const float* sdf, const float* grad, double* records, float* q_out,
                  double* grad_out, void* stream);

/* ---- the voxel baseline: TSDF fusion and the exact Euclidean distance transform ------------
 * What the map is compared with (eval/plot_utils.py:108-130 reads a "GPU fusion" result; the reference does not ship the fusion):
 * the posed depth frames fused into a truncated signed distance volume, and the full-range field of an occupancy grid by two
 * Euclidean distance transforms (datasets/sdf_util.py:371-385, sdf_from_occupancy).
 *
 * isdf_tsdf_integrate fuses F posed depth frames into a running (tsdf, weight) pair of fp32 volumes [nx][ny][nz], row-major, k
 * fastest.  The caller owns both and zeroes them before the first call.  For voxel (i, j, k) and frames f = 0 .. F-1 IN INDEX
 * ORDER, every operation rounded to fp32 and nothing fused (a = T_CW[f], camera-from-world, rows of 4):
 *   x = ox + (float)i * sx                                          (y, z alike)
 *   xc = ((a00*x + a01*y) + a02*z) + a03,  yc, zc alike             (the chain of isdf_visible_points)
 *   u = (fx*xc + cx*zc) / zc,  v = (fy*yc + cy*zc) / zc             (IEEE division)
 *   uc = u + 0.5f, vc = v + 0.5f                                    (nearest pixel: pixel c's ray passes through u = c)
 *   inside = uc >= 0 && uc < (float)W && vc >= 0 && vc < (float)H && zc > 0        (NaN and +-inf compare false)
 *   col = (int)uc, row = (int)vc;  d = depth[f][row][col]
 *   ok = inside && d > min_depth && d < max_depth                   (a pixel of 0 or NaN: no measurement)
 *   s = d - zc;  ok = ok && s >= -trunc                             (projective distance along z; occluded voxels are skipped)
 *   t = s < trunc ? s : trunc
 *   where ok:  tsdf = (tsdf*w + t) / (w + 1.0f);  w = fminf(w + 1.0f, max_weight)
 * The order over the frames defines the result: a voxel's frames are never split over workgroups or combined by atomics, so F
 * frames in one call equal the same frames in any sequence of calls, bit for bit, and two runs give the same bytes.  One launch;
 * no workspace.  F = 0 is a no-op that reads nothing.
 * ISDF_EINVAL: a NULL args / tsdf / weight (depth / T_CW too when F > 0), a side < 1 or nx*ny*nz > 2^31 - 1, F < 0, H or W < 1 or
 * H*W > 2^31 - 1, a spacing that is not finite or <= 0, an origin or intrinsic that is not finite, trunc not finite or <= 0,
 * max_weight < 1 or NaN (+inf is allowed), min_depth NaN or < 0.  max_depth may be +inf.  Nothing is launched by a refused call. */
typedef struct isdf_tsdf_args {
  int32_t nx, ny, nz;            /* voxels per axis                                             */
  int32_t F, H, W;               /* depth frames and their size                                 */
  float origin[3], spacing[3];   /* voxel (i, j, k) at origin + (i, j, k) * spacing             */
  float fx, fy, cx, cy;
  float trunc, max_weight;
  float min_depth, max_depth;
  const float* depth;            /* device [F][H][W]                                            */
  const float* T_CW;             /* device [F][4][4], camera-from-world                         */
  float* tsdf;                   /* device [nx][ny][nz], updated in place                       */
  float* weight;                 /* device [nx][ny][nz], updated in place                       */
} isdf_tsdf_args;

int isdf_tsdf_integrate(const isdf_tsdf_args* args, void* stream);

/* Exact squared Euclidean distance transform.  feature u8 [nx][ny][nz] (device); a voxel q is a FEATURE voxel iff
 * (feature[q] != 0) != (invert != 0).  dist2[p] (device int32 [nx][ny][nz]) <- min over the feature voxels q of |p - q|^2 in voxel
 * units, exact; ISDF_EDT_NONE where there is no feature voxel.  Three separable min-plus passes z, y, x:
 *   out[p] = min over q of the line of  in[q] + (p - q)^2,  saturated at ISDF_EDT_NONE
 * (in = 0 at a feature voxel and ISDF_EDT_NONE elsewhere for the first pass): integer arithmetic, so the result equals the brute
 * force minimum over all feature voxels, and sqrt((double)dist2) is scipy.ndimage.distance_transform_edt of the complement bit for
 * bit.  Three launches.  ISDF_EINVAL: a NULL feature / dist2, a side < 1 or > ISDF_EDT_MAX_SIDE.  ISDF_EWORKSPACE: a workspace that
 * is NULL or smaller than isdf_edt_ws_bytes.  No initialisation needed.                                                       */
#define ISDF_EDT_NONE 1073741824      /* 2^30 */
#define ISDF_EDT_MAX_SIDE 1024

/* 2 * up(4 * nx*ny*nz), up(x) = x rounded up to 256: two int32 volumes.  The transform passes through the first; the occupancy
 * field keeps one of its two transforms in the first and passes both through the second.  ISDF_EINVAL for a side outside
 * [1, ISDF_EDT_MAX_SIDE]. */
int64_t isdf_edt_ws_bytes(int32_t nx, int32_t ny, int32_t nz);

int isdf_distance_transform(const uint8_t* feature, int32_t nx, int32_t ny, int32_t nz, int32_t invert, int32_t* dist2,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* sdf_from_occupancy (sdf_util.py:371-385): with a = dist2 to the nearest occupied voxel (occ != 0) and b = dist2 to the nearest
 * free one, both by the transform above,
 *   out[p] = (float)((sqrt((double)a) - sqrt((double)b)) * voxel)            (correctly rounded double square roots; device fp32)
 * positive in free space.  No occupied voxel anywhere: +inf everywhere; no free voxel: -inf (the reference's result is
 * meaningless there).  Seven launches.  ISDF_EINVAL as for the transform, and for a voxel that is not finite or <= 0. */
int isdf_occupancy_sdf(const uint8_t* occ, int32_t nx, int32_t ny, int32_t nz, double voxel, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ---- ground truth from a triangle mesh: distance to the nearest triangle and generalised winding number -------------------
 * What the reference builds offline with trimesh (datasets/sdf_util.py:388-457: voxelise, fill, two distance transforms), exact
 * instead: for every query point the distance to the nearest triangle of the mesh, and the winding number of the mesh around the
 * point, which gives the sign on open and non-manifold meshes as well as on closed ones.  Brute force over points x triangles.
 *
 * isdf_tri_pack gathers vertices [nv][3] f32 and faces [m][3] i32 (device) once into `packed`: S = m rounded up to ISDF_TRI_TILE
 * slots of ISDF_TRI_SLOT_FLOATS floats, slot f for face f (ISDF_TRI_PACKED_BYTES(m) bytes, 16-byte aligned):
 *   [0..2] a   [3] ab.ab   [4..6] ab = b - a   [7] ab.ac   [8..10] ac = c - a   [11] ac.ac   [12..14] b   [15] valid (1 or 0)
 *   [16..18] c   [19] 0   [20..22] nh = n / sqrtf(n.n), three correctly rounded divisions (n below)   [23] 0
 * with every dot product (x*x' + y*y') + z*z' in rounded fp32 operations.  `transform` (HOST, 12 floats, rows of 4, or NULL) maps
 * every vertex first: x' = ((T00*x + T01*y) + T02*z) + T03, y', z' alike.  A face is SKIPPED -- its slot is all zero, and it
 * contributes nothing to any distance or winding number -- if
 *   an index lies outside [0, nv)  (tested before anything is read through it), or a (transformed) vertex coordinate is not
 *   finite:                                                                                       counted in counts[0];
 *   n.n is not > 0 in fp32, n = ab x ac = (aby*acz - abz*acy, abz*acx - abx*acz, abx*acy - aby*acx)   (zero area, a repeated
 *   vertex):                                                                                      counted in counts[1].
 * counts: device int32[2], zeroed by the call.  One launch.  m = 0 packs nothing.
 * ISDF_EINVAL: a NULL counts, nv or m < 0 or > 2^30, a NULL vertices with nv > 0, a NULL faces or packed with m > 0, a transform
 * entry that is not finite.  ISDF_EWORKSPACE: packed_bytes < ISDF_TRI_PACKED_BYTES(m).
 *
 * isdf_tri_distance: pts [n][3] f32 (device) against a packed mesh of m faces.  Per pair of a point p and a valid slot, every
 * operation rounded to fp32 and nothing fused:
 *   ap = p - a
 *   d1 = (abx*apx + aby*apy) + abz*apz      d2 = (acx*apx + acy*apy) + acz*apz
 *   d3 = d1 - ab.ab    d4 = d2 - ab.ac    d5 = d1 - ab.ac    d6 = d2 - ac.ac
 *   vc = d1*d4 - d3*d2    vb = d5*d2 - d1*d6    va = d3*d6 - d5*d4    e43 = d4 - d3    e56 = d5 - d6
 *   (den, nv, nw) = the FIRST line that applies of
 *     d1 <= 0 && d2 <= 0                  (1, 0, 0)                   vertex a
 *     d3 >= 0 && d4 <= d3                 (1, 1, 0)                   vertex b
 *     vc < 0 && d1 >= 0 && d3 <= 0        (d1 - d3, d1, 0)            edge ab
 *     d6 >= 0 && d5 <= d6                 (1, 0, 1)                   vertex c
 *     vb < 0 && d2 >= 0 && d6 <= 0        (d2 - d6, 0, d2)            edge ac
 *     va < 0 && e43 >= 0 && e56 >= 0      (e43 + e56, e56, e43)       edge bc
 *     otherwise                           ((va + vb) + vc, vb, vc)    the face
 *   r = __fdiv_rn(1, den)    v = nv*r    w = nw*r
 *   on the face:  dn = (nhx*apx + nhy*apy) + nhz*apz     dist2 = dn*dn        (the distance to the plane: exactly |dn| and
 *                 exactly 0 in the plane for an axis-aligned face, whose nh is a signed unit vector exactly)
 *   elsewhere:    dx = apx - (abx*v + acx*w)   (dy, dz alike)      dist2 = (dx*dx + dy*dy) + dz*dz
 * (the regions of Ericson, Real-Time Collision Detection 5.1.5, with d3 .. d6 from the packed dot products and the three edge
 * tests strict, so that a projection ON an edge line stays with the face).  The winner is the
 * minimum of dist2 over the valid slots, the LOWEST FACE INDEX on ties (the integer minimum of dist2's bits << 32 | index; a NaN
 * dist2 never wins); then
 *   dist = sqrtf(dist2), correctly rounded    index = the winner's face index    closest = a + (ab*v + ac*w), v and w recomputed as above
 * No valid slot (or m = 0): dist = +inf, index = -1, closest = NaN, winding = 0.
 * Winding number: per pair, with a, b, c the vertices minus the point, in rounded fp32 operations
 *   |a| = __fsqrt_rn((ax*ax + ay*ay) + az*az), the hardware square root, within one ulp  (|b|, |c| alike)    a.b = (ax*bx + ay*by) + az*bz  (b.c, c.a alike)
 *   det = (ax*(by*cz - bz*cy) + ay*(bz*cx - bx*cz)) + az*(bx*cy - by*cx)
 *   omega = 2 * atan2f(det, ((|a|*|b|*|c| + a.b*|c|) + b.c*|a|) + c.a*|b|)
 * summed in a double per point in face order, winding = (float)(sum / (4 pi)).  The faces are split into C(n, m) chunks of whole
 * tiles -- with Q = ceil(n / 1024) and t = ceil(m / ISDF_TRI_TILE):  c = min(max(ceil(1024 / Q), 1), t, 65535)  (1 for n = 0),
 * C = ceil(t / ceil(t / c))  (1 for m = 0) -- a function of n and m alone; a point's chunk sums are added in chunk order, so the
 * winding number repeats bit for bit.  A NULL `winding` selects a kernel without the solid-angle arithmetic.
 * A query point with a non-finite coordinate: dist, closest and winding NaN, index -1.
 * dist, index, closest [n][3], winding: device, each may be NULL.  record: device double[ISDF_TRI_RECORD], required:
 *   [0] sum of dist over the finite points   [1] their number   [2] the number of non-finite points   [3] the largest dist (0
 *   without a finite point)
 * per-block partials in a fixed order, combined in block order by one closing block: the record repeats bit for bit.
 * Four launches at most.  workspace: isdf_tri_ws_bytes, no initialisation needed.
 * ISDF_EINVAL: a NULL record, n or m < 0 or > 2^30, a NULL pts with n > 0, a NULL packed with m > 0.  ISDF_EWORKSPACE: a workspace
 * that is NULL or too small. */
#define ISDF_TRI_TILE 256
#define ISDF_TRI_SLOT_FLOATS 24
#define ISDF_TRI_RECORD 4
#define ISDF_TRI_PACKED_BYTES(m) ((((int64_t)(m) + ISDF_TRI_TILE - 1) / ISDF_TRI_TILE) * ISDF_TRI_TILE * ISDF_TRI_SLOT_FLOATS * 4)

int isdf_tri_pack(const float* vertices, int64_t nv, const int32_t* faces, int64_t m, const float* transform, float* packed,
                  int64_t packed_bytes, int32_t* counts, void* stream);

/* 8*n*(1 + C(n, m)) + 32*ceil(n / 256) + 256: one 64-bit key and C doubles per point, one partial record per 256 points.
 * ISDF_EINVAL for n or m < 0 or > 2^30. */
int64_t isdf_tri_ws_bytes(int64_t n, int64_t m);

int isdf_tri_distance(const float* pts, int64_t n, const float* packed, int64_t m, float* dist, int32_t* index, float* closest,
                      float* winding, double* record, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the same distance at scan scale: a flat tile index, conservative culling, far-field winding number ---------------------
 * isdf_tri_distance visits every pair.  isdf_tri_distance_tiles visits the tiles of ISDF_TRI_TILE triangles that can still hold
 * the nearest one, and returns THE SAME BITS in dist, index, closest and record: the winner is the integer minimum of
 * (dist2's bits << 32 | index), which no visiting order changes, and a tile is left out only when none of its triangles can
 * reach that minimum (the rule and its margin below).  The winding number is a sum over all faces and cannot be culled exactly:
 * a tile far from the query block adds one dipole term instead of its triangles' solid angles, an approximation the caller opts
 * into by beta > 0 and whose error depends on beta and on the order.
 *
 * order: device int32 [n_order], n_order a multiple of ISDF_TRI_TILE: slot indices into `packed`, or -1 for nothing; tile t lists
 * entries [t * ISDF_TRI_TILE, (t + 1) * ISDF_TRI_TILE).  The order is the caller's (a space-filling curve over the centroids, with the
 * few very large faces in tiles of their own, keeps the boxes small); no result of the distance depends on it.  Every valid slot
 * should be listed exactly once: a slot that is not listed is never found, one listed twice counts twice in the winding number.
 *
 * isdf_tri_tiles_build, one workgroup per tile: every entry is tested against [0, S) or -1 before anything is read through it
 * (S as for isdf_tri_pack); order_clean [n_order] receives the entry if it names a VALID slot and -1 otherwise; counts (device
 * int32[2], zeroed by the call): [0] entries that are neither -1 nor inside [0, S), [1] valid slots listed.  tiles: device double
 * [n_order / ISDF_TRI_TILE][ISDF_TRI_TILE_RECORD], over the vertices a, b, c of the tile's valid slots as double:
 *   [0..2] box lo   [3..5] box hi   (the exact float values; +inf / -inf for an empty tile)
 *   [6..8] N = sum of (1/2) (b - a) x (c - a)      [9..11] c = sum of area * ((a + b) + c) / 3, over sum of area    [12] r = max |vertex - c|
 *   [13] sum of area, area = (1/2) |(b - a) x (c - a)|     [14] the number of valid slots     [15] extent: one past the tile's last valid entry
 * the sums in the record kernels' one order (lanes by shuffle halving, the four waves in wave order).  A tile with [14] = 0 is
 * empty and never visited.  One launch.  ISDF_EINVAL: a NULL counts, m < 0 or > 2^30, n_order < 0, > 2^31 - ISDF_TRI_TILE or no
 * multiple of ISDF_TRI_TILE, a NULL order / tiles / order_clean with n_order > 0, a NULL packed with m > 0.
 *
 * isdf_tri_distance_tiles.  qperm: device int32 [n], a permutation of the queries that makes runs of 1024 spatially compact; block
 * g takes entries [1024 g, 1024 g + 1024).  An entry outside [0, n) is skipped and counted, before anything is read or written
 * through it; a query that no entry names gets dist = +inf, index = -1, winding = 0.  THE RULE, per block, in double:
 *   [bl, bh] = the box of the block's finite query points (a block without one visits nothing)
 *   per non-empty tile t with box [tl, th]:   mind = sqrt((gx*gx + gy*gy) + gz*gz),  g_k = max(0, tl_k - bh_k, bl_k - th_k)
 *                                             maxd = sqrt((hx*hx + hy*hy) + hz*hz),  h_k = max(|th_k - bl_k|, |bh_k - tl_k|)
 *   seed = the lowest t with the least maxd: visited first, and staged for the distance
 *   U = the largest running best dist2 (fp32) over the block's finite queries, recomputed after every tile staged for the distance
 *   the other tiles in ascending order: t is staged for the distance iff   mind - ISDF_TRI_TILE_EPS * maxd <= sqrt((double)U)
 * Every triangle of a tile left out is farther than sqrt(U) + EPS * maxd from every query of the block, and the per-pair sequence
 * errs by less than EPS * |p - a| <= EPS * maxd in the distance (fl(p - a) is exact to half an ulp per component, the dot products
 * and the residual add a few ulp of |p - a| each: under 16 * 2^-24 in all, EPS = 2^-16 leaves a factor 16), so its computed dist2
 * exceeds U and cannot win or tie.  A sliver whose normal or weights lose all their digits is outside this bound, as it is outside
 * the documented accuracy of isdf_tri_distance itself.
 * A staged tile is gathered through order_clean (entries tested against [0, S) once more) and passes through the per-pair
 * sequence of isdf_tri_distance, the slot index as the face index.
 * Winding number (winding != NULL): with e_k = max(0, c_k - bh_k, bl_k - c_k), tile t is FAR iff beta > 0 and
 *   sqrt((ex*ex + ey*ey) + ez*ez) >= beta * r        (the whole block decides alike)
 * a far tile adds, per query q in double with d = c - q and r2 = (dx*dx + dy*dy) + dz*dz,   ((Nx*dx + Ny*dy) + Nz*dz) / (r2 * sqrt(r2));
 * a near tile is staged and adds the fp32 solid angles of its valid slots as isdf_tri_distance computes them, in entry order.  The
 * terms are added to the query's double in visiting order (the seed, then ascending): bits repeat from run to run.  beta <= 0:
 * every tile is near, and the sum is isdf_tri_distance's up to the order of summation.  A tile may be staged for the distance, for
 * the winding number, or for both.
 * stats: device int64[4] or NULL, zeroed by the call: [0] tiles staged for the distance, summed over blocks  [1] tiles staged as
 * near  [2] blocks  [3] qperm entries skipped.
 * dist, index, closest, winding may be NULL; record as for isdf_tri_distance, required.  Up to three asynchronous memsets and three
 * launches.  ISDF_EINVAL: a NULL record, n or m < 0 or > 2^30, n_tiles < 0 or > 2^23, a NULL pts or qperm with n > 0, a NULL tiles
 * or order_clean with n_tiles > 0, a NULL packed with m > 0, a beta that is NaN.  ISDF_EWORKSPACE: a workspace that is NULL or
 * smaller than isdf_tri_tiles_ws_bytes(n). */
#define ISDF_TRI_TILE_RECORD 16
#define ISDF_TRI_TILE_EPS (1.0 / 65536.0)

int isdf_tri_tiles_build(const float* packed, int64_t m, const int32_t* order, int64_t n_order, double* tiles, int32_t* order_clean,
                         int32_t* counts, void* stream);

/* 16*n + 32*ceil(n / 256) + 256: one 64-bit key and one double per point, one partial record per 256 points.  ISDF_EINVAL for
 * n < 0 or > 2^30. */
int64_t isdf_tri_tiles_ws_bytes(int64_t n);

int isdf_tri_distance_tiles(const float* pts, int64_t n, const int32_t* qperm, const float* packed, int64_t m, const double* tiles,
                            const int32_t* order_clean, int64_t n_tiles, double beta, float* dist, int32_t* index, float* closest,
                            float* winding, double* record, int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- routing through the map: geodesic distance field of a free-space mask and the path down it --------------------------
 * The global half of planning (the local half is isdf_traj_step, which deforms a seed and cannot change which side of an obstacle
 * it passes): shortest routes over the free voxels of a grid.  The reference has no counterpart.  Volumes are [nx][ny][nz],
 * row-major, k fastest; `free` is u8 (non-zero = free), distances are int32; at most ISDF_ROUTE_MAX_VOXELS voxels.
 *
 * The graph.  Voxels are 26-connected with the integer chamfer weights <3, 4, 5>: w(p, q) = 3 for a face neighbour (one
 * coordinate differs), 4 for an edge neighbour (two), 5 for a corner neighbour (three).  A move p -> q exists iff both voxels are
 * inside the grid and free; there is no separate corner-cutting rule (the safety margin belongs to the mask).  dist[p] is the
 * cost of the cheapest path from p to any goal, ISDF_ROUTE_NONE where p is blocked or no goal can be reached.  A simple path
 * costs at most 5 * ISDF_ROUTE_MAX_VOXELS < ISDF_ROUTE_NONE: nothing saturates.
 *
 * isdf_route_init: dist <- ISDF_ROUTE_NONE everywhere, then dist <- 0 at every goal (device int32 [n_goals][3], voxel coordinates
 * i, j, k) that is inside the grid and free; other goals are ignored.  n_goals = 0 is allowed (goals may then be NULL).  Two
 * launches at most.
 *
 * isdf_route_relax: `rounds` rounds of two launches each, dist -> workspace -> dist, every launch
 *   out[p] = min(in[p], min over the 26 neighbours q inside the grid of in[q] + w(p, q))     for free p;  blocked p keep NONE
 * applied tile by tile: a workgroup loads ISDF_ROUTE_TILE^3 voxels and their one-voxel halo, repeats the update inside the tile
 * until it stops changing (or a cap is reached) and writes the tile back.  Values only decrease and each is the cost of a real
 * path, so the fixed point is the exact shortest-path distance whatever the tile, cap or number of launches: once a round changes
 * nothing, dist is that fixed point, bit for bit.  changed: device int32 [rounds], zeroed by the call (an asynchronous memset);
 * changed[r] = 1 iff round r lowered any voxel.  No host synchronisation: the caller decides when to look.  dist must come from
 * isdf_route_init (or an earlier relax) on the same mask.
 *
 * isdf_route_trace: B paths, one per start (device int32 [B][3]).  From p = start, step to the FIRST neighbour q, in the order
 *   (di, dj, dk) lexicographic over -1..1 without (0, 0, 0):  (-1,-1,-1), (-1,-1,0), (-1,-1,1), (-1,0,-1), ... , (1,1,1),
 * that lies inside the grid and has dist[q] + w(p, q) == dist[p]; stop at dist == 0.  On a converged field one always exists.
 * path: device int32 [B][max_len], the linear voxel indices (i * ny + j) * nz + k from the start to the goal; len: device int32
 * [B], the number of voxels including both ends; 0 for a start that is outside the grid, blocked or unreachable; -1 if max_len
 * is too small or no neighbour matches (a field that was not converged) -- the voxels found so far stay in path, and nothing is
 * written past max_len.  A path of cost c has at most c / 3 + 1 voxels.  One launch, one wave per path.
 *
 * ISDF_EINVAL, before anything is launched: a NULL free / dist / changed / starts / path / len (goals when n_goals > 0), a side
 * < 1, more than ISDF_ROUTE_MAX_VOXELS voxels, rounds < 1, n_goals or B < 0, max_len < 1.  ISDF_EWORKSPACE: a workspace that is
 * NULL or smaller than isdf_route_ws_bytes. */
#define ISDF_ROUTE_NONE 1073741824          /* 2^30 */
#define ISDF_ROUTE_MAX_VOXELS 134217728     /* 2^27 */
#define ISDF_ROUTE_TILE 8

int isdf_route_init(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, const int32_t* goals, int32_t n_goals, int32_t* dist,
                    void* stream);

/* up(4 * nx*ny*nz), up(x) = x rounded up to 256: one int32 volume, the ping-pong partner of dist.  ISDF_EINVAL for a side < 1 or
 * more than ISDF_ROUTE_MAX_VOXELS voxels. */
int64_t isdf_route_ws_bytes(int32_t nx, int32_t ny, int32_t nz);

int isdf_route_relax(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, int32_t* dist, void* workspace,
                     int64_t workspace_bytes, int32_t rounds, int32_t* changed, void* stream);

int isdf_route_trace(const int32_t* dist, int32_t nx, int32_t ny, int32_t nz, const int32_t* starts, int32_t B, int32_t max_len,
                     int32_t* path, int32_t* len, void* stream);

/* ---- where to look next: frontier voxels, their connected components, and the view gain of a camera pose -----------------
 * The map is incomplete; these calls say where its boundary is and how much unknown space a candidate pose would see.  The
 * reference has no counterpart.  A STATE volume is u8 [nx][ny][nz], row-major, k fastest: ISDF_VOXEL_UNKNOWN, ISDF_VOXEL_FREE, and
 * any value >= ISDF_VOXEL_OCCUPIED is occupied.  Dims follow routing's rule (every side >= 1, at most ISDF_ROUTE_MAX_VOXELS
 * voxels).  p = (i * ny + j) * nz + k is a voxel's linear index.  Every output is an integer or one float32 produced by the
 * sequence stated below: results are compared bit for bit and do not depend on the run.
 *
 * isdf_frontier_init: label[p] (device int32 [nx][ny][nz]) <- p where p is a frontier voxel, ISDF_FRONTIER_NONE elsewhere.  p
 * is a frontier voxel iff state[p] == ISDF_VOXEL_FREE and at least one of its six face neighbours INSIDE the grid is
 * ISDF_VOXEL_UNKNOWN; the outside of the grid is not unknown.  One launch.
 *
 * isdf_frontier_relax: `rounds` rounds of two launches each, label -> workspace -> label, every launch
 *   out[p] = min(in[p], min over the 26 neighbours q inside the grid of in[q])     for in[p] < NONE;  NONE stays NONE
 * applied tile by tile as isdf_route_relax applies its update (ISDF_ROUTE_TILE^3 voxels and a one-voxel halo, repeated inside the
 * tile until it stops changing or a cap is reached).  Every value written is the index of a voxel of the same 26-connected
 * component of frontier voxels and values only decrease, so the fixed point is THE LEAST LINEAR INDEX OF THE COMPONENT, whatever
 * the tile, cap or number of launches.  changed: device int32 [rounds], zeroed by the call; changed[r] = 1 iff round r lowered
 * any label.  No host synchronisation.
 *
 * isdf_frontier_clusters: a frontier voxel is one with 0 <= label[p] < NONE; q = label[p] is its root when q < nx*ny*nz and
 * label[q] == q; a frontier voxel whose label is not a root is an ORPHAN (there is none on converged labels) and joins no record.
 * counts (device int32 [3]) <- the number of roots, of frontier voxels, of orphans.  When roots <= max_clusters:
 * records (device int64 [max_clusters][ISDF_FRONTIER_RECORD]), one row per root IN ASCENDING ORDER OF THE ROOT'S INDEX (positions
 * from prefix sums, no atomic decides one):
 *   root, count, sum_i, sum_j, sum_k, min_i, min_j, min_k, max_i, max_j, max_k, 0
 * over the voxels of the root (integer atomics: sums, minima and maxima of integers are exact whatever the order).  Rows past
 * the number of roots are not written.  With more roots than max_clusters the counts are written and the records are not: the
 * caller sizes the records from counts[0] and calls again.  Four launches at most; max_clusters = 0 (records may be NULL) counts
 * only.
 *
 * isdf_view_gain: B camera-to-world poses T_WC (device float [B][4][4], rows of 4), one ray per pixel (r, c) of an H x W image.
 * origin, spacing: HOST float[3], voxel (i, j, k) centred at origin + (i, j, k) * spacing and covering [a - 0.5, a + 0.5) per axis
 * in index coordinates.  All float32, every operation rounded on its own, nothing fused, IEEE division (T = T_WC[b]):
 *   ray     x = ((float)c - cx) / fx,  y = ((float)r - cy) / fy                  (the reference's ray_dirs_C; t is z-depth)
 *           dW_a = (T[a][0]*x + T[a][1]*y) + T[a][2];   e_a = T[a][3]
 *           g0_a = (e_a - origin_a) / spacing_a;        dg_a = dW_a / spacing_a
 *           any of g0, dg not finite: the ray MISSES (count 0, depth 0, no bits) -- a NaN pose is data, not an error
 *   clip    t0 = t_min, t1 = t_max;  per axis a = 0, 1, 2 with n_a the side and hi_a = (float)n_a - 0.5f:
 *             dg_a == 0:  miss if g0_a < -0.5f or g0_a >= hi_a
 *             otherwise   ta = (-0.5f - g0_a) / dg_a,  tb = (hi_a - g0_a) / dg_a,
 *                         t0 = max(t0, min(ta, tb)),   t1 = min(t1, max(ta, tb))
 *           miss unless t0 < t1
 *   start   c_a = (int)clamp(floorf((g0_a + t0*dg_a) + 0.5f), 0, (float)(n_a - 1))          (clamped before the cast)
 *           step_a = dg_a > 0 ? 1 : -1;   inv_a = 1.0f / dg_a
 *           tMax_a = (((float)c_a + 0.5f*(float)step_a) - g0_a) * inv_a,  +inf where dg_a == 0 (0 is never multiplied by inf);
 *           tMax_a is RECOMPUTED FROM THE CELL by this formula after every step of axis a, never accumulated
 *   walk    t_in = t0; at most nx + ny + nz times:
 *             s = state[c];  s == UNKNOWN: count the voxel and set its bit;  s >= OCCUPIED: depth = t_in, stop
 *             axis = the a with the least tMax_a, the lowest a on ties (y iff tMax_y < tMax_x; z iff tMax_z < the lesser of them)
 *             t_in = tMax_axis;  stop unless t_in < t1;  c_axis += step_axis;  stop if the cell left the grid
 * unknown (device int32 [B][H][W]) <- the count; depth (device float [B][H][W]) <- the z-depth at which the ray enters its first
 * occupied voxel, 0 without one (a depth image of the voxel map).  distinct (device int32 [B], or NULL) <- the number of DISTINCT
 * unknown voxels the rays of view b pass, through a bitmap of ceil(nx*ny*nz / 32) words per view in the workspace: zeroed by the
 * call, set with atomic OR, counted by a popcount launch (integer atomics only).  distinct == NULL needs no workspace.  B = 0 is a
 * no-op.  One launch, three with distinct; no host synchronisation.
 *
 * ISDF_EINVAL, before anything is launched: a NULL state / label / changed / counts / origin / spacing (records when
 * max_clusters > 0; T_WC / unknown / depth when B > 0), a side < 1, more than ISDF_ROUTE_MAX_VOXELS voxels, rounds < 1,
 * max_clusters < 0, B < 0, H or W < 1 (or H*W, or B * ceil(H/8) * ceil(W/8), beyond 2^31 - 1), a spacing that is not finite or
 * <= 0, an origin that is not finite, fx or fy zero, an intrinsic that is not finite, t_min < 0 or NaN, t_max <= t_min or NaN
 * (+inf is allowed).  ISDF_EWORKSPACE: a workspace that is NULL or smaller than the size query says (isdf_view_gain: only with
 * distinct and B > 0). */
#define ISDF_VOXEL_UNKNOWN 0
#define ISDF_VOXEL_FREE 1
#define ISDF_VOXEL_OCCUPIED 2
#define ISDF_FRONTIER_NONE 1073741824       /* 2^30 */
#define ISDF_FRONTIER_RECORD 12             /* int64 per cluster */

int isdf_frontier_init(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t* label, void* stream);

/* up(4 * n) + up(4 * ceil(n / 256)), n = nx*ny*nz, up(x) = x rounded up to 256: one int32 volume (the ping-pong partner of label
 * for isdf_frontier_relax, the roots' slots for isdf_frontier_clusters) and one int32 per 256 voxels (the prefix sums).
 * ISDF_EINVAL for a side < 1 or more than ISDF_ROUTE_MAX_VOXELS voxels. */
int64_t isdf_frontier_ws_bytes(int32_t nx, int32_t ny, int32_t nz);

int isdf_frontier_relax(int32_t* label, int32_t nx, int32_t ny, int32_t nz, void* workspace, int64_t workspace_bytes, int32_t rounds,
                        int32_t* changed, void* stream);

int isdf_frontier_clusters(const int32_t* label, int32_t nx, int32_t ny, int32_t nz, void* workspace, int64_t workspace_bytes,
                           int32_t max_clusters, int32_t* counts, int64_t* records, void* stream);

/* up(4 * B * ceil(nx*ny*nz / 32)): the B bitmaps of isdf_view_gain's distinct count.  ISDF_EINVAL for bad dims or B < 0. */
int64_t isdf_view_gain_ws_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t B);

int isdf_view_gain(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, const float* origin, const float* spacing,
                   const float* T_WC, int32_t B, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float t_min, float t_max,
                   int32_t* unknown, float* depth, int32_t* distinct, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISDF_HIP_H */
