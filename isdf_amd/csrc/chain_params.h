// Kernel-argument structs shared by the launchers (capi.hip) and the kernels.
#pragma once
#include "isdf_common.h"
#include "chain_debug.h"

namespace isdf {

struct ChainParams {
  NetLayout lay;
  isdf_loss_cfg loss;
  const float* params;
  const uint16_t* shadow;
  const float* pts;           // [P,3]
  const float* noise;         // [P] or null
  float noise_std; uint64_t noise_seed, noise_off;   // in-kernel Philox noise when noise == null
  const int32_t* n_valid;     // device: rays (points = n_valid*S); null -> n_points_host
  int64_t n_points_host;
  int64_t pts_capacity;       // points the `pts` buffer holds (train: max_rays * S; forward only: n_points_host): what a workgroup may
                              // request BEFORE it knows n_valid -- the tile's descriptor is clipped to it (chain.hip prologue)
  int32_t S;
  // per-ray inputs (train)
  const float* z_vals; const float* depth; const float* dirsC; const float* dirsW; const float* normals;
  const float* pc_bounds; const float* pc_grad_vec;
  // outputs
  float* sdf; float* sdf_grad; float* tot_loss_mat;
  float* tot_ws;              // [maxPts] per-point total loss (train)
  float* wg_loss;             // [nTiles][8]
  float* vec_part;            // [nTiles][vecStride] bias / out-layer gradient partials (no atomics)
  int32_t vecStride;
  uint16_t* spill; SpillLayout sp;
  float* pe_aux;              // [nTiles*TILE_PTS][8] (train): x' (3), pad, gbar in x' space (3), pad -- what the dW kernel rebuilds the two
                              // embedding-shaped operands (the embedding itself and Ebar = J_pe gbar) from instead of reading them back
  int32_t n_cu;               // compute units of the device the launch goes to (set by launch_chain): dispatch round of a workgroup = blockIdx / n_cu
  ChainDebug dbg;             // empty in the shipped build (chain_debug.h)
};

struct DwParams {
  NetLayout lay;
  SpillLayout sp;
  const uint16_t* spill;
  const float* pe_aux;   // [nTiles*TILE_PTS][8], written by the chain kernel (ChainParams::pe_aux)
  const int32_t* n_valid; int64_t n_points_host; int32_t S;
  int32_t cap_tiles;     // tiles the spill and pe_aux buffers hold (WorkspaceLayout::nTiles): a K-split's first tile is requested before
                         // n_valid is known, through descriptors that are empty for a tile index at or beyond it (dw.hip prologue)
  float* dwPart;   // [dw_total_slabs][256*256] (isdf_common.h)
};

// ---- the step tail (optim.hip): capi.hip fills TailParams by field name, the launchers add what they derive (AdamwCoef, the grid
// split) and pass it to step_tail_kernel by value -- field order and types ARE the kernel argument
struct AdamwHyper { float lr, b1, b2, eps, wd; int step; };   // one AdamW step's hyper-parameters (host side)
struct AdamwCoef { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; };
struct FinalizeArgs {
  const float* wg_loss; int64_t maxTiles; const int32_t* n_valid; int S; const float* tot_ws;
  const int64_t *ib, *ih, *iw; int n_frames, H, W;
  float *loss_sums, *block_loss, *block_cnt;
  // optional (single-GPU tail only): the per-frame averages of loss.frame_avg written straight away --
  // loss_approx [F,8,8] and frame_avg[fa_index ? fa_index[f] : f] (the keyframe store's frame_avg_losses)
  float *la_out, *fa_out; const int32_t* fa_index;
  int fa_inline_n; int32_t fa_inline[8];     // the same index list as kernel arguments (isdf_optim_args.frame_avg_index_inline)
  // optional: loss sums mirrored into pinned host memory; caller-owned tail of the reduction message
  float* mailbox; float* extra; int n_extra, extra_slot; float extra_value;
};
static_assert(ISDF_MAX_INLINE_FRAMES == 8, "FinalizeArgs::fa_inline holds isdf_optim_args.frame_avg_index_inline");
// phase 0 (single GPU): everything.  phase 1: grad + fin only, the optimiser fields stay zero.  phase 2 (launch_adamw_pack):
// params/m/v/shadow + count_ptr, grad = the reduced gradient; of fin the bins, frame-average outputs, loss_sums/extra/mailbox
struct TailParams {
  NetLayout lay;
  const float* dwPart; const float* vecPart; int32_t vecStride;
  float* grad;                       // [n_params] summed gradient (still written: reduce_buf contract)
  float *params, *m, *v; uint16_t* shadow;
  AdamwCoef c; float grad_scale;     // gradient = sum * grad_scale / (n_valid * S)   [PHASE 0]
  const float* count_ptr;            // PHASE 2: gradient = grad[] * grad_scale / *count_ptr (reduced count)
  FinalizeArgs fin;
  int nW, nV;                        // blocks of the weight and the vector sections
  int wBlock0;                       // first weight block of this launch (a split tail runs the weight section in two launches)
};

}  // namespace isdf
