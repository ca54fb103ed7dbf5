// extern "C" entry points declared in include/isdf_hip.h: argument validation,
// layout computation and kernel launches.  No allocation, no synchronisation,
// no global state.
#include <cstdio>
#include "isdf_common.h"
#include "chain_params.h"
#include "launchers.h"

using namespace isdf;

namespace isdf { thread_local int g_isdf_last_hip_error = 0; }

extern "C" {

int isdf_abi_version(void) { return ISDF_ABI_VERSION; }

static thread_local int g_isdf_last_collective_error = 0;

const char* isdf_error_string(int code) {
  switch (code) {
    case ISDF_OK: return "ok";
    case ISDF_EINVAL: return "invalid argument";
    case ISDF_EUNSUPPORTED: return "unsupported configuration (the tile kernels take hidden_feature_size <= 512 (zero-padded to 256 / 512), n_freqs = n_embed_funcs+1 in 1..12, any hidden_layers_block up to 7; bounds_method ray|pc)";
    case ISDF_EWORKSPACE: return "workspace too small";
    case ISDF_EHIP: {
      static thread_local char buf[160];
      snprintf(buf, sizeof(buf), "HIP runtime error: %s", g_isdf_last_hip_error ? hipGetErrorString((hipError_t)g_isdf_last_hip_error) : "(no launch status recorded)");
      return buf;
    }
    case ISDF_ECOLLECTIVE: {
      static thread_local char buf[96];
      snprintf(buf, sizeof(buf), "the collective library refused the all-reduce (ncclResult_t %d)", g_isdf_last_collective_error);
      return buf;
    }
  }
  return "unknown error";
}

int isdf_check_net(const isdf_net_cfg* net) {
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  return layout_supported(l) ? ISDF_OK : ISDF_EUNSUPPORTED;
}

int64_t isdf_param_count(const isdf_net_cfg* net) {
  NetLayout l; int rc = make_layout(net, &l);
  return rc ? rc : l.n_params;
}

int64_t isdf_shadow_bytes(const isdf_net_cfg* net) {
  NetLayout l; int rc = make_layout(net, &l);
  return rc ? rc : l.shadowElems * 2;
}

int64_t isdf_workspace_bytes(const isdf_net_cfg* net, int64_t max_points, int32_t train) {
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (max_points < 0) return ISDF_EINVAL;
  WorkspaceLayout w; make_workspace(l, max_points, max_points, train != 0, &w);
  return w.totalBytes;
}

int64_t isdf_reduce_floats(const isdf_net_cfg* net, int32_t n_frames) {
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  return reduce_layout(l, n_frames).total;
}

int64_t isdf_reduce_split_floats(const isdf_net_cfg* net) {
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  return l.offW[l.cat];    // cat_layer.0.weight: everything from here on is final at isdf_step_out.split_event
}

int isdf_pack_weights(const isdf_net_cfg* net, const float* params, void* shadow, void* stream) {
  isdf_clear_stale_hip_error();
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (!params || !shadow) return ISDF_EINVAL;
  return launch_pack(l, params, (uint16_t*)shadow, (hipStream_t)stream);
}

int64_t isdf_sample_scan_bytes(int64_t max_rays) { return max_rays < 1 ? ISDF_EINVAL : sample_scan_bytes(max_rays); }

int isdf_sample_rays(const isdf_sample_args* a, const isdf_sample_out* o, void* scan_ws, int64_t scan_ws_bytes,
                     void* stream) {
  isdf_clear_stale_hip_error();
  if (!a || !o || !a->depth_batch || !a->T_WC_batch || !o->n_valid || !o->indices_b ||
      !o->indices_h || !o->indices_w || !o->depth_sample || !o->dirs_C_sample || !o->dirs_W_sample || !o->z_vals ||
      !o->pc)
    return ISDF_EINVAL;
  if (a->n_inline != 0 && (a->n_inline != a->n_frames || a->n_inline > ISDF_MAX_INLINE_FRAMES)) return ISDF_EINVAL;
  for (int f = 0; f < a->n_inline; ++f)   // inline window indices are host values: reject what would gather in front of the keyframe buffers
    if (a->frame_idx_inline[f] < 0 || (a->normal_batch && a->normal_idx_inline[f] < 0)) return ISDF_EINVAL;
  if (a->n_inline == 0 && (!a->frame_idx || (a->normal_batch && !a->normal_idx))) return ISDF_EINVAL;
  if (a->n_frames < 1 || a->n_rays < 1 || a->H < 1 || a->W < 1 || a->n_strat < 1 || a->n_surf < 0) return ISDF_EINVAL;
  if ((int64_t)a->n_frames * a->n_rays > 0x7fffffff / 64) return ISDF_EINVAL;
  if (a->rng_mode == 0 && (!a->draw_h || !a->draw_w || !a->draw_u || (a->n_surf > 1 && !a->draw_n))) return ISDF_EINVAL;
  if (!scan_ws || scan_ws_bytes < sample_scan_bytes((int64_t)a->n_frames * a->n_rays)) return ISDF_EWORKSPACE;
  return launch_sample_rays(*a, *o, scan_ws, (hipStream_t)stream);
}

int isdf_sdf_eval(const isdf_net_cfg* net, const float* params, const void* shadow, const float* pts,
                  int64_t n_points, const float* noise, float* sdf, float* sdf_grad, void* workspace,
                  int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (!layout_supported(l)) return ISDF_EUNSUPPORTED;
  if (!params || !shadow || !pts || !sdf || n_points < 0) return ISDF_EINVAL;
  if (n_points == 0) return ISDF_OK;
  ChainParams p = {};
  p.lay = l; p.params = params; p.shadow = (const uint16_t*)shadow; p.pts = pts; p.noise = noise;
  p.n_points_host = n_points; p.pts_capacity = n_points; p.S = 1; p.sdf = sdf; p.sdf_grad = sdf_grad;
  const int mode = sdf_grad ? 1 : 0;
  WorkspaceLayout w; make_workspace(l, n_points, 0, false, &w);
  if (mode == 1) {
    if (!workspace || workspace_bytes < w.totalBytes) return ISDF_EWORKSPACE;
    p.spill = (uint16_t*)((char*)workspace + w.offSpill); p.sp = w.sp;
  }
  // (development build only: phase stamps go to the last 4 KB of a caller-provided workspace; no-op in the shipped build)
  chain_debug_from_env(p.dbg, workspace && workspace_bytes >= 4096 ? (char*)workspace + workspace_bytes - 4096 : nullptr);
  return launch_chain(p, mode, w.nTiles, (hipStream_t)stream);
}

// The checks every entry point that takes isdf_optim_args shares; n_frames: the window the inline index list must cover
static bool optim_args_ok(const isdf_optim_args* opt, int32_t n_frames) {
  if (!opt || !opt->params || !opt->exp_avg || !opt->exp_avg_sq || !opt->shadow || opt->step < 1) return false;
  if ((opt->loss_approx == nullptr) != (opt->frame_avg == nullptr)) return false;   // both or neither
  if (opt->frame_avg_inline_n != 0 && (opt->frame_avg_inline_n != n_frames || opt->frame_avg_inline_n > ISDF_MAX_INLINE_FRAMES))
    return false;
  for (int f = 0; f < opt->frame_avg_inline_n; ++f)   // inline indices are host values: a negative one would write in front of frame_avg
    if (opt->frame_avg_index_inline[f] < 0) return false;
  return true;
}

// The optimiser's share of the step tail's block (opt: validated by optim_args_ok).  Returns the hyper-parameters for the launcher.
static AdamwHyper tail_optim(TailParams& t, const isdf_optim_args& opt) {
  t.params = opt.params; t.m = opt.exp_avg; t.v = opt.exp_avg_sq; t.shadow = (uint16_t*)opt.shadow;
  t.grad_scale = opt.grad_scale;
  FinalizeArgs& f = t.fin;
  f.la_out = opt.loss_approx; f.fa_out = opt.frame_avg; f.fa_index = opt.frame_avg_index;
  f.fa_inline_n = opt.frame_avg_inline_n;
  for (int k = 0; k < opt.frame_avg_inline_n; ++k) f.fa_inline[k] = opt.frame_avg_index_inline[k];
  return AdamwHyper{opt.lr, opt.beta1, opt.beta2, opt.eps, opt.weight_decay, opt.step};
}

static int train_step_impl(const isdf_net_cfg* net, const isdf_loss_cfg* loss, const float* params, const void* shadow,
                           const isdf_step_args* a, const isdf_step_out* o, void* workspace, int64_t workspace_bytes,
                           void* stream, const isdf_optim_args* opt) {
  isdf_clear_stale_hip_error();
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (!layout_supported(l)) return ISDF_EUNSUPPORTED;
  if (!loss || !params || !shadow || !a || !o || !workspace || !o->reduce_buf) return ISDF_EINVAL;
  if (!a->pc || !a->z_vals || !a->depth_sample || !a->dirs_C_sample || !a->dirs_W_sample || !a->indices_b ||
      !a->indices_h || !a->indices_w || !a->n_valid)
    return ISDF_EINVAL;
  if (a->max_rays < 1 || a->S < 1 || a->n_frames < 1 || a->H < 8 || a->W < 8) return ISDF_EINVAL;
  // the 8x8 block bins tile the image exactly (the reference's .view(-1, 8, H/8, 8, W/8) raises otherwise, loss.py:208-219)
  if (a->H % 8 != 0 || a->W % 8 != 0 || a->H >= 65536 || a->W >= 65536) return ISDF_EINVAL;
  if (loss->bounds_method != 0 && loss->bounds_method != 1) return ISDF_EUNSUPPORTED;  // "normal" is broken upstream (loss.py:29)
  if (loss->bounds_method == 1 && (!a->pc_bounds || !a->pc_grad_vec)) return ISDF_EINVAL;
  if (loss->loss_type != 0 && loss->loss_type != 1) return ISDF_EINVAL;
  if (loss->grad_weight != 0.f && !a->norm_sample) return ISDF_EINVAL;
  const int64_t maxPts = (int64_t)a->max_rays * a->S;
  if (maxPts > 0x7fffffff) return ISDF_EINVAL;   // the loss stage indexes points with 32-bit arithmetic
  // every argument check sits in front of the first launch: a rejected call leaves workspace and spills untouched
  if (a->extra_floats < 0 || a->extra_floats > 1016 || (a->extra_floats > 0 && (a->extra_slot < 0 || a->extra_slot >= a->extra_floats)))
    return ISDF_EINVAL;
  WorkspaceLayout w; make_workspace(l, maxPts, a->max_rays, true, &w);
  if (workspace_bytes < w.totalBytes) return ISDF_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* wgLoss = (float*)(ws + w.offWgLoss);
  float* dwPart = (float*)(ws + w.offDwPart);
  float* vecPart = (float*)(ws + w.offVecPart);
  float* totLoss = (float*)(ws + w.offTotLoss);
  // every element of reduce_buf is written exactly once below (no memset, no atomics)

  ChainParams p = {};
  p.lay = l; p.loss = *loss; p.params = params; p.shadow = (const uint16_t*)shadow;
  p.pts = a->pc; p.pts_capacity = maxPts; p.noise = a->noise; p.n_valid = a->n_valid; p.S = a->S;
  p.noise_std = a->noise_std; p.noise_seed = a->noise_seed; p.noise_off = a->noise_offset;
  p.z_vals = a->z_vals; p.depth = a->depth_sample; p.dirsC = a->dirs_C_sample; p.dirsW = a->dirs_W_sample;
  p.normals = a->norm_sample; p.pc_bounds = a->pc_bounds; p.pc_grad_vec = a->pc_grad_vec;
  p.sdf = o->sdf; p.sdf_grad = o->sdf_grad; p.tot_loss_mat = o->tot_loss_mat;
  p.tot_ws = totLoss; p.wg_loss = wgLoss; p.vec_part = vecPart; p.vecStride = w.vecStride;
  p.spill = (uint16_t*)(ws + w.offSpill); p.sp = w.sp;
  p.pe_aux = (float*)(ws + w.offPeAux);
  chain_debug_from_env(p.dbg, ws + w.totalBytes - 4096);   // no-op in the shipped build (chain_debug.h)
  hipEvent_t* ev = (hipEvent_t*)o->prof_events;
  if (ev && hipEventRecord(ev[0], st) != hipSuccess) return ISDF_EHIP;
  rc = launch_chain(p, 2, w.nTiles, st);
  if (rc) return rc;
  if (ev && hipEventRecord(ev[1], st) != hipSuccess) return ISDF_EHIP;

  DwParams d = {};
  d.lay = l; d.sp = w.sp; d.spill = p.spill; d.pe_aux = p.pe_aux; d.n_valid = a->n_valid; d.S = a->S; d.cap_tiles = (int32_t)w.nTiles;
  d.dwPart = dwPart;
  rc = launch_dw(d, st);
  if (rc) return rc;
  if (ev && hipEventRecord(ev[2], st) != hipSuccess) return ISDF_EHIP;
  const ReduceLayout r = reduce_layout(l, a->n_frames);
  TailParams t = {};
  t.lay = l; t.dwPart = dwPart; t.vecPart = vecPart; t.vecStride = w.vecStride; t.grad = o->reduce_buf;
  FinalizeArgs& f = t.fin;
  f.wg_loss = wgLoss; f.maxTiles = w.nTiles; f.n_valid = a->n_valid; f.S = a->S; f.tot_ws = totLoss;
  f.ib = a->indices_b; f.ih = a->indices_h; f.iw = a->indices_w; f.n_frames = a->n_frames; f.H = a->H; f.W = a->W;
  f.loss_sums = o->reduce_buf + r.lossSums; f.block_loss = o->reduce_buf + r.blockLoss; f.block_cnt = o->reduce_buf + r.blockCnt;
  f.mailbox = o->host_mailbox; f.extra = o->reduce_buf + r.extra;   // caller-owned tail (extra_floats), right behind isdf_reduce_floats
  f.n_extra = a->extra_floats; f.extra_slot = a->extra_slot; f.extra_value = a->extra_value;
  if (opt) {   // single-GPU tail: slab reduction + AdamW + operand repack + loss/bin finalisation in one launch
    const AdamwHyper hyper = tail_optim(t, *opt);
    rc = launch_step_tail(0, t, &hyper, 0, st);
    if (rc) return rc;
  }
  // two-call / data-parallel form: slab + partial reduction and loss/bin finalisation in ONE launch; the summed
  // gradient then goes to the all-reduce and isdf_adamw.  With o->split_event: TWO launches, the event between them -- the
  // message's suffix (layers from the cat layer up, out layer, loss sums, bins) is final at the event.
  const int parts = opt ? 0 : o->split_event ? 2 : 1;   // (0: the fused tail above was the closing launch)
  for (int part = 1; part <= parts; ++part) {
    rc = launch_step_tail(1, t, nullptr, parts == 1 ? 0 : part, st);
    if (rc) return rc;
    if (parts == 2 && part == 1 && hipEventRecord((hipEvent_t)o->split_event, st) != hipSuccess) return ISDF_EHIP;
  }
  if (ev && hipEventRecord(ev[3], st) != hipSuccess) return ISDF_EHIP;
  return ISDF_OK;
}

int isdf_train_step(const isdf_net_cfg* net, const isdf_loss_cfg* loss, const float* params,
                    const void* shadow, const isdf_step_args* a, const isdf_step_out* o,
                    void* workspace, int64_t workspace_bytes, void* stream) {
  return train_step_impl(net, loss, params, shadow, a, o, workspace, workspace_bytes, stream, nullptr);
}

int isdf_train_step_adamw(const isdf_net_cfg* net, const isdf_loss_cfg* loss, const isdf_step_args* a,
                          const isdf_step_out* o, const isdf_optim_args* opt, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  if (!a || !optim_args_ok(opt, a->n_frames)) return ISDF_EINVAL;
  if (o && o->split_event) return ISDF_EINVAL;   // the fused form has no message to split
  return train_step_impl(net, loss, opt->params, opt->shadow, a, o, workspace, workspace_bytes, stream, opt);
}

int isdf_train_step_finish(const isdf_net_cfg* net, const isdf_optim_args* opt, const float* reduce_buf, int32_t n_frames,
                           int32_t extra_floats, float* host_mailbox, void* stream) {
  isdf_clear_stale_hip_error();
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (!layout_supported(l)) return ISDF_EUNSUPPORTED;
  if (!optim_args_ok(opt, n_frames) || !reduce_buf) return ISDF_EINVAL;
  if (opt->loss_approx && n_frames < 1) return ISDF_EINVAL;
  if (extra_floats < 0 || extra_floats > 1016 || n_frames < 0) return ISDF_EINVAL;
  if (extra_floats > 0 && !host_mailbox) return ISDF_EINVAL;   // the reduced tail has nowhere to go: say so instead of dropping it
  const ReduceLayout r = reduce_layout(l, n_frames);
  float* msg = const_cast<float*>(reduce_buf);   // phase 2 only reads the message
  TailParams t = {};
  t.lay = l; t.grad = msg; t.count_ptr = reduce_buf + r.lossSums + ISDF_LS_COUNT;
  const AdamwHyper hyper = tail_optim(t, *opt);
  FinalizeArgs& f = t.fin;
  f.n_frames = opt->loss_approx ? n_frames : 0;
  f.loss_sums = msg + r.lossSums; f.block_loss = msg + r.blockLoss; f.block_cnt = msg + r.blockCnt;
  f.extra = msg + r.extra; f.n_extra = extra_floats; f.mailbox = host_mailbox;
  return launch_adamw_pack(t, hyper, (hipStream_t)stream);
}

int isdf_allreduce_sum_f32(isdf_nccl_allreduce_fn nccl_all_reduce, void* comm, float* buf, int64_t count, void* stream) {
  if (!nccl_all_reduce || !comm || !buf || count < 1) return ISDF_EINVAL;
  constexpr int kNcclFloat32 = 7, kNcclSum = 0;            // ncclDataType_t / ncclRedOp_t (rccl.h)
  const int rc = nccl_all_reduce(buf, buf, (size_t)count, kNcclFloat32, kNcclSum, comm, stream);
  if (rc != 0) { g_isdf_last_collective_error = rc; return ISDF_ECOLLECTIVE; }
  return ISDF_OK;
}

int isdf_bounds_pc(const int32_t* n_valid, int32_t max_rays, int32_t S, const float* pc, const float* z_vals,
                   const float* depth_sample, const float* surf_pts, int64_t n_surf, float* bounds, float* grad_vec,
                   void* stream) {
  isdf_clear_stale_hip_error();
  if (!n_valid || !pc || !z_vals || !depth_sample || !bounds || !grad_vec || max_rays < 1 || S < 1) return ISDF_EINVAL;
  if (surf_pts && n_surf < 1) return ISDF_EINVAL;
  return launch_bounds_pc(n_valid, max_rays, S, pc, z_vals, depth_sample, surf_pts, n_surf, bounds, grad_vec,
                          (hipStream_t)stream);
}

int isdf_frame_avg(const float* reduce_buf, int64_t n_params, int32_t n_frames, float* loss_approx,
                   float* frame_avg_loss, const int32_t* frame_avg_index, void* stream) {
  isdf_clear_stale_hip_error();
  if (!reduce_buf || !loss_approx || !frame_avg_loss || n_frames < 1 || n_params < 0) return ISDF_EINVAL;
  const ReduceLayout r = reduce_layout(n_params, n_frames);
  return launch_frame_avg(reduce_buf + r.blockLoss, reduce_buf + r.blockCnt, n_frames, loss_approx, frame_avg_loss, frame_avg_index,
                          (hipStream_t)stream);
}

int isdf_estimate_normals(const float* depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                          float* normals, void* stream) {
  isdf_clear_stale_hip_error();
  if (!depth || !normals || H < 1 || W < 1 || fx == 0.f || fy == 0.f) return ISDF_EINVAL;
  return launch_normals(depth, H, W, fx, fy, cx, cy, normals, (hipStream_t)stream);
}

int isdf_render_depth(const int32_t* n_valid, int64_t n_rays_host, int64_t max_rays, int32_t S, const float* z_vals,
                      const float* sdf, const float* depth_sample, float kf_dist_th, float* view_depth,
                      int32_t* below_count, void* stream) {
  isdf_clear_stale_hip_error();
  if (!z_vals || !sdf || !view_depth || S < 1 || max_rays < 1) return ISDF_EINVAL;
  if (!n_valid && (n_rays_host < 0 || n_rays_host > max_rays)) return ISDF_EINVAL;
  return launch_render_depth(n_valid, n_rays_host, max_rays, S, z_vals, sdf, depth_sample, kf_dist_th, view_depth,
                             below_count, (hipStream_t)stream);
}

int isdf_adamw(const isdf_net_cfg* net, float* params, float* exp_avg, float* exp_avg_sq, const float* grad_sum,
               const float* count_ptr, float grad_scale, float lr, float beta1, float beta2, float eps,
               float weight_decay, int32_t step, void* shadow, void* stream) {
  isdf_clear_stale_hip_error();
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (!params || !exp_avg || !exp_avg_sq || !grad_sum || step < 1) return ISDF_EINVAL;
  const AdamwHyper hyper = {lr, beta1, beta2, eps, weight_decay, step};
  if (shadow && layout_supported(l)) {   // update + the four packed operand copies in one launch
    TailParams t = {};
    t.lay = l; t.grad = const_cast<float*>(grad_sum); t.count_ptr = count_ptr; t.grad_scale = grad_scale;
    t.params = params; t.m = exp_avg; t.v = exp_avg_sq; t.shadow = (uint16_t*)shadow;
    return launch_adamw_pack(t, hyper, (hipStream_t)stream);
  }
  rc = launch_adamw(params, exp_avg, exp_avg_sq, grad_sum, count_ptr, grad_scale, hyper, l.n_params, (hipStream_t)stream);
  if (rc || !shadow) return rc;
  return launch_pack(l, params, (uint16_t*)shadow, (hipStream_t)stream);
}

static bool mesh_dims_ok(int32_t D0, int32_t D1, int32_t D2) {
  return D0 >= 2 && D1 >= 2 && D2 >= 2 && (int64_t)D0 * D1 * D2 <= 0x7fffffff;
}

int64_t isdf_mesh_ws_bytes(int32_t D0, int32_t D1, int32_t D2) {
  if (!mesh_dims_ok(D0, D1, D2)) return ISDF_EINVAL;
  return mesh_ws_layout((int64_t)D0 * D1 * D2, nullptr, nullptr, nullptr, nullptr);
}

int isdf_marching_cubes(const isdf_mc_args* a, int64_t* counts, float* verts, float* normals, int64_t max_verts,
                        int32_t* faces, int64_t max_faces, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!a || !a->volume || !counts || !mesh_dims_ok(a->D0, a->D1, a->D2) || max_verts < 0 || max_faces < 0) return ISDF_EINVAL;
  if ((max_verts > 0 && !verts) || (max_faces > 0 && !faces)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_mesh_ws_bytes(a->D0, a->D1, a->D2)) return ISDF_EWORKSPACE;
  float N[9];
  if (a->has_transform) {   // normals: inverse transpose of the affine's 3x3 part (cofactor matrix / determinant)
    const float* m = a->index_to_world;
    auto M = [m](int r, int c) { return (double)m[4 * r + c]; };
    double cof[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        cof[3 * r + c] = M(r1, c1) * M(r2, c2) - M(r1, c2) * M(r2, c1);
      }
    const double det = M(0, 0) * cof[0] + M(0, 1) * cof[1] + M(0, 2) * cof[2];
    if (!(det != 0.0) || !__builtin_isfinite(det)) return ISDF_EINVAL;
    for (int q = 0; q < 9; ++q) N[q] = (float)(cof[q] / det);   // (A^-1)^T = cof(A) / det(A)
  }
  return launch_marching_cubes(a->volume, a->D0, a->D1, a->D2, a->level, a->has_transform ? a->index_to_world : nullptr,
                               a->has_transform ? N : nullptr, counts, verts, normals, max_verts, faces, max_faces, workspace,
                               (hipStream_t)stream);
}

int isdf_mc_tables(int32_t* edge_corners_host, int8_t* tri_table_host) {
  mc_tables_host(edge_corners_host, tri_table_host);
  return ISDF_OK;
}

// ---- rendered views: workspace = z [B*R*S] | pc [B*R*S*3] | sdf [B*R*S] | depth [B*R] | normal points [B*R*3] |
// their sdf [B*R] | gradient [B*R*3] | the input-gradient forward's own workspace for B*R points; 256-byte aligned pieces
struct RenderWs { int64_t z, pc, sdf, depth, npts, nsdf, ngrad, fwd, fwdBytes, total; };

static int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

static int render_ws_layout(const isdf_net_cfg* net, int32_t B, int32_t H, int32_t W, int32_t S, RenderWs* w) {
  if (B < 0 || H < 1 || W < 1 || S < 1) return ISDF_EINVAL;
  NetLayout l; int rc = make_layout(net, &l);
  if (rc) return rc;
  if (!layout_supported(l)) return ISDF_EUNSUPPORTED;
  const int64_t rays = (int64_t)B * H * W, pts = rays * S;
  if ((int64_t)H * W > 0x7fffffff || pts > ((int64_t)1 << 40)) return ISDF_EINVAL;
  WorkspaceLayout fw; make_workspace(l, rays > 0 ? rays : 1, 0, false, &fw);
  int64_t o = 0;
  w->z = o; o = align256(o + 4 * pts);
  w->pc = o; o = align256(o + 12 * pts);
  w->sdf = o; o = align256(o + 4 * pts);
  w->depth = o; o = align256(o + 4 * rays);
  w->npts = o; o = align256(o + 12 * rays);
  w->nsdf = o; o = align256(o + 4 * rays);
  w->ngrad = o; o = align256(o + 12 * rays);
  w->fwd = o; w->fwdBytes = fw.totalBytes; o = align256(o + fw.totalBytes);
  w->total = o;
  return ISDF_OK;
}

int64_t isdf_render_ws_bytes(const isdf_net_cfg* net, int32_t n_views, int32_t H, int32_t W, int32_t n_samples) {
  if (!net) return ISDF_EINVAL;
  RenderWs w; int rc = render_ws_layout(net, n_views, H, W, n_samples, &w);
  return rc ? rc : w.total;
}

int isdf_render_views(const isdf_net_cfg* net, const float* params, const void* shadow, const isdf_render_args* a,
                      float* depth_out, float* normals_out, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!net || !a || !params || !shadow || (!depth_out && !normals_out)) return ISDF_EINVAL;
  const bool given = a->depth_in != nullptr;
  const int S = given ? 1 : a->n_samples;
  RenderWs w; int rc = render_ws_layout(net, a->n_views, a->H, a->W, S, &w);
  if (rc) return rc;
  if (a->n_views == 0) return ISDF_OK;
  if (!a->T_WC || !a->dirs_C || (given && !normals_out)) return ISDF_EINVAL;
  if (!given) {
    if (a->range_mode == ISDF_RANGE_SCALAR) {
      if (!(a->bin_length >= 0.f)) return ISDF_EINVAL;
    } else if (a->range_mode == ISDF_RANGE_DEPTH || a->range_mode == ISDF_RANGE_UPSAMPLE) {
      if (!a->src_depth || a->src_H < 1 || a->src_W < 1) return ISDF_EINVAL;
    } else {
      return ISDF_EINVAL;
    }
    if ((a->rng_mode != 0 && a->rng_mode != 1) || (a->rng_mode == 0 && !a->draw_u)) return ISDF_EINVAL;
  }
  if (!workspace || workspace_bytes < w.total) return ISDF_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int64_t R = (int64_t)a->H * a->W, rays = (int64_t)a->n_views * R;
  const float* depth = a->depth_in;
  if (!given) {
    float* z = (float*)(ws + w.z);
    float* pc = (float*)(ws + w.pc);
    float* sdf = (float*)(ws + w.sdf);
    float* dst = depth_out ? depth_out : (float*)(ws + w.depth);
    if ((rc = launch_render_samples(*a, z, pc, st))) return rc;
    if ((rc = isdf_sdf_eval(net, params, shadow, pc, rays * S, nullptr, sdf, nullptr, nullptr, 0, stream))) return rc;
    if ((rc = launch_render_depth(nullptr, rays, rays, S, z, sdf, nullptr, 0.f, dst, nullptr, st))) return rc;
    depth = dst;
  }
  if (!normals_out) return ISDF_OK;
  float* npts = (float*)(ws + w.npts);
  float* ngrad = (float*)(ws + w.ngrad);
  if ((rc = launch_normal_points(a->T_WC, a->dirs_C, R, rays, depth, npts, st))) return rc;
  if ((rc = isdf_sdf_eval(net, params, shadow, npts, rays, nullptr, (float*)(ws + w.nsdf), ngrad, ws + w.fwd, w.fwdBytes,
                          stream)))
    return rc;
  return launch_normal_finish(a->T_WC, R, rays, ngrad, normals_out, st);
}

// ---- evaluation against ground truth (eval.hip)
static bool gt_volume_ok(const isdf_gt_volume* vol) {
  if (vol->nx < 2 || vol->ny < 2 || vol->nz < 2 || (int64_t)vol->nx * vol->ny * vol->nz > 0x7fffffff) return false;
  for (int k = 0; k < 3; ++k)
    if (!(vol->spacing[k] > 0.f) || !__builtin_isfinite(vol->spacing[k]) || !__builtin_isfinite(vol->origin[k])) return false;
  return true;
}

int isdf_sdf_metrics(const isdf_gt_volume* vol, const float* pts, const float* sdf, int64_t n, int32_t exclude_zero_gt,
                     float oob_fill, double* record, float* gt_out, uint8_t* valid_out, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!vol || !record || n < 0 || (n > 0 && (!pts || !sdf))) return ISDF_EINVAL;
  if (!gt_volume_ok(vol)) return ISDF_EINVAL;
  if (n > 0 && !vol->values) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < ISDF_SDF_METRICS_WS_BYTES) return ISDF_EWORKSPACE;
  return launch_sdf_metrics(*vol, pts, sdf, n, exclude_zero_gt != 0, oob_fill, record, gt_out, valid_out, (double*)workspace,
                            (hipStream_t)stream);
}

int isdf_region_metrics(const isdf_region_args* a, double* records, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!a || !records || a->n < 0 || a->n > ((int64_t)1 << 40)) return ISDF_EINVAL;
  if ((a->vol != nullptr) == (a->gt_in != nullptr)) return ISDF_EINVAL;          // exactly one ground-truth source
  if (a->grad_sets && (!a->sdf_grad || a->gt_in)) return ISDF_EINVAL;
  if (!(a->delta > 0.0) || !__builtin_isfinite(a->delta)) return ISDF_EINVAL;
  if (a->vol) {
    if (!gt_volume_ok(a->vol)) return ISDF_EINVAL;
    for (int k = 0; k < 3; ++k)
      if (!(a->spacing[k] > 0.0) || !__builtin_isfinite(a->spacing[k]) || !__builtin_isfinite(a->origin[k])) return ISDF_EINVAL;
    if (a->n > 0 && !a->vol->values) return ISDF_EINVAL;
  }
  if (a->n > 0 && (!a->pts || !a->sdf)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < ISDF_REGION_METRICS_WS_BYTES) return ISDF_EWORKSPACE;
  return launch_region_metrics(*a, records, (double*)workspace, (hipStream_t)stream);
}

int isdf_nn_distance(const float* query, int64_t n, const float* target, int64_t m, float* dist, int32_t* index,
                     double* dist_sum, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!dist_sum || n < 0 || n > ((int64_t)1 << 40) || (n > 0 && (!query || !target || m < 1 || m > 0xfffffffe))) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < ISDF_NN_WS_BYTES(n)) return ISDF_EWORKSPACE;
  unsigned long long* keys = (unsigned long long*)workspace;
  return launch_nn_distance(query, n, target, m, dist, index, dist_sum, keys, (double*)(keys + n), (hipStream_t)stream);
}

// ---- SDF slice images (slices.hip)
int isdf_slice_images(const float* pts, const float* sdf, int64_t n, const isdf_colormap* cmap, const isdf_gt_volume* vol,
                      float oob_fill, float chomp_eps, uint8_t* pred_rgb, float* gt_out, uint8_t* gt_rgb, float* pred_cost,
                      float* gt_cost, void* stream) {
  isdf_clear_stale_hip_error();
  const bool pred = pred_rgb || pred_cost, gt = gt_out || gt_rgb || gt_cost;
  if (n < 0 || n > ((int64_t)1 << 40) || (!pred && !gt)) return ISDF_EINVAL;
  if (gt && !vol) return ISDF_EINVAL;
  if ((pred_rgb || gt_rgb) && !cmap) return ISDF_EINVAL;
  if ((pred_cost || gt_cost) && !(chomp_eps > 0.f && __builtin_isfinite(chomp_eps))) return ISDF_EINVAL;
  if (cmap && (cmap->n_colors < 1 || cmap->n_colors > ISDF_COLORMAP_MAX_COLORS || !(cmap->range > 0.f) ||
               !__builtin_isfinite(cmap->range) || !__builtin_isfinite(cmap->vmin)))
    return ISDF_EINVAL;
  if (vol && !gt_volume_ok(vol)) return ISDF_EINVAL;
  if (n == 0) return ISDF_OK;
  if ((pred && !sdf) || (gt && (!pts || !vol->values)) || (cmap && (pred_rgb || gt_rgb) && !cmap->lut)) return ISDF_EINVAL;
  // inputs nothing reads are dropped here, so the kernel's tests stay "pointer given = output wanted"
  return launch_slice_images((pred_rgb || gt_rgb) ? cmap : nullptr, gt ? vol : nullptr, pts, pred ? sdf : nullptr, n, oob_fill,
                             chomp_eps, pred_rgb, gt_out, gt_rgb, pred_cost, gt_cost, (hipStream_t)stream);
}

int isdf_plane_points(const float* origin, const float* du, const float* dv, int32_t H, int32_t W, float* pts_out,
                      void* stream) {
  isdf_clear_stale_hip_error();
  if (!origin || !du || !dv || H < 0 || W < 0 || (int64_t)H * W > 0x7fffffff) return ISDF_EINVAL;
  if ((int64_t)H * W == 0) return ISDF_OK;
  if (!pts_out) return ISDF_EINVAL;
  return launch_plane_points(origin, du, dv, H, W, pts_out, (hipStream_t)stream);
}

// ---- visibility against posed depth frames (visible.hip)
int isdf_visible_points(const float* pts, int64_t n, const float* T_CW, const float* depth, int32_t F, int32_t H, int32_t W,
                        float fx, float fy, float cx, float cy, float trunc, int32_t* count, uint8_t* mask, int64_t* n_seen,
                        void* stream) {
  isdf_clear_stale_hip_error();
  if (n < 0 || n > ((int64_t)1 << 38) || F < 0 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff) return ISDF_EINVAL;
  if (F > 0 && n > INT64_MAX / F) return ISDF_EINVAL;                      // the [F, n] mask is indexed in int64
  for (float v : {fx, fy, cx, cy, trunc})
    if (!__builtin_isfinite(v)) return ISDF_EINVAL;
  if (n > 0 && (!count || (F > 0 && (!pts || !T_CW || !depth)))) return ISDF_EINVAL;
  return launch_visible_points(pts, n, T_CW, depth, F, H, W, fx, fy, cx, cy, trunc, count, mask, n_seen, (hipStream_t)stream);
}

// ---- narrow-band selection for surface extraction (band.hip)
static bool band_args_ok(const isdf_band_args* a) {
  if (!a || !mesh_dims_ok(a->D0, a->D1, a->D2)) return false;
  if (a->coarse < 2 || (a->coarse & (a->coarse - 1)) != 0) return false;
  if (!(a->slack >= 0.f) || !__builtin_isfinite(a->slack) || !__builtin_isfinite(a->level)) return false;
  if (a->has_transform)
    for (int q = 0; q < 12; ++q)
      if (!__builtin_isfinite(a->index_to_world[q])) return false;
  return true;
}

// a stride the hierarchy has: a power of two in [lo, coarse]
static bool band_stride_ok(const isdf_band_args* a, int32_t stride, int32_t lo) {
  return stride >= lo && stride <= a->coarse && (stride & (stride - 1)) == 0;
}

int64_t isdf_band_ws_bytes(int32_t D0, int32_t D1, int32_t D2, int32_t coarse) {
  if (!mesh_dims_ok(D0, D1, D2) || coarse < 2 || (coarse & (coarse - 1)) != 0) return ISDF_EINVAL;
  return band_ws_bytes(D0, D1, D2, coarse);
}

int isdf_band_begin(const isdf_band_args* a, float* volume, void* stream) {
  isdf_clear_stale_hip_error();
  if (!band_args_ok(a) || !volume) return ISDF_EINVAL;
  return launch_band_fill(volume, (int64_t)a->D0 * a->D1 * a->D2, (hipStream_t)stream);
}

int isdf_band_select(const isdf_band_args* a, int32_t stride, const float* volume, int64_t* counts, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!band_args_ok(a) || !band_stride_ok(a, stride, 1) || !volume || !counts) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < band_ws_bytes(a->D0, a->D1, a->D2, a->coarse)) return ISDF_EWORKSPACE;
  return launch_band_select(*a, stride, volume, counts, workspace, (hipStream_t)stream);
}

int isdf_band_emit(const isdf_band_args* a, int32_t stride, const float* volume, int32_t* index_out, float* pts_out, int64_t n,
                   void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!band_args_ok(a) || !band_stride_ok(a, stride, 1) || !volume || n < 0) return ISDF_EINVAL;
  if (n == 0) return ISDF_OK;
  if (!index_out || !pts_out) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < band_ws_bytes(a->D0, a->D1, a->D2, a->coarse)) return ISDF_EWORKSPACE;
  return launch_band_emit(*a, stride, volume, index_out, pts_out, n, workspace, (hipStream_t)stream);
}

int isdf_band_update(const isdf_band_args* a, int32_t stride, float* volume, const int32_t* index, const float* values, int64_t n,
                     int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!band_args_ok(a) || !band_stride_ok(a, stride, 1) || !volume || n < 0 || (n > 0 && (!index || !values))) return ISDF_EINVAL;
  if (stride > 1 && !counts) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < band_ws_bytes(a->D0, a->D1, a->D2, a->coarse)) return ISDF_EWORKSPACE;
  return launch_band_update(*a, stride, volume, index, values, n, counts, workspace, (hipStream_t)stream);
}

int isdf_band_leaks(const isdf_band_args* a, const float* volume, int64_t* counts, void* workspace, int64_t workspace_bytes,
                    void* stream) {
  isdf_clear_stale_hip_error();
  if (!band_args_ok(a) || !volume || !counts) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < band_ws_bytes(a->D0, a->D1, a->D2, a->coarse)) return ISDF_EWORKSPACE;
  return launch_band_leaks(*a, volume, counts, workspace, (hipStream_t)stream);
}

int isdf_grid_points(int32_t D0, int32_t D1, int32_t D2, const float* index_to_world, float* pts_out, void* stream) {
  isdf_clear_stale_hip_error();
  if (!mesh_dims_ok(D0, D1, D2) || !index_to_world || !pts_out) return ISDF_EINVAL;
  return launch_grid_points(D0, D1, D2, index_to_world, pts_out, (hipStream_t)stream);
}

// ---- frame-to-map pose alignment (pose.hip)
// everything of isdf_pose_args the host can check: sizes, intrinsics, depth limits, and the two host arrays entry by entry
static bool pose_args_ok(const isdf_pose_args* a) {
  if (!a || !a->depth || !a->T_WC) return false;
  if (a->B < 1 || a->B > ISDF_POSE_MAX_POSES || a->F < 1 || a->H < 1 || a->W < 1 || a->stride < 1) return false;
  if ((int64_t)a->H * a->W > 0x7fffffff) return false;
  for (float v : {a->fx, a->fy, a->cx, a->cy})
    if (!__builtin_isfinite(v)) return false;
  if (a->fx == 0.f || a->fy == 0.f) return false;
  if (!(a->min_depth <= a->max_depth)) return false;                    // also refuses a NaN limit
  if (!a->frame_of_pose && a->B > a->F) return false;
  for (int64_t q = 0; q < (int64_t)a->B * 12; ++q)
    if (!__builtin_isfinite(a->T_WC[q])) return false;
  if (a->frame_of_pose)
    for (int32_t b = 0; b < a->B; ++b)
      if (a->frame_of_pose[b] < 0 || a->frame_of_pose[b] >= a->F) return false;
  return true;
}

// a stride beyond the image selects pixel (0, 0) alone, as the largest in-image stride does: the kernels' ceil(H / stride) then
// never adds past INT_MAX
static isdf_pose_args pose_clamped(const isdf_pose_args* a) {
  isdf_pose_args c = *a;
  const int32_t most = a->H > a->W ? a->H : a->W;
  if (c.stride > most) c.stride = most;
  return c;
}

int64_t isdf_pose_ws_bytes(int32_t B) {
  if (B < 1 || B > ISDF_POSE_MAX_POSES) return ISDF_EINVAL;
  return (int64_t)B * ISDF_POSE_MAX_BLOCKS * ISDF_POSE_RECORD * 8;
}

int isdf_pose_points(const isdf_pose_args* a, float* pts_out, void* stream) {
  isdf_clear_stale_hip_error();
  if (!pose_args_ok(a) || !pts_out) return ISDF_EINVAL;
  return launch_pose_points(pose_clamped(a), pts_out, (hipStream_t)stream);
}

int isdf_pose_system(const isdf_pose_args* a, const float* pts, const float* sdf, const float* grad, float huber, float trunc,
                     double* records, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!pose_args_ok(a) || !pts || !sdf || !grad || !records) return ISDF_EINVAL;
  if (!(huber > 0.f) || !(trunc > 0.f) || !__builtin_isfinite(huber) || !__builtin_isfinite(trunc)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_pose_ws_bytes(a->B)) return ISDF_EWORKSPACE;
  return launch_pose_system(pose_clamped(a), pts, sdf, grad, huber, trunc, records, (double*)workspace, (hipStream_t)stream);
}

// ---- planning against the map (traj.hip)
// everything of isdf_traj_args the host can check: the sizes and the two host arrays entry by entry
static bool traj_args_ok(const isdf_traj_args* a) {
  if (!a || !a->x || !a->offsets || !a->radii) return false;
  if (a->B < 1 || a->B > ISDF_TRAJ_MAX_TRAJ || a->T < 3 || a->T > ISDF_TRAJ_MAX_WAYPOINTS || a->S < 1 || a->S > ISDF_TRAJ_MAX_SPHERES)
    return false;
  if ((int64_t)a->B * a->T * a->S > 0x7fffffff) return false;
  for (int32_t q = 0; q < a->S * 3; ++q)
    if (!__builtin_isfinite(a->offsets[q])) return false;
  for (int32_t s = 0; s < a->S; ++s)
    if (!(a->radii[s] >= 0.f) || !__builtin_isfinite(a->radii[s])) return false;
  return true;
}

// the six parameters of a descent step, isdf_traj_step's and isdf_arm_step's alike
static bool descent_params_ok(float eps, float w_obs, float w_smooth, float eta, float max_step, float tol) {
  for (float v : {w_obs, w_smooth, tol})
    if (!(v >= 0.f) || !__builtin_isfinite(v)) return false;
  return eps > 0.f && eta > 0.f && max_step > 0.f && __builtin_isfinite(eps) && __builtin_isfinite(eta);   // no NaN; max_step may be +inf
}

int isdf_traj_points(const isdf_traj_args* a, float* q_out, void* stream) {
  isdf_clear_stale_hip_error();
  if (!traj_args_ok(a) || !q_out) return ISDF_EINVAL;
  return launch_traj_points(*a, q_out, (hipStream_t)stream);
}

int isdf_traj_step(const isdf_traj_args* a, const float* sdf, const float* grad, double* records, float* q_out, double* grad_out,
                   void* stream) {
  isdf_clear_stale_hip_error();
  if (!traj_args_ok(a) || !a->state || !sdf || !grad || !records) return ISDF_EINVAL;
  if (!descent_params_ok(a->eps, a->w_obs, a->w_smooth, a->eta, a->max_step, a->tol)) return ISDF_EINVAL;
  return launch_traj_step(*a, sdf, grad, records, q_out, grad_out, (hipStream_t)stream);
}

// ---- planning for articulated robots (arm.hip)
// everything of isdf_arm_args the host can check: the sizes and the chain entry by entry
static bool arm_args_ok(const isdf_arm_args* a) {
  if (!a || !a->theta || !a->base || !a->X || !a->kinds || !a->axes || !a->links || !a->centres || !a->radii) return false;
  if (a->B < 1 || a->B > ISDF_ARM_MAX_TRAJ || a->T < 3 || a->T > ISDF_ARM_MAX_WAYPOINTS || a->J < 1 || a->J > ISDF_ARM_MAX_JOINTS ||
      a->S < 1 || a->S > ISDF_ARM_MAX_SPHERES)
    return false;
  if ((int64_t)a->B * a->T * a->S > 0x7fffffff) return false;
  for (int i = 0; i < 12; ++i)
    if (!__builtin_isfinite(a->base[i])) return false;
  for (int32_t i = 0; i < a->J * 12; ++i)
    if (!__builtin_isfinite(a->X[i])) return false;
  for (int32_t j = 0; j < a->J; ++j) {
    if (a->kinds[j] != 0 && a->kinds[j] != 1) return false;
    const float* u = a->axes + j * 3;
    const float n2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    if (!(__builtin_fabsf(n2 - 1.f) <= 1e-5f)) return false;                                              // also refuses NaN
    const float lo = a->lo ? a->lo[j] : -__builtin_inff(), hi = a->hi ? a->hi[j] : __builtin_inff();
    if (!(lo <= hi)) return false;                                                                        // also refuses NaN
  }
  for (int32_t s = 0; s < a->S; ++s) {
    if (a->links[s] < 0 || a->links[s] > a->J) return false;
    for (int k = 0; k < 3; ++k)
      if (!__builtin_isfinite(a->centres[s * 3 + k])) return false;
    if (!(a->radii[s] >= 0.f) || !__builtin_isfinite(a->radii[s])) return false;
  }
  return true;
}

int isdf_arm_points(const isdf_arm_args* a, float* q_out, void* stream) {
  isdf_clear_stale_hip_error();
  if (!arm_args_ok(a) || !q_out) return ISDF_EINVAL;
  return launch_arm_points(*a, q_out, (hipStream_t)stream);
}

int isdf_arm_step(const isdf_arm_args* a, const float* q, const float* sdf, const float* grad, double* records, float* q_out,
                  double* grad_out, void* stream) {
  isdf_clear_stale_hip_error();
  if (!arm_args_ok(a) || !a->state || !q || !sdf || !grad || !records) return ISDF_EINVAL;
  if (!descent_params_ok(a->eps, a->w_obs, a->w_smooth, a->eta, a->max_step, a->tol)) return ISDF_EINVAL;
  return launch_arm_step(*a, q, sdf, grad, records, q_out, grad_out, (hipStream_t)stream);
}

// ---- the voxel baseline: TSDF fusion and the distance transform (fusion.hip)
int isdf_tsdf_integrate(const isdf_tsdf_args* a, void* stream) {
  isdf_clear_stale_hip_error();
  if (!a || !a->tsdf || !a->weight) return ISDF_EINVAL;
  if (a->nx < 1 || a->ny < 1 || a->nz < 1 || (int64_t)a->nx * a->ny > 0x7fffffff || (int64_t)a->nx * a->ny * a->nz > 0x7fffffff)
    return ISDF_EINVAL;
  if (a->F < 0 || a->H < 1 || a->W < 1 || (int64_t)a->H * a->W > 0x7fffffff) return ISDF_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!(a->spacing[k] > 0.f) || !__builtin_isfinite(a->spacing[k]) || !__builtin_isfinite(a->origin[k])) return ISDF_EINVAL;
  for (float v : {a->fx, a->fy, a->cx, a->cy})
    if (!__builtin_isfinite(v)) return ISDF_EINVAL;
  if (!(a->trunc > 0.f) || !__builtin_isfinite(a->trunc)) return ISDF_EINVAL;
  if (!(a->max_weight >= 1.f) || !(a->min_depth >= 0.f)) return ISDF_EINVAL;     // also refuses NaN; max_weight may be +inf
  if (a->F > 0 && (!a->depth || !a->T_CW)) return ISDF_EINVAL;
  return launch_tsdf_integrate(*a, (hipStream_t)stream);
}

static bool edt_dims_ok(int32_t nx, int32_t ny, int32_t nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && nx <= ISDF_EDT_MAX_SIDE && ny <= ISDF_EDT_MAX_SIDE && nz <= ISDF_EDT_MAX_SIDE;
}

int64_t isdf_edt_ws_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return edt_dims_ok(nx, ny, nz) ? 2 * edt_volume_bytes(nx, ny, nz) : ISDF_EINVAL;
}

int isdf_distance_transform(const uint8_t* feature, int32_t nx, int32_t ny, int32_t nz, int32_t invert, int32_t* dist2,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!feature || !dist2 || !edt_dims_ok(nx, ny, nz)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_edt_ws_bytes(nx, ny, nz)) return ISDF_EWORKSPACE;
  return launch_distance_transform(feature, nx, ny, nz, invert, dist2, (int32_t*)workspace, (hipStream_t)stream);
}

int isdf_occupancy_sdf(const uint8_t* occ, int32_t nx, int32_t ny, int32_t nz, double voxel, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!occ || !out || !edt_dims_ok(nx, ny, nz) || !(voxel > 0.0) || !__builtin_isfinite(voxel)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_edt_ws_bytes(nx, ny, nz)) return ISDF_EWORKSPACE;
  return launch_occupancy_sdf(occ, nx, ny, nz, voxel, out, workspace, (hipStream_t)stream);
}

// ---- ground truth from a triangle mesh (tri.hip)
static bool tri_size_ok(int64_t v) { return v >= 0 && v <= ((int64_t)1 << 30); }

int isdf_tri_pack(const float* vertices, int64_t nv, const int32_t* faces, int64_t m, const float* transform, float* packed,
                  int64_t packed_bytes, int32_t* counts, void* stream) {
  isdf_clear_stale_hip_error();
  if (!counts || !tri_size_ok(nv) || !tri_size_ok(m) || (nv > 0 && !vertices) || (m > 0 && (!faces || !packed))) return ISDF_EINVAL;
  if (transform)
    for (int k = 0; k < 12; ++k)
      if (!__builtin_isfinite(transform[k])) return ISDF_EINVAL;
  if (packed_bytes < ISDF_TRI_PACKED_BYTES(m)) return ISDF_EWORKSPACE;
  return launch_tri_pack(vertices, nv, faces, m, transform, packed, counts, (hipStream_t)stream);
}

int64_t isdf_tri_ws_bytes(int64_t n, int64_t m) {
  if (!tri_size_ok(n) || !tri_size_ok(m)) return ISDF_EINVAL;
  return 8 * n * (1 + tri_splits(n, m)) + 32 * ((n + 255) / 256) + 256;
}

int isdf_tri_distance(const float* pts, int64_t n, const float* packed, int64_t m, float* dist, int32_t* index, float* closest,
                      float* winding, double* record, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!record || !tri_size_ok(n) || !tri_size_ok(m) || (n > 0 && !pts) || (m > 0 && !packed)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_tri_ws_bytes(n, m)) return ISDF_EWORKSPACE;
  return launch_tri_distance(pts, n, packed, m, dist, index, closest, winding, record, workspace, (hipStream_t)stream);
}

// ---- the tile index and the culled distance (tri_tiles.hip)
int isdf_tri_tiles_build(const float* packed, int64_t m, const int32_t* order, int64_t n_order, double* tiles, int32_t* order_clean,
                         int32_t* counts, void* stream) {
  isdf_clear_stale_hip_error();
  if (!counts || !tri_size_ok(m) || n_order < 0 || n_order > ((int64_t)1 << 31) - ISDF_TRI_TILE || n_order % ISDF_TRI_TILE != 0)
    return ISDF_EINVAL;
  if ((n_order > 0 && (!order || !tiles || !order_clean)) || (m > 0 && !packed)) return ISDF_EINVAL;
  return launch_tri_tiles_build(packed, m, order, n_order, tiles, order_clean, counts, (hipStream_t)stream);
}

int64_t isdf_tri_tiles_ws_bytes(int64_t n) {
  if (!tri_size_ok(n)) return ISDF_EINVAL;
  return 16 * n + 32 * ((n + 255) / 256) + 256;
}

int isdf_tri_distance_tiles(const float* pts, int64_t n, const int32_t* qperm, const float* packed, int64_t m, const double* tiles,
                            const int32_t* order_clean, int64_t n_tiles, double beta, float* dist, int32_t* index, float* closest,
                            float* winding, double* record, int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!record || !tri_size_ok(n) || !tri_size_ok(m) || n_tiles < 0 || n_tiles > ((int64_t)1 << 23) || beta != beta) return ISDF_EINVAL;
  if ((n > 0 && (!pts || !qperm)) || (n_tiles > 0 && (!tiles || !order_clean)) || (m > 0 && !packed)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_tri_tiles_ws_bytes(n)) return ISDF_EWORKSPACE;
  return launch_tri_distance_tiles(pts, n, qperm, packed, m, tiles, order_clean, n_tiles, beta, dist, index, closest, winding, record,
                                   stats, workspace, (hipStream_t)stream);
}

// ---- routing through the map (route.hip)
static bool route_dims_ok(int32_t nx, int32_t ny, int32_t nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny <= ISDF_ROUTE_MAX_VOXELS && (int64_t)nx * ny * nz <= ISDF_ROUTE_MAX_VOXELS;
}

int isdf_route_init(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, const int32_t* goals, int32_t n_goals, int32_t* dist,
                    void* stream) {
  isdf_clear_stale_hip_error();
  if (!free || !dist || !route_dims_ok(nx, ny, nz) || n_goals < 0 || (n_goals > 0 && !goals)) return ISDF_EINVAL;
  return launch_route_init(free, nx, ny, nz, goals, n_goals, dist, (hipStream_t)stream);
}

int64_t isdf_route_ws_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return route_dims_ok(nx, ny, nz) ? route_volume_bytes(nx, ny, nz) : ISDF_EINVAL;
}

int isdf_route_relax(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, int32_t* dist, void* workspace,
                     int64_t workspace_bytes, int32_t rounds, int32_t* changed, void* stream) {
  isdf_clear_stale_hip_error();
  if (!free || !dist || !changed || !route_dims_ok(nx, ny, nz) || rounds < 1) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_route_ws_bytes(nx, ny, nz)) return ISDF_EWORKSPACE;
  return launch_route_relax(free, nx, ny, nz, dist, (int32_t*)workspace, rounds, changed, (hipStream_t)stream);
}

int isdf_route_trace(const int32_t* dist, int32_t nx, int32_t ny, int32_t nz, const int32_t* starts, int32_t B, int32_t max_len,
                     int32_t* path, int32_t* len, void* stream) {
  isdf_clear_stale_hip_error();
  if (!dist || !starts || !path || !len || !route_dims_ok(nx, ny, nz) || B < 0 || max_len < 1) return ISDF_EINVAL;
  return launch_route_trace(dist, nx, ny, nz, starts, B, max_len, path, len, (hipStream_t)stream);
}

// ---- where to look next: frontiers, clusters and view gain (explore.hip); the grids follow routing's rule
int isdf_frontier_init(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t* label, void* stream) {
  isdf_clear_stale_hip_error();
  if (!state || !label || !route_dims_ok(nx, ny, nz)) return ISDF_EINVAL;
  return launch_frontier_init(state, nx, ny, nz, label, (hipStream_t)stream);
}

int64_t isdf_frontier_ws_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return route_dims_ok(nx, ny, nz) ? frontier_ws_bytes(nx, ny, nz) : ISDF_EINVAL;
}

int isdf_frontier_relax(int32_t* label, int32_t nx, int32_t ny, int32_t nz, void* workspace, int64_t workspace_bytes, int32_t rounds,
                        int32_t* changed, void* stream) {
  isdf_clear_stale_hip_error();
  if (!label || !changed || !route_dims_ok(nx, ny, nz) || rounds < 1) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_frontier_ws_bytes(nx, ny, nz)) return ISDF_EWORKSPACE;
  return launch_frontier_relax(label, nx, ny, nz, (int32_t*)workspace, rounds, changed, (hipStream_t)stream);
}

int isdf_frontier_clusters(const int32_t* label, int32_t nx, int32_t ny, int32_t nz, void* workspace, int64_t workspace_bytes,
                           int32_t max_clusters, int32_t* counts, int64_t* records, void* stream) {
  isdf_clear_stale_hip_error();
  if (!label || !counts || !route_dims_ok(nx, ny, nz) || max_clusters < 0 || (max_clusters > 0 && !records)) return ISDF_EINVAL;
  if (!workspace || workspace_bytes < isdf_frontier_ws_bytes(nx, ny, nz)) return ISDF_EWORKSPACE;
  return launch_frontier_clusters(label, nx, ny, nz, workspace, max_clusters, counts, records, (hipStream_t)stream);
}

int64_t isdf_view_gain_ws_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t B) {
  if (!route_dims_ok(nx, ny, nz) || B < 0) return ISDF_EINVAL;
  return (4 * view_gain_words(nx, ny, nz) * B + 255) / 256 * 256;
}

int isdf_view_gain(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, const float* origin, const float* spacing,
                   const float* T_WC, int32_t B, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float t_min, float t_max,
                   int32_t* unknown, float* depth, int32_t* distinct, void* workspace, int64_t workspace_bytes, void* stream) {
  isdf_clear_stale_hip_error();
  if (!state || !origin || !spacing || !route_dims_ok(nx, ny, nz) || B < 0 || H < 1 || W < 1) return ISDF_EINVAL;
  if (B > 0 && (!T_WC || !unknown || !depth)) return ISDF_EINVAL;
  // one wave per 8 x 8 pixel tile, four to a block; the outputs are indexed in 64 bits
  if ((int64_t)H * W > 0x7fffffff || (int64_t)B * (((int64_t)H + 7) / 8) * (((int64_t)W + 7) / 8) > 0x7fffffff) return ISDF_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!(spacing[k] > 0.f) || !__builtin_isfinite(spacing[k]) || !__builtin_isfinite(origin[k])) return ISDF_EINVAL;
  if (fx == 0.f || fy == 0.f) return ISDF_EINVAL;
  for (float v : {fx, fy, cx, cy})
    if (!__builtin_isfinite(v)) return ISDF_EINVAL;
  if (!(t_min >= 0.f) || !(t_max > t_min)) return ISDF_EINVAL;      // also refuses NaN; t_max may be +inf
  if (distinct && B > 0 && (!workspace || workspace_bytes < isdf_view_gain_ws_bytes(nx, ny, nz, B))) return ISDF_EWORKSPACE;
  return launch_view_gain(state, nx, ny, nz, origin, spacing, T_WC, B, fx, fy, cx, cy, H, W, t_min, t_max, unknown, depth, distinct,
                          workspace, (hipStream_t)stream);
}

}  // extern "C"
