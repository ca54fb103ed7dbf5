// Every host launcher and layout helper that crosses a translation unit, declared ONCE: the defining .hip file and capi.hip both
// include this, so a definition that drifts from its declaration fails to compile instead of (at best) failing to link.
#pragma once
#include "isdf_common.h"

namespace isdf {

struct ChainParams; struct DwParams; struct TailParams; struct AdamwHyper;   // chain_params.h

int launch_chain(const ChainParams& p, int mode, int64_t nTiles, hipStream_t st);                                   // chain.hip
bool fwd_pair_supported(const NetLayout& l);                                                                        // fwd_pair.hip
int launch_fwd_pair(const ChainParams& p, int64_t nTiles, hipStream_t st);
int launch_dw(const DwParams& p, hipStream_t st);                                                                   // dw.hip
int launch_sample_rays(const isdf_sample_args& a, const isdf_sample_out& o, void* scan_ws, hipStream_t st);         // sampler.hip
int64_t sample_scan_bytes(int64_t max_rays);
// optim.hip.  The step tail: `block` as capi.hip filled it; the launcher derives AdamwCoef and the grid.  phase 0 needs `hyper`,
// phase 1 takes none; part 0 = one launch, 1 / 2 = the split tail (phase 1 only)
int launch_step_tail(int phase, const TailParams& block, const AdamwHyper* hyper, int part, hipStream_t st);
int launch_adamw_pack(const TailParams& block, const AdamwHyper& hyper, hipStream_t st);
int launch_adamw(float* p, float* m, float* v, const float* g, const float* cnt, float gs, const AdamwHyper& hyper, int64_t n,
                 hipStream_t st);
int launch_pack(const NetLayout& L, const float* params, uint16_t* shadow, hipStream_t st);
int launch_frame_avg(const float* bl, const float* bc, int F, float* la, float* fa, const int32_t* fa_index, hipStream_t st);
int launch_bounds_pc(const int32_t* n_valid, int max_rays, int S, const float* pc, const float* z, const float* depth,
                     const float* surf, int64_t n_surf, float* bounds, float* gv, hipStream_t st);
int launch_normals(const float* depth, int H, int W, float fx, float fy, float cx, float cy, float* normals, hipStream_t st);   // ingest.hip
int launch_render_depth(const int32_t* n_valid, int64_t n_host, int64_t max_rays, int S, const float* z, const float* sdf,
                        const float* depth_sample, float th, float* view, int32_t* below, hipStream_t st);
int64_t mesh_ws_layout(int64_t P, int64_t* nBlocks, int64_t* offOff, int64_t* offTot, int64_t* offVbase);          // mesh.hip
int launch_marching_cubes(const float* vol, int32_t D0, int32_t D1, int32_t D2, float level, const float* A, const float* N,
                          int64_t* counts, float* verts, float* normals, int64_t max_verts, int32_t* faces, int64_t max_faces,
                          void* workspace, hipStream_t st);
void mc_tables_host(int32_t* edge_corners, int8_t* tri_table);
int launch_render_samples(const isdf_render_args& a, float* z, float* pc, hipStream_t st);                          // render.hip
int launch_normal_points(const float* T_WC, const float* dirs_C, int64_t R, int64_t n_rays, const float* depth, float* pts,
                         hipStream_t st);
int launch_normal_finish(const float* T_WC, int64_t R, int64_t n_rays, const float* grad, float* normals, hipStream_t st);
int launch_sdf_metrics(const isdf_gt_volume& vol, const float* pts, const float* sdf, int64_t n, int exclude_zero,  // eval.hip
                       float oob_fill, double* record, float* gt_out, uint8_t* valid_out, double* part, hipStream_t st);
int launch_region_metrics(const isdf_region_args& a, double* records, double* part, hipStream_t st);
int launch_nn_distance(const float* query, int64_t n, const float* target, int64_t m, float* dist, int32_t* index,
                       double* dist_sum, unsigned long long* keys, double* part, hipStream_t st);
int launch_slice_images(const isdf_colormap* cmap, const isdf_gt_volume* vol, const float* pts, const float* sdf, int64_t n,   // slices.hip
                        float oob_fill, float chomp_eps, uint8_t* pred_rgb, float* gt_out, uint8_t* gt_rgb, float* pred_cost,
                        float* gt_cost, hipStream_t st);
int launch_plane_points(const float* origin, const float* du, const float* dv, int32_t H, int32_t W, float* pts_out,
                        hipStream_t st);
int launch_reduce_partials(const double* part, int64_t nPart, int width, uint64_t max_mask, double* out, hipStream_t st);   // reduce.hip
int launch_visible_points(const float* pts, int64_t n, const float* T_CW, const float* depth, int32_t F, int32_t H, int32_t W,   // visible.hip
                          float fx, float fy, float cx, float cy, float trunc, int32_t* count, uint8_t* mask, int64_t* n_seen,
                          hipStream_t st);
int64_t band_ws_bytes(int32_t D0, int32_t D1, int32_t D2, int32_t coarse);                                          // band.hip
int launch_band_fill(float* vol, int64_t P, hipStream_t st);
int launch_band_select(const isdf_band_args& a, int32_t stride, const float* vol, int64_t* counts, void* workspace, hipStream_t st);
int launch_band_emit(const isdf_band_args& a, int32_t stride, const float* vol, int32_t* index_out, float* pts_out, int64_t n,
                     void* workspace, hipStream_t st);
int launch_band_update(const isdf_band_args& a, int32_t stride, float* vol, const int32_t* index, const float* values, int64_t n,
                       int64_t* counts, void* workspace, hipStream_t st);
int launch_band_leaks(const isdf_band_args& a, const float* vol, int64_t* counts, void* workspace, hipStream_t st);
int launch_grid_points(int32_t D0, int32_t D1, int32_t D2, const float* A, float* pts_out, hipStream_t st);
int launch_pose_points(const isdf_pose_args& a, float* pts, hipStream_t st);                                        // pose.hip
int launch_pose_system(const isdf_pose_args& a, const float* pts, const float* sdf, const float* grad, float huber, float trunc,
                       double* records, double* part, hipStream_t st);
int launch_traj_points(const isdf_traj_args& a, float* q_out, hipStream_t st);                                       // traj.hip
int launch_traj_step(const isdf_traj_args& a, const float* sdf, const float* grad, double* records, float* q_out, double* grad_out,
                     hipStream_t st);
int launch_arm_points(const isdf_arm_args& a, float* q_out, hipStream_t st);                                         // arm.hip
int launch_arm_step(const isdf_arm_args& a, const float* q, const float* sdf, const float* grad, double* records, float* q_out,
                    double* grad_out, hipStream_t st);
int launch_tsdf_integrate(const isdf_tsdf_args& a, hipStream_t st);                                                 // fusion.hip
int64_t edt_volume_bytes(int32_t nx, int32_t ny, int32_t nz);
int launch_distance_transform(const uint8_t* feature, int32_t nx, int32_t ny, int32_t nz, int invert, int32_t* dist2, int32_t* scratch,
                              hipStream_t st);
int launch_occupancy_sdf(const uint8_t* occ, int32_t nx, int32_t ny, int32_t nz, double voxel, float* out, void* ws, hipStream_t st);
int64_t tri_splits(int64_t n, int64_t m);                                                                           // tri.hip
int launch_tri_pack(const float* verts, int64_t nv, const int32_t* faces, int64_t m, const float* T, float* packed, int32_t* counts,
                    hipStream_t st);
int launch_tri_distance(const float* pts, int64_t n, const float* packed, int64_t m, float* dist, int32_t* index, float* closest,
                        float* winding, double* record, void* workspace, hipStream_t st);
int launch_tri_finish(const float* pts, int64_t n, const float* packed, const unsigned long long* keys, const double* wpart,
                      int64_t splits, float* dist, int32_t* index, float* closest, float* winding, double* record, double* part,
                      hipStream_t st);
int launch_tri_tiles_build(const float* packed, int64_t m, const int32_t* order, int64_t n_order, double* tiles, int32_t* order_clean,   // tri_tiles.hip
                           int32_t* counts, hipStream_t st);
int launch_tri_distance_tiles(const float* pts, int64_t n, const int32_t* qperm, const float* packed, int64_t m, const double* tiles,
                              const int32_t* order_clean, int64_t n_tiles, double beta, float* dist, int32_t* index, float* closest,
                              float* winding, double* record, int64_t* stats, void* workspace, hipStream_t st);
int launch_route_init(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, const int32_t* goals, int32_t n_goals, int32_t* dist,   // route.hip
                      hipStream_t st);
int64_t route_volume_bytes(int32_t nx, int32_t ny, int32_t nz);
int launch_route_relax(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, int32_t* dist, int32_t* ws, int32_t rounds,
                       int32_t* changed, hipStream_t st);
int launch_route_trace(const int32_t* dist, int32_t nx, int32_t ny, int32_t nz, const int32_t* starts, int32_t B, int32_t max_len,
                       int32_t* path, int32_t* len, hipStream_t st);
int launch_frontier_init(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t* label, hipStream_t st);   // explore.hip
int64_t frontier_ws_bytes(int32_t nx, int32_t ny, int32_t nz);
int launch_frontier_relax(int32_t* label, int32_t nx, int32_t ny, int32_t nz, int32_t* ws, int32_t rounds, int32_t* changed,
                          hipStream_t st);
int launch_frontier_clusters(const int32_t* label, int32_t nx, int32_t ny, int32_t nz, void* ws, int32_t max_clusters, int32_t* counts,
                             int64_t* records, hipStream_t st);
int64_t view_gain_words(int32_t nx, int32_t ny, int32_t nz);
int launch_view_gain(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, const float* origin, const float* spacing,
                     const float* T_WC, int32_t B, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float t_min,
                     float t_max, int32_t* unknown, float* depth, int32_t* distinct, void* ws, hipStream_t st);

}  // namespace isdf
