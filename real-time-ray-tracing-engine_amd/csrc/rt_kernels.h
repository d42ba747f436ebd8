// rt_kernels.h — every rtk_* launcher, declared once: included by the files
// that define them (rt_kernel.hip, rt_frame.hip, rt_adaptive.hip, rt_guides.hip,
// rt_denoise.hip, rt_temporal.hip, rt_bvh_build.hip, rt_bvh_sah.hip, rt_collapse.hip, rt_refit.hip, rt_query.hip, rt_occlusion.hip, rt_radiance.hip, rt_motion.hip) and by their caller (rt_api.cpp), so a
// definition whose parameter list drifts from its callers' no longer compiles.
#ifndef RT_KERNELS_H
#define RT_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_layout.h"
#include "rt_lds_plan.h"
#include "rt_live.h"

extern "C" {

// ---- rt_kernel.hip: the render instances.  P carries its plan (rt_plan.h apply_plan)
hipError_t rtk_launch_render(const DScene *S, const DCamera *C, const DLaunch *P, double *out,
                             unsigned long long *stats, hipStream_t stream);
// the residency plan's inputs (rt_lds_plan.h): the one-unit instance of a
// feature set (pc_waves 0) or its persistent instance in blocks of pc_waves waves
hipError_t rtk_instance_attrs(int features, int pc_waves, KernelAttrs *attrs);
int rtk_cost_f(int features);
// RT_UNIT_TIMES builds only (tools/unit_timeline.py)
hipError_t rtk_unit_times(unsigned long long *host, int n_units);
hipError_t rtk_unit_times_clear(void);

// ---- rt_frame.hip: frame assembly, tile exchange, dispatch order, bytes
// after rtk_launch_render of a frame launch with chunked tiles: P->parts -> out
hipError_t rtk_launch_split_sum(const DCamera *C, const DLaunch *P, double *out, hipStream_t stream);
// after rtk_launch_render of a tile-layout launch: P->parts -> out[P->tile_order[tile]]
hipError_t rtk_launch_shard_finish(const DLaunch *P, double *out, hipStream_t stream);
hipError_t rtk_launch_tiles_sum(const double *parts, int64_t n_tiles, int chunks, double *out,
                                hipStream_t stream);
hipError_t rtk_launch_tile_order(const uint32_t *cost, int n, int n_head, int32_t *order, hipStream_t stream);
hipError_t rtk_launch_tiles_to_frame(const double *tiles, int n_shards, int64_t shard_stride, int W,
                                     int row_begin, int row_end, double scale, int scaled, int accumulate,
                                     double *out, hipStream_t stream);
hipError_t rtk_launch_to_bytes(const double *rgb, int64_t n, double scale, uint8_t *bytes, hipStream_t stream);

// ---- rt_adaptive.hip: adaptive sampling
hipError_t rtk_launch_tile_list_copy(const int32_t *in, int n, int tiles, int32_t *out, hipStream_t stream);
hipError_t rtk_launch_adaptive_update(const double *delta, int batch_strata, const int32_t *list, int n_tiles,
                                      int W, int H, double *acc, double *s1, double *s2, int32_t *tile_strata,
                                      hipStream_t stream);
hipError_t rtk_launch_adaptive_select(const double *s1, const double *s2, const int32_t *tile_strata,
                                      int batch_strata, int W, int H, double threshold, double floor_,
                                      int min_batches, const int32_t *list, int n_in, int32_t *out,
                                      int32_t *count_out, double *tile_error, hipStream_t stream);
hipError_t rtk_launch_to_bytes_tiles(const double *rgb, const int32_t *tile_strata, int W, int H, uint8_t *bytes,
                                     hipStream_t stream);
// guided sampling: history = a variance history (its col plane is read), variance = [H][W] doubles;
// tile_strata may be null (then strata_now counts); tile_error / tile_count may be null
hipError_t rtk_launch_guided_select(const void *history, const double *variance, const int32_t *tile_strata,
                                    int strata_now, int W, int H, double threshold, double floor_,
                                    double min_count, const int32_t *list, int n_in, int32_t *out,
                                    int32_t *count_out, double *tile_error, double *tile_count,
                                    hipStream_t stream);

// ---- rt_guides.hip: first-hit guide sums [rows][W][8] (P: launch_geometry's fields; no plan)
hipError_t rtk_launch_guides(const DScene *S, const DCamera *C, const DLaunch *P, double *out,
                             hipStream_t stream);

// ---- rt_query.hip: hits[k] = the closest hit of rays[k], k in [0, n) (rt_query.h; xf_obj: the
// object of each xforms[] record; n <= 0 queues nothing)
hipError_t rtk_launch_trace(const DScene *S, const int32_t *xf_obj, int64_t n, const rt_ray *rays,
                            rt_ray_hit *hits, hipStream_t stream);

// ---- rt_motion.hip: motion[j * W + i] = the motion of the surface under pixel (i, j) of the frame
// since `pose_prev` was taken (rt_motion.h; c: the pose's layout, rt_live.h; an empty frame queues nothing)
hipError_t rtk_launch_motion(const DScene *S, const int32_t *xf_obj, const rt_frame *frame,
                             const rt_live::PoseCounts *c, const double *pose_prev, rt_motion *motion,
                             hipStream_t stream);

// ---- rt_occlusion.hip: occluded[k] = 1 where something stands in (0.001, t_max] of rays[k], else 0,
// k in [0, n): one byte each (rt_occlusion.h; n <= 0 queues nothing)
hipError_t rtk_launch_occluded(const DScene *S, int64_t n, const rt_ray *rays, uint8_t *occluded,
                               hipStream_t stream);

// ---- rt_radiance.hip: rgb[k] (3 doubles) = (accumulate: itself) + the p->samples path-traced samples of
// rays[k], k in [0, n) (rt_radiance.h; C: bg and max_depth are read; p checked by the caller; n <= 0
// queues nothing)
hipError_t rtk_launch_radiance(const DScene *S, const DCamera *C, const rt_radiance_params *p, int64_t n,
                               const rt_ray *rays, double *rgb, hipStream_t stream);
// host only: rays[(j - row_begin) * W + i] = the render's camera ray of stratum `stratum` of pixel (i, j)
void rtk_camera_rays_host(const DCamera *C, uint64_t seed, int32_t stratum, int32_t row_begin, int32_t row_end,
                          rt_ray *rays);

// ---- rt_denoise.hip: the a-trous filters, one launcher.  Sigmas resolved: > 0 on, <= 0 off; passes < 0: none
size_t rtk_denoise_workspace_bytes(int W, int H);          // the plain layout
size_t rtk_denoise_variance_workspace_bytes(int W, int H); // the variance layout (both variance kinds)
enum {
  RTK_FILTER_PLAIN = 0,    // rt_denoise_device
  RTK_FILTER_VARIANCE = 1, // rt_denoise_variance_device: v from the moments and the spatial estimate
  RTK_FILTER_GIVEN = 2     // rt_denoise_given_variance_device: v is the caller's plane, no estimation stage
};
struct FilterLaunch {
  int kind;
  int W, H;
  const double *rgb;
  double scale;
  const int32_t *tile_strata;
  const double *guides;
  int guide_strata;
  const double *s1, *s2; // VARIANCE: the batch moments, null = none
  int batch_strata;
  int min_batches;        // VARIANCE: resolved (>= 2)
  const double *variance; // GIVEN: [H][W]
  int passes;
  double sigma_n, sigma_z, sigma_h;
  double sigma_c; // PLAIN: the colour sigma; the variance kinds: sigma_l
  void *workspace;
  double *out;
  double *var_out; // the variance kinds; may be null
};
hipError_t rtk_launch_filter(const FilterLaunch *args, hipStream_t stream);

// ---- rt_temporal.hip: the temporal reprojection (params checked, may be null; prev /
// history_prev both null: no history); the _variance pair takes histories with a var plane
size_t rtk_history_variance_bytes(int W, int H);
hipError_t rtk_launch_temporal_variance(const rt_frame *now, const double *rgb, double scale,
                                        const int32_t *tile_strata, int strata_now, const double *guides,
                                        int guide_strata, const rt_frame *prev, const void *history_prev,
                                        const double *variance_now, const rt_temporal_params *params,
                                        void *history_out, double *out, double *variance_out, hipStream_t stream);
// the _motion pair: `motion` is rt_motion_device's plane (not null)
hipError_t rtk_launch_temporal_variance_motion(const rt_frame *now, const double *rgb, double scale,
                                               const int32_t *tile_strata, int strata_now, const double *guides,
                                               int guide_strata, const rt_frame *prev, const void *history_prev,
                                               const rt_motion *motion, const double *variance_now,
                                               const rt_temporal_params *params, void *history_out, double *out,
                                               double *variance_out, hipStream_t stream);
hipError_t rtk_launch_temporal_motion(const rt_frame *now, const double *rgb, double scale,
                                      const int32_t *tile_strata, int strata_now, const double *guides,
                                      int guide_strata, const rt_frame *prev, const void *history_prev,
                                      const rt_motion *motion, const rt_temporal_params *params, void *history_out,
                                      double *out, hipStream_t stream);
size_t rtk_history_bytes(int W, int H);
hipError_t rtk_launch_temporal(const rt_frame *now, const double *rgb, double scale, const int32_t *tile_strata,
                               int strata_now, const double *guides, int guide_strata, const rt_frame *prev,
                               const void *history_prev, const rt_temporal_params *params, void *history_out,
                               double *out, hipStream_t stream);

// ---- rt_bvh_build.hip, rt_bvh_sah.hip: the device BVH builders
size_t rtk_lbvh_temp_bytes(int n);
hipError_t rtk_build_lbvh(const double *boxes, const DItem *items_in, int n, const double *scene_lo,
                          const double *scene_hi, DNode *nodes, DItem *items_out, int *depth_dev, void *temp,
                          size_t temp_bytes, hipStream_t st);
size_t rtk_sah_temp_bytes(int n);
hipError_t rtk_build_sah(const double *boxes, const DItem *items_in, int n, DNode *nodes, DItem *items_out,
                         void *temp, size_t temp_bytes, int stack_budget, int *n_nodes, int *depth,
                         int *root_leaf, hipStream_t st);

// ---- rt_collapse.hip: the binary tree `bin` (n_nodes records, root 0, any order) collapsed to
// 4-wide nodes in BFS order, the bytes of rt_scene.cpp's collapse_bvh4 (rt_collapse.h is the source
// of both).  out: room for n_nodes records, the first *n_nodes4 written; *levels: the 4-wide levels.
// n_nodes < 1, a short temp and buffers that overlap are refused before anything is queued.
// Synchronises `st` once per level; the tree is complete on return.
size_t rtk_collapse4_temp_bytes(int n_nodes);
hipError_t rtk_collapse4(const DNode *bin, int n_nodes, DNode4 *out, void *temp, size_t temp_bytes, int *n_nodes4,
                         int *levels, hipStream_t st);

// ---- rt_refit.hip: moved spheres and the bottom-up refit of the world tree's boxes.
// nodes: DNode (arity 2) or DNode4 (arity 4) records.  temp (rtk_refit_temp_bytes) holds the
// links rtk_refit_links builds once per tree and the arrival counters each rtk_refit_boxes clears;
// boxes: n_items x (lo xyz, hi xyz) fp64 in leaf order.  rtk_refit = links + one refit (tests).
size_t rtk_refit_temp_bytes(int n_items, int n_nodes);
hipError_t rtk_refit_links(const void *nodes, int arity, int n_nodes, void *temp, size_t temp_bytes, hipStream_t st);
hipError_t rtk_refit_boxes(void *nodes, int arity, int n_nodes, int n_items, const double *boxes, void *temp,
                           size_t temp_bytes, hipStream_t st);
hipError_t rtk_refit(void *nodes, int arity, int n_nodes, int root_leaf, const DItem *items, int n_items,
                     const double *boxes, void *temp, size_t temp_bytes, hipStream_t st);
// each world item's fp64 box from the tables (rt_refit.h item_box)
hipError_t rtk_item_boxes(const DItem *items, int n_items, const DSphere *spheres, const DQuad *quads,
                          const DXform *xforms, double *boxes, hipStream_t st);
// One move: entry j sets spheres[sphere_of[ids[j]]].c0 = centres[j] (and the matching roots[] copy
// of a flat world, root_items its items) when ids[j] is in [0, n_objects), sphere_of[] of it is
// >= 0, no other applicable entry names it and the centre is finite; any other entry is skipped.
// named: n_objects counters (scratch).
struct RefitMove {
  const int32_t *ids;
  const double *centres;
  int32_t n, n_objects;
  const int32_t *sphere_of;
  unsigned *named;
  DSphere *spheres;
  DRoot *roots;
  const DItem *root_items;
  int32_t n_roots, pad_;
};
hipError_t rtk_move_spheres(const RefitMove *m, hipStream_t st);
// Live transforms and quads (rt_live.h: the entry rules and what an entry writes).  Entry j of
// ids / values (n x 3 fp64) is applied when rt_live::transform_entry / quad_entry accepts it and
// no other accepted entry names its object; any other entry is skipped.  index: device pointers;
// named: n_objects counters (scratch).
struct LiveEdit {
  const int32_t *ids;
  const double *values;
  int32_t n, pad_;
  rt_live::LiveIndex index;
  unsigned *named;
  DXform *xforms;
  DQuad *quads;
};
hipError_t rtk_set_transforms(const LiveEdit *e, hipStream_t st);
hipError_t rtk_move_quads(const LiveEdit *e, hipStream_t st);
// the pose of these tables (rt_live.h: pose_bytes(c) bytes at `pose`), one thread per record
hipError_t rtk_pose(const rt_live::PoseCounts *c, const DXform *xforms, const DSphere *spheres, const DQuad *quads,
                    double *pose, hipStream_t st);
// each world medium's box from the tables (rt_refit.h medium_box) into mbox (6 floats per medium)
hipError_t rtk_medium_boxes(const DItem *mitems, int n_mitems, const DMedium *media, const DItem *bitems,
                            const DSphere *spheres, const DQuad *quads, const DXform *xforms, float *mbox,
                            hipStream_t st);

} // extern "C"
#endif
