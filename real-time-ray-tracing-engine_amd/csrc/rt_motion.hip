// rt_motion.hip — object motion vectors on gfx950 (rt_motion_device; the
// per-pixel code is rt_motion.h).
//
// A query kernel (§7p's recipe): one lane per pixel, one wavefront per 64
// consecutive pixels in row-major order, no atomics.  The lane forms its
// pixel-centre ray from the frame (no 64-B ray is read), walks, places the
// local hit with the current tables and with the pose, and writes its 64-B
// record once with plain stores; lanes past W * H neither trace nor write.
// The six instances of rt_query.hip (query_features); nodes are read from
// memory, the dynamic LDS is the traversal stacks alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions are rt_kernel.o's to export: this
// file's copies of the per-path code are its own (as in rt_query.hip)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_motion.h"
#pragma clang attribute pop
#include "rt_ray_launch.h"

namespace {

using namespace rtm;

template <unsigned F>
__global__ __launch_bounds__(64 * block_waves(F)) void motion_kernel(DScene S_, const int32_t *xf_obj, rt_frame frame,
                                                                     rt_live::PoseCounts c, const double *pose,
                                                                     int64_t n, rt_motion *motion) {
  extern __shared__ int4 dyn_lds[];
  const rtl::RayLane L;
  const int64_t k = L.ray<block_waves(F)>();
  if (k >= n) return; // pixels past W * H are neither traced nor written
  const DScene S = query_scene(S_);
  int *stk = rtl::lane_stack(L, dyn_lds, S.stack_depth);
  const int W = frame.image_width;
  const int j = (int)(k / W), i = (int)(k - (int64_t)j * W);
  motion[k] = motion_pixel<F>(S, xf_obj, frame, c, pose, i, j, stk);
}

} // namespace

extern "C" hipError_t rtk_launch_motion(const DScene *S, const int32_t *xf_obj, const rt_frame *frame,
                                        const rt_live::PoseCounts *c, const double *pose_prev, rt_motion *motion,
                                        hipStream_t stream) {
  static constexpr auto table = feature_table([](auto f) { return motion_kernel<query_features(decltype(f)::value)>; });
  const unsigned f = (unsigned)(S->features & F_ALL);
  const int64_t n = (int64_t)frame->image_width * frame->image_height;
  return rtl::launch_per_ray(table[f], query_features(f), S->stack_depth, n, stream, *S, xf_obj, *frame, *c, pose_prev,
                             n, motion);
}
