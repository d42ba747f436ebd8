// rt_occlusion.hip — any-hit visibility of caller rays on gfx950
// (rt_occluded_device; the per-ray code is rt_occlusion.h).
//
// A separate kernel beside the megakernel, the guide kernel and the query
// kernel: their instances, registers, frames and records stay what they were.
// One lane per ray, one wavefront per 64 consecutive rays, no atomics: the
// lane reads its 64-B ray, decides whether it is traced at all, walks until
// the first primitive it accepts, and writes its verdict byte once with a
// plain byte store -- a wave's 64 bytes are consecutive; lanes past n neither
// trace nor write.  None of the scene's scratch.
//
// The same six instances as the query kernel (rt_query.h query_features:
// F_XFORM, F_FLAT, F_BVH4).  Nothing is staged: the walks read nodes from
// memory (query_scene), the dynamic LDS is the traversal stacks
// [block_waves(F)][stack_depth][64] alone.
// Lane set-up and launch: rt_ray_launch.h; the instance table: rt_path.h feature_table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions are rt_kernel.o's to export: this
// file's copies of the per-path code are its own (as in rt_query.hip)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_occlusion.h"
#pragma clang attribute pop
#include "rt_ray_launch.h"

namespace {

using namespace rto;

template <unsigned F>
__global__ __launch_bounds__(64 * block_waves(F)) void occlusion_kernel(DScene S_, int64_t n, const rt_ray *rays,
                                                                        uint8_t *occluded) {
  extern __shared__ int4 dyn_lds[];
  const rtl::RayLane L;
  const int64_t k = L.ray<block_waves(F)>();
  if (k >= n) return; // rays past n are neither traced nor written
  const DScene S = query_scene(S_);
  int *stk = rtl::lane_stack(L, dyn_lds, S.stack_depth);
  const rt_ray q = rays[k];
  occluded[k] = occluded_ray<F>(S, q, stk);
}

} // namespace

extern "C" hipError_t rtk_launch_occluded(const DScene *S, int64_t n, const rt_ray *rays, uint8_t *occluded,
                                          hipStream_t stream) {
  static constexpr auto table =
      feature_table([](auto f) { return occlusion_kernel<query_features(decltype(f)::value)>; });
  const unsigned f = (unsigned)(S->features & F_ALL);
  return rtl::launch_per_ray(table[f], query_features(f), S->stack_depth, n, stream, *S, n, rays, occluded);
}
