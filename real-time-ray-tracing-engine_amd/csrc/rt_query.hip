// rt_query.hip — closest hits of caller rays on gfx950 (rt_trace_device; the
// per-ray code is rt_query.h).
//
// A separate kernel beside the megakernel and the guide kernel: their
// instances, registers and frames stay what they were.  One lane per ray, one
// wavefront per 64 consecutive rays, no atomics: the lane reads its 64-B ray,
// decides whether it is traced at all, walks, and writes its 72-B record once
// with plain stores; lanes past n neither trace nor write.  No persistent
// units, no work-unit plan, none of the scene's scratch.
//
// Specialised by what the search and the record read of the scene's feature
// bits (rt_query.h query_features: F_XFORM, F_FLAT, F_BVH4 -- six instances).
// Nothing is staged: the walks read nodes from memory (query_scene), the
// dynamic LDS is the traversal stacks [block_waves(F)][stack_depth][64] alone.
// Lane set-up and launch: rt_ray_launch.h; the instance table: rt_path.h feature_table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions are rt_kernel.o's to export: this
// file's copies of the per-path code are its own (as in rt_guides.hip)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_query.h"
#pragma clang attribute pop
#include "rt_ray_launch.h"

namespace {

using namespace rtq;

template <unsigned F>
__global__ __launch_bounds__(64 * block_waves(F)) void query_kernel(DScene S_, const int32_t *xf_obj, int64_t n,
                                                                    const rt_ray *rays, rt_ray_hit *hits) {
  extern __shared__ int4 dyn_lds[];
  const rtl::RayLane L;
  const int64_t k = L.ray<block_waves(F)>();
  if (k >= n) return; // rays past n are neither traced nor written
  const DScene S = query_scene(S_);
  int *stk = rtl::lane_stack(L, dyn_lds, S.stack_depth);
  const rt_ray q = rays[k];
  hits[k] = query_ray<F>(S, xf_obj, q, stk);
}

} // namespace

extern "C" hipError_t rtk_launch_trace(const DScene *S, const int32_t *xf_obj, int64_t n, const rt_ray *rays,
                                       rt_ray_hit *hits, hipStream_t stream) {
  static constexpr auto table = feature_table([](auto f) { return query_kernel<query_features(decltype(f)::value)>; });
  const unsigned f = (unsigned)(S->features & F_ALL);
  return rtl::launch_per_ray(table[f], query_features(f), S->stack_depth, n, stream, *S, xf_obj, n, rays, hits);
}
