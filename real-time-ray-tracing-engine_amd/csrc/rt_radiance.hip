// rt_radiance.hip — path-traced light along caller rays on gfx950
// (rt_radiance_device; the per-ray code is rt_radiance.h).
//
// The third kernel of the query family (rt_query.hip, rt_occlusion.hip) and
// the only one whose hot path is the full integrator: segment<false, F, false,
// MS> with the (F, MS) that render_instance (rt_kernel.hip) picks for the
// scene, so a ray that the render's camera makes carries the render's bits.
// A separate translation unit: the megakernel, the guide kernel and both query
// kernels keep their instances, registers and frames.
//
// One lane per ray, one wavefront per 64 consecutive rays, blocks of
// block_waves(F) waves.  A lane owns its ray's samples and adds them, in
// ascending order, to three sums it holds in registers: no LDS accumulator, no
// atomics, and no item is ever pulled across rays as render_tiles pulls them
// across pixels -- that would tie a ray's bits to its neighbours.  The lane
// reads its 64-B ray, writes its three doubles once with plain stores; lanes
// past n neither trace nor write.  Nothing is staged: the walks read nodes and
// the Perlin table from memory (radiance_scene), the dynamic LDS is the
// traversal stacks [block_waves(F)][stack_depth][64] alone.  No persistent
// units, no work-unit plan, no cost order, none of the scene's scratch.
// Lane set-up and launch: rt_ray_launch.h; the instance table: rt_path.h feature_table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions are rt_kernel.o's to export: this
// file's copies of the per-path code are its own (as in rt_guides.hip)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_radiance.h"
#pragma clang attribute pop
#include "rt_ray_launch.h"

namespace {

using namespace rtr;

// The occupancy target of the render instance of the same feature set
// (rt_kernel.hip RT_WAVES_PER_EU, measured there): the integrator is the same
// code under the same register pressure.
#define RT_RADIANCE_WAVES_PER_EU(F) ((F) == F_FLAT ? 4 : (((F) & ~F_BVH4) == 0 ? 4 : 3))

template <unsigned F, MatSet MS>
__global__ __launch_bounds__(64 * block_waves(F)) __attribute__((amdgpu_waves_per_eu(RT_RADIANCE_WAVES_PER_EU(F)))) void
radiance_kernel(DScene S_, DCamera C, DRadiance P, const rt_ray *rays, double *rgb) {
  extern __shared__ int4 dyn_lds[];
  const rtl::RayLane L;
  const int64_t k = L.ray<block_waves(F)>();
  if (k >= P.n) return; // rays past n are neither traced nor written
  const DScene S = radiance_scene(S_);
  int *stk = rtl::lane_stack(L, dyn_lds, S.stack_depth);
  const rt_ray *q = rays + k;
  double *px = rgb + 3 * k;
  RadianceState st = radiance_begin(C, P, k, *q, px);
  // One flat loop over trips, not a loop over samples around a loop over
  // segments: a lane that ends a path starts its next sample in the next trip
  // while its wave mates go on with theirs.  The wave leaves when no lane has
  // a path under way or a sample left; by radiance_trip's termination argument
  // that is after at most samples * max_depth + samples trips.
  while (__ballot(radiance_more(st, P)) != 0) radiance_trip<F, MS>(S, C, P, q, st, stk);
  px[0] = st.sum[0];
  px[1] = st.sum[1];
  px[2] = st.sum[2];
}

using RadianceFn = void (*)(DScene, DCamera, DRadiance, const rt_ray *, double *);

// render_instance's choice (rt_kernel.hip): the table's instance, or the
// Lambertian-only twin of the plain flat world
RadianceFn radiance_instance(int features) {
  static constexpr auto table =
      feature_table([](auto f) { return radiance_kernel<canonical_features(decltype(f)::value), M_ANY>; });
  if (diffuse_twin(features)) return radiance_kernel<F_FLAT, M_DIFFUSE>;
  return table[features & F_ALL];
}

} // namespace

extern "C" hipError_t rtk_launch_radiance(const DScene *S, const DCamera *C, const rt_radiance_params *p, int64_t n,
                                          const rt_ray *rays, double *rgb, hipStream_t stream) {
  return rtl::launch_per_ray(radiance_instance(S->features), canonical_features((unsigned)(S->features & F_ALL)),
                             S->stack_depth, n, stream, *S, *C, radiance_launch(*p, n), rays, rgb);
}

// The render's camera rays on the host (rt_camera_rays): camera_ray of
// stratum k for every pixel of rows [row_begin, row_end), row-major, under
// Key{seed; j * W + i, k}.  This file's host pass, built with
// -ffp-contract=off like every build of rt_path.h: sqrt and fma are correctly
// rounded on both sides, so these are the doubles the kernels form.
extern "C" void rtk_camera_rays_host(const DCamera *C, uint64_t seed, int32_t stratum, int32_t row_begin,
                                     int32_t row_end, rt_ray *rays) {
  for (int j = row_begin; j < row_end; ++j)
    for (int i = 0; i < C->W; ++i) {
      const Key key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(j * C->W + i), (uint32_t)stratum};
      const Ray r = camera_ray(*C, key, i, j, stratum);
      rt_ray &o = rays[(size_t)(j - row_begin) * C->W + i];
      o.origin[0] = r.o.x, o.origin[1] = r.o.y, o.origin[2] = r.o.z;
      o.direction[0] = r.d.x, o.direction[1] = r.d.y, o.direction[2] = r.d.z;
      o.time = r.tm;
      o.t_max = kInf;
    }
}
