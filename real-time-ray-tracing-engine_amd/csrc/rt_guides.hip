// rt_guides.hip — first-hit guide sums on gfx950 (rt_render_guides_device;
// the per-sample code is rt_guides.h).
//
// A separate, primary-ray-only kernel: the megakernel (rt_kernel.hip) emits
// nothing for the denoiser, so its instances, registers and frames stay what
// they were.  One wavefront per 8x8 tile, one lane per pixel, no atomics: the
// lane starts from the buffer's value (accumulate) or 0, adds its strata in
// ascending order and writes its eight doubles once; lanes outside the image
// neither trace nor write.  One work unit per wavefront only -- no persistent
// units, no work-unit plan, no tile order.
//
// Specialised by the scene's feature bits as the render is (F_LIGHTS masked:
// a guide sample never shades).  Nothing is staged: the walks read nodes and
// the Perlin table from memory (rt_guides.h guide_scene), the dynamic LDS is
// the traversal stacks [block_waves(F)][stack_depth][64] alone.
// Lane set-up and launch: rt_ray_launch.h; the instance table: rt_path.h feature_table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions (sin_wide, items_closest_t) are
// rt_kernel.o's to export: this file's copies of the per-path code are its
// own (every header rt_path.h includes is already in, so only rt_path.h's and
// rt_guides.h's functions are covered)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_guides.h"
#pragma clang attribute pop
#include "rt_ray_launch.h"

namespace {

using namespace rtg;

template <unsigned F>
__global__ __launch_bounds__(64 * block_waves(F)) void guides_kernel(DScene S_, DCamera C, DLaunch P, double *out) {
  extern __shared__ int4 dyn_lds[];
  const rtl::RayLane L;
  const int lane = L.lane, tile = L.wave<block_waves(F)>();
  if (tile >= P.tiles_x * P.tiles_y) return; // wave-uniform; no block-wide barrier below
  const DScene S = guide_scene(S_);
  int *stk = rtl::lane_stack(L, dyn_lds, S.stack_depth);
  const int i = (tile % P.tiles_x) * 8 + (lane & 7);
  const int j = P.row_begin + (tile / P.tiles_x) * 8 + (lane >> 3);
  if (i >= C.W || j >= P.row_end) return; // pixels outside the image are not written
  double *px = out + (size_t)kGuideChannels * ((size_t)(j - P.row_begin) * C.W + i);
  guide_pixel<F>(S, C, P.seed_lo, P.seed_hi, i, j, P.sample_begin, P.sample_count, P.accumulate, stk, px);
}

// one instance per feature set without F_LIGHTS
constexpr unsigned guide_instance(unsigned f) { return guide_features(canonical_features(f)); }

} // namespace

extern "C" hipError_t rtk_launch_guides(const DScene *S, const DCamera *C, const DLaunch *P, double *out,
                                        hipStream_t stream) {
  static constexpr auto table = feature_table([](auto f) { return guides_kernel<guide_instance(decltype(f)::value)>; });
  const unsigned f = (unsigned)(S->features & F_ALL);
  if (P->sample_count < 0) return hipSuccess;
  // a wave's tile is its 64 rays
  return rtl::launch_per_ray(table[f], guide_instance(f), S->stack_depth, (int64_t)P->tiles_x * P->tiles_y * 64, stream,
                             *S, *C, *P, out);
}
