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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include <array>
#include <utility>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions (sin_wide, items_closest_t) are
// rt_kernel.o's to export: this file's copies of the per-path code are its
// own (every header rt_path.h includes is already in, so only rt_path.h's and
// rt_guides.h's functions are covered)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_guides.h"
#pragma clang attribute pop

namespace {

using namespace rtg;

template <unsigned F>
__global__ __launch_bounds__(64 * block_waves(F)) void guides_kernel(DScene S_, DCamera C, DLaunch P, double *out) {
  constexpr int BW = block_waves(F);
  extern __shared__ int4 dyn_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tile = blockIdx.x * BW + wv;
  if (tile >= P.tiles_x * P.tiles_y) return; // wave-uniform; no block-wide barrier below
  const DScene S = guide_scene(S_);
  int *stk = reinterpret_cast<int *>(dyn_lds) + wv * S.stack_depth * 64 + lane;
  const int i = (tile % P.tiles_x) * 8 + (lane & 7);
  const int j = P.row_begin + (tile / P.tiles_x) * 8 + (lane >> 3);
  if (i >= C.W || j >= P.row_end) return; // pixels outside the image are not written
  double *px = out + (size_t)kGuideChannels * ((size_t)(j - P.row_begin) * C.W + i);
  guide_pixel<F>(S, C, P.seed_lo, P.seed_hi, i, j, P.sample_begin, P.sample_count, P.accumulate, stk, px);
}

using GuideFn = void (*)(DScene, DCamera, DLaunch, double *);

// one instance per feature set without F_LIGHTS; F_BVH4 never comes with
// F_FLAT (rt_kernel.hip canonical)
constexpr unsigned canonical(unsigned f) {
  return guide_features((f & F_FLAT) ? (f & ~(unsigned)F_BVH4) : f);
}
template <unsigned... Fs>
constexpr std::array<GuideFn, sizeof...(Fs)> instance_table(std::integer_sequence<unsigned, Fs...>) {
  return {guides_kernel<canonical(Fs)>...};
}

} // namespace

extern "C" hipError_t rtk_launch_guides(const DScene *S, const DCamera *C, const DLaunch *P, double *out,
                                        hipStream_t stream) {
  static constexpr auto table = instance_table(std::make_integer_sequence<unsigned, F_ALL + 1>{});
  const unsigned f = (unsigned)(S->features & F_ALL);
  const int bw = block_waves(canonical(f));
  const int64_t tiles = (int64_t)P->tiles_x * P->tiles_y;
  if (tiles <= 0 || P->sample_count < 0) return hipSuccess;
  const size_t lds = lds_bytes((int)canonical(f), S->stack_depth, 0);
  hipLaunchKernelGGL(table[f], dim3((unsigned)((tiles + bw - 1) / bw)), dim3(64 * bw), lds, stream, *S, *C, *P,
                     out);
  return hipGetLastError();
}
