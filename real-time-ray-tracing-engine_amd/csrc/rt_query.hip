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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include <array>
#include <utility>

#include "rt_kernels.h"
#include "rt_lds_plan.h"
// rt_path.h's few non-inline host functions are rt_kernel.o's to export: this
// file's copies of the per-path code are its own (as in rt_guides.hip)
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_query.h"
#pragma clang attribute pop

namespace {

using namespace rtq;

template <unsigned F>
__global__ __launch_bounds__(64 * block_waves(F)) void query_kernel(DScene S_, const int32_t *xf_obj, int64_t n,
                                                                    const rt_ray *rays, rt_ray_hit *hits) {
  constexpr int BW = block_waves(F);
  extern __shared__ int4 dyn_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t k = ((int64_t)blockIdx.x * BW + wv) * 64 + lane;
  if (k >= n) return; // rays past n are neither traced nor written; no block-wide barrier below
  const DScene S = query_scene(S_);
  int *stk = reinterpret_cast<int *>(dyn_lds) + wv * S.stack_depth * 64 + lane;
  const rt_ray q = rays[k];
  hits[k] = query_ray<F>(S, xf_obj, q, stk);
}

using QueryFn = void (*)(DScene, const int32_t *, int64_t, const rt_ray *, rt_ray_hit *);

template <unsigned... Fs>
constexpr std::array<QueryFn, sizeof...(Fs)> instance_table(std::integer_sequence<unsigned, Fs...>) {
  return {query_kernel<query_features(Fs)>...};
}

} // namespace

extern "C" hipError_t rtk_launch_trace(const DScene *S, const int32_t *xf_obj, int64_t n, const rt_ray *rays,
                                       rt_ray_hit *hits, hipStream_t stream) {
  static constexpr auto table = instance_table(std::make_integer_sequence<unsigned, F_ALL + 1>{});
  if (n <= 0) return hipSuccess;
  const unsigned f = (unsigned)(S->features & F_ALL);
  const int per_block = 64 * block_waves(query_features(f));
  const int64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t lds = lds_bytes((int)query_features(f), S->stack_depth, 0);
  hipLaunchKernelGGL(table[f], dim3((unsigned)blocks), dim3(64 * block_waves(query_features(f))), lds, stream, *S,
                     xf_obj, n, rays, hits);
  return hipGetLastError();
}
