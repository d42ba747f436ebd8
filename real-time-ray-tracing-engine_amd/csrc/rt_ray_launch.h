// rt_ray_launch.h — the launch shape of the kernels that give a lane one ray
// (HIP only): rt_query.hip, rt_occlusion.hip, rt_radiance.hip,
// and rt_guides.hip with a wave's 8x8 tile for its 64 rays.  One wavefront per
// 64 consecutive rays, blocks of block_waves(F) waves, the dynamic LDS the
// traversal stacks [block_waves(F)][stack_depth][64] alone.
#ifndef RT_RAY_LAUNCH_H
#define RT_RAY_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_lds_plan.h"

namespace rtl {

// A thread's place in a launch of BW-wave blocks.
struct RayLane {
  int wv, lane; // of the block, of the wave
  __device__ __forceinline__ RayLane() : wv(threadIdx.x >> 6), lane(threadIdx.x & 63) {}
  // the wave's number in the launch (the guide kernel's tile), and the lane's ray: a lane whose ray
  // is past n returns before anything else (no block-wide barrier may follow)
  template <int BW> __device__ __forceinline__ int wave() const { return blockIdx.x * BW + wv; }
  template <int BW> __device__ __forceinline__ int64_t ray() const { return ((int64_t)blockIdx.x * BW + wv) * 64 + lane; }
};
// The lane's traversal stack, stride 64, in the block's dynamic LDS.  L by
// value ahead of the depth, wv stored ahead of lane: other forms swap two
// operands of a v_mul_lo_u32 or a v_or3_b32; this one is, instance for
// instance, the text of the kernels that spelt it out (tools/isa_same.py).
__device__ __forceinline__ int *lane_stack(RayLane L, int4 *dyn_lds, int stack_depth) {
  return reinterpret_cast<int *>(dyn_lds) + L.wv * stack_depth * 64 + L.lane;
}

// Queues `kernel`, the instance of `canonical_features`, over n rays: n <= 0
// queues nothing, more than 2^31 - 1 blocks are refused.
template <class... Params, class... Args>
hipError_t launch_per_ray(void (*kernel)(Params...), unsigned canonical_features, int stack_depth, int64_t n,
                          hipStream_t stream, const Args &...args) {
  if (n <= 0) return hipSuccess;
  const int per_block = 64 * block_waves(canonical_features);
  const int64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t lds = lds_bytes((int)canonical_features, stack_depth, 0);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(per_block), lds, stream, args...);
  return hipGetLastError();
}

} // namespace rtl
#endif
