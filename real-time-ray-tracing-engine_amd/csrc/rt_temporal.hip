// rt_temporal.hip — temporal reprojection of the displayed frame
// (rt_temporal_device; statement of record: rtx/temporal.py NumpyOps.temporal,
// DESIGN.md §7e).  The per-pixel code is rt_temporal.h, shared with the host twin.
//
// One lane per pixel in the filter's blocks of 64 x 4 pixels: a wavefront is
// one 64-pixel row segment, so its own reads (24 B rgb, 64 B guides per lane)
// and writes (two 16-B history stores, 24 B out) are contiguous, and its four
// taps land on row segments of the previous planes shifted by the camera
// move -- near-contiguous 16-B-per-lane loads.  No atomics, no LDS; every pixel
// writes its own outputs once, so two runs are bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"
#include "rt_temporal.h"

namespace {

constexpr int kBX = 64, kBY = 4;

__global__ void __launch_bounds__(kBX *kBY)
    temporal_kernel(rtt::Cam now, rtt::Cam prev, int W, int H, const double *rgb, double scale,
                    const int32_t *tile_strata, int strata_now, const double *guides, double g,
                    const rtt::F4 *pcol, const rtt::F4 *pgeo, rtt::Coef K, rtt::F4 *ocol, rtt::F4 *ogeo,
                    double *out) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  rtt::temporal_pixel(now, prev, W, H, x, y, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo, K,
                      ocol, ogeo, out);
}

} // namespace

extern "C" size_t rtk_history_bytes(int W, int H) {
  const size_t plane = (((size_t)W * H * sizeof(rtt::F4)) + 255) & ~(size_t)255;
  return 2 * plane;
}

extern "C" hipError_t rtk_launch_temporal(const rt_frame *now, const double *rgb, double scale,
                                          const int32_t *tile_strata, int strata_now, const double *guides,
                                          int guide_strata, const rt_frame *prev, const void *history_prev,
                                          const rt_temporal_params *params, void *history_out, double *out, hipStream_t stream) {
  const int W = now->image_width, H = now->image_height;
  if ((int64_t)W * H <= 0) return hipSuccess;
  const size_t plane = rtk_history_bytes(W, H) / 2;
  const rtt::Coef K = rtt::coef_of(params);
  const rtt::F4 *pcol = static_cast<const rtt::F4 *>(history_prev);
  const rtt::F4 *pgeo =
      history_prev ? reinterpret_cast<const rtt::F4 *>(static_cast<const char *>(history_prev) + plane) : nullptr;
  rtt::F4 *ocol = static_cast<rtt::F4 *>(history_out);
  rtt::F4 *ogeo = reinterpret_cast<rtt::F4 *>(static_cast<char *>(history_out) + plane);
  const rtt::Cam cn = rtt::cam_of(*now), cp = rtt::cam_of(prev ? *prev : *now);
  const dim3 grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
  hipLaunchKernelGGL(temporal_kernel, grid, dim3(kBX * kBY), 0, stream, cn, cp, W, H, rgb, scale, tile_strata,
                     strata_now, guides, (double)guide_strata, pcol, pgeo, K, ocol, ogeo, out);
  return hipGetLastError();
}
