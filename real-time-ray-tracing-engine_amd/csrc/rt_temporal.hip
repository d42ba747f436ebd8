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
// rt_temporal_variance_device is a second kernel of the same shape over a
// history with a third plane (the variance of e's luminance).
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

// temporal_kernel with the variance of e's luminance carried along
// (rt_temporal_variance_device): the same lane-per-pixel shape;
// over temporal_kernel's traffic a lane reads its own 8-B variance_now and one
// 4-B var per tap (the taps' row segments again) and writes 8 B variance_out
// and 4 B var -- contiguous per wavefront.
__global__ void __launch_bounds__(kBX *kBY)
    temporal_variance_kernel(rtt::Cam now, rtt::Cam prev, int W, int H, const double *rgb, double scale,
                             const int32_t *tile_strata, int strata_now, const double *guides, double g,
                             const rtt::F4 *pcol, const rtt::F4 *pgeo, const float *pvar, rtt::Coef K,
                             rtt::F4 *ocol, rtt::F4 *ogeo, float *ovar, double *out, const double *v_now,
                             double *v_out) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  rtt::temporal_variance_pixel(now, prev, W, H, x, y, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo,
                               pvar, K, ocol, ogeo, ovar, out, v_now, v_out);
}

// The two kernels above with object motion (rt_temporal_motion_device,
// rt_temporal_variance_motion_device): a lane also reads its own
// 64-B rt_motion record -- contiguous per wavefront, like its guides -- and a
// moved surface pixel projects where its surface point stood.
__global__ void __launch_bounds__(kBX *kBY)
    temporal_motion_kernel(rtt::Cam now, rtt::Cam prev, int W, int H, const double *rgb, double scale,
                           const int32_t *tile_strata, int strata_now, const double *guides, double g,
                           const rtt::F4 *pcol, const rtt::F4 *pgeo, const rt_motion *motion, rtt::Coef K,
                           rtt::F4 *ocol, rtt::F4 *ogeo, double *out) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  rtt::temporal_motion_pixel(now, prev, W, H, x, y, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo,
                             motion, K, ocol, ogeo, out);
}

__global__ void __launch_bounds__(kBX *kBY)
    temporal_variance_motion_kernel(rtt::Cam now, rtt::Cam prev, int W, int H, const double *rgb, double scale,
                                    const int32_t *tile_strata, int strata_now, const double *guides, double g,
                                    const rtt::F4 *pcol, const rtt::F4 *pgeo, const float *pvar,
                                    const rt_motion *motion, rtt::Coef K, rtt::F4 *ocol, rtt::F4 *ogeo, float *ovar,
                                    double *out, const double *v_now, double *v_out) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  rtt::temporal_variance_motion_pixel(now, prev, W, H, x, y, rgb, scale, tile_strata, strata_now, guides, g, pcol,
                                      pgeo, pvar, motion, K, ocol, ogeo, ovar, out, v_now, v_out);
}

} // namespace

extern "C" hipError_t rtk_launch_temporal_variance_motion(const rt_frame *now, const double *rgb, double scale,
                                                          const int32_t *tile_strata, int strata_now,
                                                          const double *guides, int guide_strata,
                                                          const rt_frame *prev, const void *history_prev,
                                                          const rt_motion *motion, const double *variance_now,
                                                          const rt_temporal_params *params, void *history_out,
                                                          double *out, double *variance_out, hipStream_t stream) {
  const int W = now->image_width, H = now->image_height;
  if ((int64_t)W * H <= 0) return hipSuccess;
  const size_t plane = rtk_history_bytes(W, H) / 2;
  const rtt::Coef K = rtt::coef_of(params);
  const char *hp = static_cast<const char *>(history_prev);
  char *ho = static_cast<char *>(history_out);
  const rtt::F4 *pcol = reinterpret_cast<const rtt::F4 *>(hp);
  const rtt::F4 *pgeo = hp ? reinterpret_cast<const rtt::F4 *>(hp + plane) : nullptr;
  const float *pvar = hp ? reinterpret_cast<const float *>(hp + 2 * plane) : nullptr;
  const rtt::Cam cn = rtt::cam_of(*now), cp = rtt::cam_of(prev ? *prev : *now);
  const dim3 grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
  hipLaunchKernelGGL(temporal_variance_motion_kernel, grid, dim3(kBX * kBY), 0, stream, cn, cp, W, H, rgb, scale,
                     tile_strata, strata_now, guides, (double)guide_strata, pcol, pgeo, pvar, motion, K,
                     reinterpret_cast<rtt::F4 *>(ho), reinterpret_cast<rtt::F4 *>(ho + plane),
                     reinterpret_cast<float *>(ho + 2 * plane), out, variance_now, variance_out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_temporal_motion(const rt_frame *now, const double *rgb, double scale,
                                                 const int32_t *tile_strata, int strata_now, const double *guides,
                                                 int guide_strata, const rt_frame *prev, const void *history_prev,
                                                 const rt_motion *motion, const rt_temporal_params *params,
                                                 void *history_out, double *out, hipStream_t stream) {
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
  hipLaunchKernelGGL(temporal_motion_kernel, grid, dim3(kBX * kBY), 0, stream, cn, cp, W, H, rgb, scale, tile_strata,
                     strata_now, guides, (double)guide_strata, pcol, pgeo, motion, K, ocol, ogeo, out);
  return hipGetLastError();
}

extern "C" size_t rtk_history_bytes(int W, int H) {
  const size_t plane = (((size_t)W * H * sizeof(rtt::F4)) + 255) & ~(size_t)255;
  return 2 * plane;
}

// a plain history and the var plane (fp32 scalars) behind it
extern "C" size_t rtk_history_variance_bytes(int W, int H) {
  return rtk_history_bytes(W, H) + ((((size_t)W * H * sizeof(float)) + 255) & ~(size_t)255);
}

extern "C" hipError_t rtk_launch_temporal_variance(const rt_frame *now, const double *rgb, double scale,
                                                   const int32_t *tile_strata, int strata_now,
                                                   const double *guides, int guide_strata, const rt_frame *prev,
                                                   const void *history_prev, const double *variance_now,
                                                   const rt_temporal_params *params, void *history_out,
                                                   double *out, double *variance_out, hipStream_t stream) {
  const int W = now->image_width, H = now->image_height;
  if ((int64_t)W * H <= 0) return hipSuccess;
  const size_t plane = rtk_history_bytes(W, H) / 2;
  const rtt::Coef K = rtt::coef_of(params);
  const char *hp = static_cast<const char *>(history_prev);
  char *ho = static_cast<char *>(history_out);
  const rtt::F4 *pcol = reinterpret_cast<const rtt::F4 *>(hp);
  const rtt::F4 *pgeo = hp ? reinterpret_cast<const rtt::F4 *>(hp + plane) : nullptr;
  const float *pvar = hp ? reinterpret_cast<const float *>(hp + 2 * plane) : nullptr;
  const rtt::Cam cn = rtt::cam_of(*now), cp = rtt::cam_of(prev ? *prev : *now);
  const dim3 grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
  hipLaunchKernelGGL(temporal_variance_kernel, grid, dim3(kBX * kBY), 0, stream, cn, cp, W, H, rgb, scale,
                     tile_strata, strata_now, guides, (double)guide_strata, pcol, pgeo, pvar, K,
                     reinterpret_cast<rtt::F4 *>(ho), reinterpret_cast<rtt::F4 *>(ho + plane),
                     reinterpret_cast<float *>(ho + 2 * plane), out, variance_now, variance_out);
  return hipGetLastError();
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
