// rt_adaptive.hip — device side of adaptive sampling (rt_render_tiles_device,
// rt_adaptive_update_device, rt_adaptive_select_device,
// rt_to_bytes_tiles_device, rt_guided_select_device; host side in rt_api.cpp,
// drivers in rtx/adaptive.py and rtx/guided.py).
//
// The render kernel is untouched: a tile-list launch hands it the caller's
// list, copied and clamped here, as its dispatch order (DLaunch.tile_order).
// The kernels below keep per-pixel batch moments of the luminance, turn them
// into one relative standard error per 8x8 tile and compact the tiles that
// still need samples -- in list order, so the result is reproducible.
//
// Arithmetic is fp64 and written operation by operation as
// rtx/adaptive.py: NumpyOps states it (the build contracts nothing:
// -ffp-contract=off), so acc / s1 / s2 agree with it bit for bit; the tile
// error's 64-lane sum is a butterfly, so it agrees to rounding.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_kernels.h"

namespace {

constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ int clamp_tile(int t, int tiles) { return min(max(t, 0), tiles - 1); }

// The caller's tile list -> the scene's order buffer, every entry clamped into
// [0, tiles - 1]: whatever the list holds, the render kernel and
// split_sum_kernel only ever see tiles of the launch's row range.
__global__ void tile_list_copy_kernel(const int32_t *in, int n, int tiles, int32_t *out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = clamp_tile(in[k], tiles);
}

// One wavefront per listed tile, one lane per pixel.
__global__ void __launch_bounds__(64 * kWavesPerBlock)
    adaptive_update_kernel(const double *delta, int batch_strata, const int32_t *list, int n_tiles, int W,
                           int H, int tiles_x, int tiles, double *acc, double *s1, double *s2,
                           int32_t *tile_strata) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (k >= n_tiles) return; // wave-uniform
  const int t = clamp_tile(list[k], tiles);
  const int i = (t % tiles_x) * 8 + (lane & 7), j = (t / tiles_x) * 8 + (lane >> 3);
  if (i < W && j < H) {
    const size_t p = (size_t)j * W + i;
    const double r = delta[3 * p + 0], g = delta[3 * p + 1], b = delta[3 * p + 2];
    acc[3 * p + 0] += r;
    acc[3 * p + 1] += g;
    acc[3 * p + 2] += b;
    const double y = (0.2126 * r + 0.7152 * g + 0.0722 * b) / (double)batch_strata;
    s1[p] += y;
    s2[p] += y * y;
  }
  if (lane == 0) tile_strata[t] += batch_strata;
}

// One wavefront per tile of the input list: the tile's error, and its flag
// into out[k] (the tile itself: still active; -1: retired) for the compaction.
__global__ void __launch_bounds__(64 * kWavesPerBlock)
    adaptive_error_kernel(const double *s1, const double *s2, const int32_t *tile_strata, int batch_strata,
                          int W, int H, int tiles_x, int tiles, double threshold, double floor_,
                          int min_batches, const int32_t *list, int n_in, int32_t *out, double *tile_error) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (k >= n_in) return; // wave-uniform
  const int t = clamp_tile(list[k], tiles);
  const int nb = tile_strata[t] / batch_strata; // batches in the moments
  const int x0 = (t % tiles_x) * 8, y0 = (t / tiles_x) * 8;
  const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
  double rel = 0.0;
  if (nb >= 2 && i < W && j < H) {
    const size_t p = (size_t)j * W + i;
    const double b = (double)nb, a1 = s1[p], a2 = s2[p];
    const double mean = a1 / b;
    double var = (a2 - a1 * a1 / b) / (b - 1.0);
    var = var > 0.0 ? var : 0.0; // max(0, .); NumpyOps writes it as the same comparison
    const double se = sqrt(var / b);
    rel = se / (mean + floor_);
  }
  // 64-lane butterfly sum; lanes outside the image hold 0
  for (int off = 32; off > 0; off >>= 1) rel += __shfl_xor(rel, off);
  if (lane == 0) {
    const int n_px = min(8, W - x0) * min(8, H - y0);
    // fewer than two batches have no variance estimate: the error is infinite
    const double e = nb >= 2 ? rel / (double)n_px : __builtin_huge_val();
    const bool retire = nb >= max(2, min_batches) && e <= threshold;
    out[k] = retire ? -1 : t;
    if (tile_error != nullptr) tile_error[t] = e;
  }
}

// rt_guided_select_device's rule (rtx/guided.py NumpyOps.select states it): one
// wavefront per tile of the input list, one lane per pixel; a 16-B load of the
// displayed frame's col plane (e.r, e.g, e.b, count) and an 8-B load of its
// variance per lane.  The tile's flag goes into out[k] as adaptive_error_kernel
// writes it, for the same compaction.
__global__ void __launch_bounds__(64 * kWavesPerBlock)
    guided_error_kernel(const float4 *col, const double *variance, const int32_t *tile_strata, int strata_now,
                        int W, int H, int tiles_x, int tiles, double threshold, double floor_, double min_count,
                        const int32_t *list, int n_in, int32_t *out, double *tile_error, double *tile_count) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (k >= n_in) return; // wave-uniform
  const int t = clamp_tile(list[k], tiles);
  const double n_c = (double)(tile_strata != nullptr ? max(tile_strata[t], 0) : strata_now);
  const int x0 = (t % tiles_x) * 8, y0 = (t / tiles_x) * 8;
  const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
  double rel = 0.0, cnt = __builtin_huge_val(); // what a lane outside the image contributes
  if (i < W && j < H) {
    const size_t p = (size_t)j * W + i;
    const float4 c = col[p];
    const double r = (double)c.x, g = (double)c.y, b = (double)c.z, stored = (double)c.w;
    const double y = 0.2126 * r + 0.7152 * g + 0.0722 * b;
    double v = variance[p];
    v = v > 0.0 ? v : 0.0; // a NaN or negative variance: 0
    rel = sqrt(v) / (y + floor_);
    // (x - x) is 0 for a finite x and NaN otherwise
    if (r - r != 0.0 || g - g != 0.0 || b - b != 0.0 || rel != rel) rel = __builtin_huge_val();
    cnt = stored > n_c ? stored : n_c; // a stored count of 0 (or NaN): the pixel's own samples
  }
  // 64-lane butterflies: the sum of rel, the minimum of the counts
  for (int off = 32; off > 0; off >>= 1) {
    rel += __shfl_xor(rel, off);
    const double other = __shfl_xor(cnt, off);
    cnt = other < cnt ? other : cnt;
  }
  if (lane == 0) {
    const int n_px = min(8, W - x0) * min(8, H - y0);
    const double e = rel / (double)n_px;
    const bool drop = cnt >= min_count && e <= threshold; // a NaN error keeps the tile
    out[k] = drop ? -1 : t;
    if (tile_error != nullptr) tile_error[t] = e;
    if (tile_count != nullptr) tile_count[t] = cnt;
  }
}

// Order-preserving compaction of the flags in place (entries >= 0 kept), by one
// block: chunks of 1024 x kPer entries, each thread holding kPer consecutive
// ones in registers, a block-wide exclusive scan of the threads' counts, then
// the writes.  A chunk is read completely before any of its writes, and its
// writes land at or below the entries it read, so no later chunk's entry is
// overwritten before it is read.
constexpr int kScanThreads = 1024, kPer = 8;
__global__ void __launch_bounds__(kScanThreads)
    adaptive_compact_kernel(int32_t *list, int n, int32_t *count_out) {
  __shared__ int wave_sum[kScanThreads / 64];
  __shared__ int chunk_total;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int base_out = 0;
  for (int base = 0; base < n; base += kScanThreads * kPer) {
    int v[kPer];
    int mine = 0;
    const int first = base + threadIdx.x * kPer;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      v[q] = first + q < n ? list[first + q] : -1;
      mine += v[q] >= 0;
    }
    int incl = mine; // inclusive scan within the wave
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sum[wv] = incl;
    __syncthreads(); // every read of the chunk done, wave sums visible
    if (threadIdx.x == 0) {
      int run = 0;
      for (int w = 0; w < kScanThreads / 64; ++w) {
        const int c = wave_sum[w];
        wave_sum[w] = run;
        run += c;
      }
      chunk_total = run;
    }
    __syncthreads();
    int o = base_out + wave_sum[wv] + incl - mine;
#pragma unroll
    for (int q = 0; q < kPer; ++q)
      if (v[q] >= 0) list[o++] = v[q];
    base_out += chunk_total;
    __syncthreads(); // wave_sum / chunk_total are rewritten by the next chunk
  }
  if (threadIdx.x == 0) *count_out = base_out;
}

// rt_to_bytes_device's quantisation with each pixel's own tile's scale.
__global__ void to_bytes_tiles_kernel(const double *rgb, const int32_t *tile_strata, int W, int H,
                                      int tiles_x, uint8_t *bytes) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)W * H * 3) return;
  const int64_t pix = idx / 3;
  const int i = (int)(pix % W), j = (int)(pix / W);
  const int n = tile_strata[(j >> 3) * tiles_x + (i >> 3)];
  const double scale = 1.0 / (double)max(1, n);
  const double x = scale * rgb[idx];
  double g = (x > 0) ? sqrt(x) : 0; // ColorUtility.hpp:11-26
  if (g < 0.000) g = 0.000;
  if (g > 0.999) g = 0.999;
  bytes[idx] = (uint8_t)(256 * g);
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

} // namespace

extern "C" hipError_t rtk_launch_tile_list_copy(const int32_t *in, int n, int tiles, int32_t *out,
                                                hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(tile_list_copy_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, stream, in, n, tiles, out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_adaptive_update(const double *delta, int batch_strata, const int32_t *list,
                                                 int n_tiles, int W, int H, double *acc, double *s1,
                                                 double *s2, int32_t *tile_strata, hipStream_t stream) {
  if (n_tiles <= 0) return hipSuccess;
  const int tiles_x = (W + 7) / 8, tiles = tiles_x * ((H + 7) / 8);
  hipLaunchKernelGGL(adaptive_update_kernel, dim3(blocks_of(n_tiles, kWavesPerBlock)),
                     dim3(64 * kWavesPerBlock), 0, stream, delta, batch_strata, list, n_tiles, W, H, tiles_x,
                     tiles, acc, s1, s2, tile_strata);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_adaptive_select(const double *s1, const double *s2,
                                                 const int32_t *tile_strata, int batch_strata, int W, int H,
                                                 double threshold, double floor_, int min_batches,
                                                 const int32_t *list, int n_in, int32_t *out,
                                                 int32_t *count_out, double *tile_error,
                                                 hipStream_t stream) {
  const int tiles_x = (W + 7) / 8, tiles = tiles_x * ((H + 7) / 8);
  if (n_in > 0) {
    hipLaunchKernelGGL(adaptive_error_kernel, dim3(blocks_of(n_in, kWavesPerBlock)),
                       dim3(64 * kWavesPerBlock), 0, stream, s1, s2, tile_strata, batch_strata, W, H, tiles_x,
                       tiles, threshold, floor_, min_batches, list, n_in, out, tile_error);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // n_in 0: the loop body never runs, the count becomes 0
  hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(kScanThreads), 0, stream, out, n_in, count_out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_guided_select(const void *history, const double *variance,
                                               const int32_t *tile_strata, int strata_now, int W, int H,
                                               double threshold, double floor_, double min_count,
                                               const int32_t *list, int n_in, int32_t *out, int32_t *count_out,
                                               double *tile_error, double *tile_count, hipStream_t stream) {
  const int tiles_x = (W + 7) / 8, tiles = tiles_x * ((H + 7) / 8);
  if (n_in > 0) {
    // the col plane is the history's first: 256-B aligned (checked by the caller), so every float4 is 16-B aligned
    hipLaunchKernelGGL(guided_error_kernel, dim3(blocks_of(n_in, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       stream, (const float4 *)history, variance, tile_strata, strata_now, W, H, tiles_x, tiles,
                       threshold, floor_, min_count, list, n_in, out, tile_error, tile_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(kScanThreads), 0, stream, out, n_in, count_out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_to_bytes_tiles(const double *rgb, const int32_t *tile_strata, int W, int H,
                                                uint8_t *bytes, hipStream_t stream) {
  const int64_t total = (int64_t)W * H * 3;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(to_bytes_tiles_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, stream, rgb,
                     tile_strata, W, H, (W + 7) / 8, bytes);
  return hipGetLastError();
}
