// rt_frame.hip — the small kernels around the render launch: frame assembly
// from chunk partials, the tile-shard exchange, the dispatch-order sort and the
// byte conversion.  Every sum over chunk partials here runs in chunk order
// over the records rt_plan.h assigns, so the frames of every plan consumer
// agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"
#include "rt_plan.h"

namespace {

// A tile's record is 64 pixel slots x 3 channels = 192 doubles; one thread per
// double, consecutive threads on consecutive doubles (coalesced).
constexpr int kTileD = 64 * 3;

unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// Frame assembly after a split frame launch (rtk_launch_split_sum): each pixel
// of a chunked tile gets its stratum-chunk partial sums added in chunk order
// (scaled / accumulated as the launch asks) -- the head tiles' head_chunks
// partials when head_chunks > 1, the tail tiles' n_chunks partials; whole
// tiles' pixels were written by their own units.  One thread per (chunked
// tile, pixel slot, channel).
__global__ void split_sum_kernel(DCamera C, DLaunch P, double *out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int first = plan_first_chunked(P);
  if (idx >= (int64_t)(P.n_local_tiles - first) * kTileD) return;
  const int ch = (int)(idx % 3);
  const int slot = (int)((idx / 3) & 63);
  const int tile = first + (int)(idx / kTileD); // frame launches: tile_first 0, tile_stride 1
  const int pt = P.tile_order != nullptr ? P.tile_order[tile] : tile; // the plan's tile -> the frame's
  const int i = (pt % P.tiles_x) * 8 + (slot & 7), j = P.row_begin + (pt / P.tiles_x) * 8 + (slot >> 3);
  if (i >= C.W || j >= P.row_end) return;
  const int nc = plan_tile_chunks(P, tile);
  const double *p = P.parts + (plan_tile_part0(P, tile) * 64 + slot) * 3 + ch;
  double sum = p[0];
  for (int k = 1; k < nc; ++k) sum += p[(size_t)k * kTileD];
  if (P.output == RT_OUT_SCALED) sum = C.scale * sum;
  double *o = out + ((size_t)(j - P.row_begin) * C.W + i) * 3 + ch;
  *o = P.accumulate ? *o + sum : sum;
}

// ---- tile-shard exchange (multi-GPU: rt_multi_render, rtx/dist.py) ----
// Every kernel below adds chunk partials in chunk order (split_sum_kernel's
// order), so a sharded frame is bit-identical to the one-device frame launch.

// Tile-layout chunk partials [tile][chunk][64][3] -> tile sums [tile][64][3].
__global__ void tiles_sum_kernel(const double *parts, int64_t n_tiles, int chunks, double *out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_tiles * kTileD) return;
  const int64_t tile = idx / kTileD, r = idx - tile * kTileD;
  const double *p = parts + tile * chunks * kTileD + r;
  double sum = p[0];
  for (int c = 1; c < chunks; ++c) sum += p[(int64_t)c * kTileD];
  out[idx] = sum;
}

// One shard's compact tiles finished on its own device: its whole head tiles
// are already in out[lt]; each chunked tile's partials (the launch's parts
// layout, DLaunch) are summed in chunk order into out[lt].
__global__ void shard_finish_kernel(DLaunch P, double *out) {
  const int first = plan_first_chunked(P);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)(P.n_local_tiles - first) * kTileD) return;
  const int lt = first + (int)(idx / kTileD);
  const int r = (int)(idx % kTileD);
  const int nc = plan_tile_chunks(P, lt);
  const double *p = P.parts + plan_tile_part0(P, lt) * kTileD + r;
  double sum = p[0];
  for (int c = 1; c < nc; ++c) sum += p[(int64_t)c * kTileD];
  out[(int64_t)(P.tile_order != nullptr ? P.tile_order[lt] : lt) * kTileD + r] = sum; // the plan's tile -> the launch's
}

// Cost-ordered dispatch (rt_api.cpp "tile order"): the local tiles sorted by
// the cost the previous launch of the same shape measured (tile_cost, 100 MHz
// ticks summed over a tile's units), most expensive first -- the next launch
// dispatches them in that order (longest processing time first), so its last
// units are short ones.  Two segments, one block each: the plan's head tiles
// [0, n_head) among themselves and its tail tiles [n_head, n) among
// themselves, so every tile keeps its own unit split (whole / head chunks /
// tail chunks) and so its sums, bit for bit.  Per block: a histogram of 256
// log-spaced buckets (8 per octave), a descending scan, a scatter; ties land in
// any order (scheduling only).
__global__ void tile_order_kernel(const uint32_t *cost, int n, int n_head, int32_t *order) {
  const int lo = blockIdx.x == 0 ? 0 : n_head, hi = blockIdx.x == 0 ? n_head : n;
  if (lo >= hi) return;
  cost += lo;
  order += lo;
  n = hi - lo;
  __shared__ uint32_t hist[256];
  for (int k = threadIdx.x; k < 256; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  auto bucket = [](uint32_t c) -> int {
    if (c == 0) return 0;
    const int lz = __clz(c);
    return (31 - lz) * 8 + (int)(((c << lz) >> 28) & 7u);
  };
  for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[bucket(cost[i])], 1u);
  __syncthreads();
  if (threadIdx.x == 0) { // exclusive scan from the top bucket down
    uint32_t run = 0;
    for (int k = 255; k >= 0; --k) {
      const uint32_t c = hist[k];
      hist[k] = run;
      run += c;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) order[atomicAdd(&hist[bucket(cost[i])], 1u)] = lo + i;
}

// Compact tiles of n_shards shards -> frame rows [row_begin, row_end): tile t
// of the row range (row-major tile order) is local tile t / n_shards of shard
// t % n_shards, at tiles[(shard * shard_stride + local) * 192].  One thread per
// frame double: the frame writes are coalesced, the tile reads come in runs
// of 8 pixels (192 B).
__global__ void tiles_to_frame_kernel(const double *tiles, int n_shards, int64_t shard_stride, int W,
                                      int row_begin, int row_end, int tiles_x, double scale, int scaled,
                                      int accumulate, double *out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)(row_end - row_begin) * W * 3) return;
  const int ch = (int)(idx % 3);
  const int64_t pix = idx / 3;
  const int i = (int)(pix % W), jr = (int)(pix / W);
  const int t = (jr >> 3) * tiles_x + (i >> 3), slot = (jr & 7) * 8 + (i & 7);
  const int k = t % n_shards, lt = t / n_shards;
  double v = tiles[((int64_t)k * shard_stride + lt) * kTileD + slot * 3 + ch];
  if (scaled) v = scale * v;
  out[idx] = accumulate ? out[idx] + v : v;
}

__global__ void to_bytes_kernel(const double *rgb, int64_t n, double scale, uint8_t *bytes) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * n) return;
  double x = scale * rgb[i];
  double g = (x > 0) ? sqrt(x) : 0; // ColorUtility.hpp:11-26
  if (g < 0.000) g = 0.000;
  if (g > 0.999) g = 0.999;
  bytes[i] = (uint8_t)(256 * g);
}

} // namespace

// ---------------------------------------------------------------- launchers
extern "C" hipError_t rtk_launch_split_sum(const DCamera *C, const DLaunch *P, double *out, hipStream_t stream) {
  const int64_t total = (int64_t)(P->n_local_tiles - plan_first_chunked(*P)) * kTileD;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(split_sum_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, *C, *P, out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_shard_finish(const DLaunch *P, double *out, hipStream_t stream) {
  const int64_t total = (int64_t)(P->n_local_tiles - plan_first_chunked(*P)) * kTileD;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(shard_finish_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, *P, out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_tiles_sum(const double *parts, int64_t n_tiles, int chunks, double *out,
                                           hipStream_t stream) {
  if (n_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(tiles_sum_kernel, dim3(blocks_for(n_tiles * kTileD)), dim3(256), 0, stream, parts,
                     n_tiles, chunks, out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_tile_order(const uint32_t *cost, int n, int n_head, int32_t *order,
                                            hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(tile_order_kernel, dim3(2), dim3(1024), 0, stream, cost, n, n_head, order);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_tiles_to_frame(const double *tiles, int n_shards, int64_t shard_stride,
                                                int W, int row_begin, int row_end, double scale, int scaled,
                                                int accumulate, double *out, hipStream_t stream) {
  const int64_t total = (int64_t)(row_end - row_begin) * W * 3;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(tiles_to_frame_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, tiles, n_shards,
                     shard_stride, W, row_begin, row_end, (W + 7) / 8, scale, scaled, accumulate, out);
  return hipGetLastError();
}

extern "C" hipError_t rtk_launch_to_bytes(const double *rgb, int64_t n, double scale, uint8_t *bytes,
                                          hipStream_t stream) {
  const int64_t total = 3 * n;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(to_bytes_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, rgb, n, scale, bytes);
  return hipGetLastError();
}
