// rt_collapse.hip — the binary world BVH collapsed to 4-wide nodes on the GPU:
// rt_scene.cpp's collapse_bvh4, level by level.
//
// collapse_bvh4 is a BFS over 4-wide nodes whose every expansion is local
// (rt_collapse.h: the source binary node and at most two more), so the nodes
// of one 4-wide level are independent.  Per level:
//   collapse_expand  one thread per 4-wide node of the level: its children
//                    from its source binary node (rt_collapse::expand, the
//                    host's own source), the DNode4 written with the inner
//                    entries still naming binary nodes, and the node's count
//                    of inner children;
//   exclusive scan   (hipCUB) of those counts: the rank of each node's first
//                    inner child among the next level's nodes;
//   collapse_link    one thread per node: its inner slots, in slot order, get
//                    the indices next_level_base + rank + j, and the binary
//                    nodes they named become the next level's source list.
// That is the host's BFS numbering exactly -- level by level, parent order,
// slot order -- so the bytes are collapse_bvh4's (tests/test_collapse_gpu.py).
// The size of the next level goes to the host once per level (two ints and a
// synchronisation, as rtk_build_sah does): the launches are sized to the level
// and the host can refuse a "tree" that would outgrow the output.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "rt_collapse.h"
#include "rt_kernels.h"
#include "rt_layout.h"

namespace {

__global__ void collapse_expand(const DNode *bin, int n_bin, const int *src, int level_size, DNode4 *level_out,
                                int *inner) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= level_size) return;
  rt_collapse::Child c[4];
  rt_collapse::expand(bin, n_bin, src[t], c);
  const DNode4 q = rt_collapse::node_of(c);
  int count = 0;
  for (int i = 0; i < 4; ++i) count += rt_collapse::is_inner(q.entry[i], n_bin) ? 1 : 0;
  level_out[t] = q;
  inner[t] = count;
}

__global__ void collapse_link(DNode4 *level_out, int n_bin, int level_size, const int *rank, int next_base,
                              int *src_next) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= level_size) return;
  int r = rank[t];
  for (int i = 0; i < 4; ++i) {
    const int32_t e = level_out[t].entry[i];
    if (!rt_collapse::is_inner(e, n_bin)) continue;
    src_next[r] = e;
    level_out[t].entry[i] = next_base + r;
    ++r;
  }
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

size_t scan_bytes(int n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int *)nullptr, (int *)nullptr, n);
  return b;
}

struct Temp {
  size_t src0, src1, inner, rank, cub, total;
};
Temp layout(int n_nodes) {
  const int n = n_nodes > 0 ? n_nodes : 1;
  const size_t each = align256(sizeof(int) * (size_t)n); // a level holds at most every node
  Temp t;
  t.src0 = 0;
  t.src1 = each;
  t.inner = 2 * each;
  t.rank = 3 * each;
  t.cub = 4 * each;
  t.total = t.cub + align256(scan_bytes(n));
  return t;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

const int B = 256;
int grid(int n) { return (n + B - 1) / B; }

} // namespace

extern "C" size_t rtk_collapse4_temp_bytes(int n_nodes) { return layout(n_nodes).total; }

// bin: n_nodes binary nodes, root 0, in any order; out: room for n_nodes DNode4 records, of which
// the first *n_nodes4 are written; *levels: the 4-wide levels (the longest root-to-node path).
// Refused before anything is queued: n_nodes < 1, a null pointer, a short temp, buffers that
// overlap.  A "tree" whose entries reach more than n_nodes 4-wide nodes (a node named twice) is
// refused at the level that would pass the output's end, with nothing written past it.
// Synchronises `st` once per level.
extern "C" hipError_t rtk_collapse4(const DNode *bin, int n_nodes, DNode4 *out, void *temp, size_t temp_bytes,
                                    int *n_nodes4, int *levels, hipStream_t st) {
  if (n_nodes < 1 || !bin || !out || !temp || !n_nodes4 || !levels) return hipErrorInvalidValue;
  const Temp t = layout(n_nodes);
  if (temp_bytes < t.total) return hipErrorInvalidValue;
  const size_t in_bytes = sizeof(DNode) * (size_t)n_nodes, out_bytes = sizeof(DNode4) * (size_t)n_nodes;
  if (overlap(bin, in_bytes, out, out_bytes) || overlap(bin, in_bytes, temp, t.total) ||
      overlap(out, out_bytes, temp, t.total))
    return hipErrorInvalidValue;
  char *base = (char *)temp;
  int *src[2] = {(int *)(base + t.src0), (int *)(base + t.src1)};
  int *inner = (int *)(base + t.inner), *rank = (int *)(base + t.rank);
  hipError_t e = hipMemsetAsync(src[0], 0, sizeof(int), st); // the root's source: binary node 0
  if (e != hipSuccess) return e;
  int level_size = 1, level_base = 0, cur = 0, lev = 0;
  while (level_size > 0) {
    ++lev;
    DNode4 *level_out = out + level_base;
    hipLaunchKernelGGL(collapse_expand, dim3(grid(level_size)), dim3(B), 0, st, bin, n_nodes, src[cur], level_size,
                       level_out, inner);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t cb = t.total - t.cub;
    if ((e = hipcub::DeviceScan::ExclusiveSum(base + t.cub, cb, inner, rank, level_size, st)) != hipSuccess) return e;
    int tail[2];
    if ((e = hipMemcpyAsync(&tail[0], rank + level_size - 1, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(&tail[1], inner + level_size - 1, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
      return e;
    const int next_size = tail[0] + tail[1], next_base = level_base + level_size;
    if (next_size < 0 || next_size > n_nodes - next_base) return hipErrorInvalidValue; // not a tree of n_nodes
    if (next_size > 0) { // the last level holds leaves only: complete as expanded, and waited for above
      hipLaunchKernelGGL(collapse_link, dim3(grid(level_size)), dim3(B), 0, st, level_out, n_nodes, level_size, rank,
                         next_base, src[cur ^ 1]);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    level_base = next_base;
    level_size = next_size;
    cur ^= 1;
  }
  *n_nodes4 = level_base;
  *levels = lev;
  return hipSuccess;
}
