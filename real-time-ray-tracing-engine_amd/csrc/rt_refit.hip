// rt_refit.hip — moving spheres: new centres into the sphere records, and the
// world BVH's boxes refitted bottom-up on the GPU, the topology kept.
//
// A tree's child boxes are a pure function of its topology and of its items'
// boxes, and the closest hit does not depend on the tree (every hit is decided
// by the fp64 primitive tests), so after a move the scene renders exactly as a
// freshly built one at the new positions -- only slower the further the
// spheres have drifted from where the topology was chosen (rt_scene_bvh_cost
// tells).  Per move:
//   1. move_count / move_apply: one thread per entry; an entry is applied when
//                     its id names a movable sphere once and its centre is
//                     finite (DSphere::c0, and the DRoot copy of a flat world);
//   2. item_boxes:    each world item's fp64 box from the device tables
//                     (rt_refit.h: the scene compiler's rules restated);
//   3. refit:         one thread per node slot; a leaf slot's thread unions
//                     its items' rounded boxes into the slot and arrives at
//                     the node; the last arrival of a node's children unions
//                     the node's slots into the parent's slot and goes on up.
//                     No thread waits for another.  The arrival counter is an
//                     acq_rel agent-scope fetch_add, as in rt_bvh_build.hip's
//                     refit_boxes: the 8 XCDs' L2s are not coherent, the
//                     release / acquire pair is what makes a sibling's slot
//                     visible to the last arrival.
// Transforms and quads of a live scene are edited the same way (xform_count /
// xform_apply, quad_count / quad_apply; rt_live.h holds the entry rules), and
// every update, a sphere move included, is followed by medium_boxes: one thread
// per world medium recomputes DScene::mbox from the medium's boundary items and
// chain (rt_refit.h medium_box), before steps 2 and 3.
// Every refit is a full one over boxes computed from the tables, so the tree
// never depends on the history of moves; unions of fp32 boxes are exact, so
// the result does not depend on the arrival order either.
// The links (each node's parent slot and child count) are built once per scene
// by refit_links, over any node order: linear BVHs are not in BFS order.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_kernels.h"
#include "rt_layout.h"
#include "rt_refit.h"

namespace {

using rt_refit::NodeOf;

// parent[e] = (node << 2) | slot for every inner child e; n_child[i] = the
// node's non-empty slots.  parent[] starts at -1 (the root keeps it).
template <int A>
__global__ void refit_links(const NodeOf<A> *nodes, int n_nodes, int32_t *parent, int32_t *n_child) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  int c = 0;
  for (int k = 0; k < A; ++k) {
    const int32_t e = nodes[i].entry[k];
    if (e == -1) continue;
    ++c;
    if (e >= 0 && e < n_nodes) parent[e] = (i << 2) | k;
  }
  n_child[i] = c;
}

template <int A>
__global__ void refit_slots(NodeOf<A> *nodes, int n_nodes, int n_items, const double *boxes,
                            const int32_t *parent, const int32_t *n_child, unsigned *arrived) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_nodes * A) return;
  int i = t / A, k = t % A;
  const int32_t e = nodes[i].entry[k];
  if (e >= 0 || e == -1) return; // an inner child's slot is its last arrival's; an empty slot stays
  if (((~e) >> 3) + ((~e) & 7) > n_items) return; // a leaf past the items: not this scene's tree
  float lo[3], hi[3];
  rt_refit::leaf_union(e, boxes, lo, hi);
  for (;;) {
    for (int a = 0; a < 3; ++a) {
      nodes[i].lo[a][k] = lo[a];
      nodes[i].hi[a][k] = hi[a];
    }
    // acq_rel at agent scope: releases the slot just written and, for the last
    // arrival, acquires the other slots of the node (written behind another XCD's L2).
    // (In the gfx950 code: the slot's stores, buffer_wbl2 sc1, s_waitcnt vmcnt(0), the
    // add, its wait, buffer_inv sc1, then the loads -- the wait between the write-back
    // and the add is what the hand-off rests on; look for it after a compiler change.)
    const unsigned prev = __hip_atomic_fetch_add(&arrived[i], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)prev + 1 != n_child[i]) return;
    const int32_t p = parent[i];
    if (p < 0) return; // the root: its own box is stored nowhere
    rt_refit::node_union<A>(nodes[i], lo, hi);
    i = p >> 2;
    k = p & 3;
  }
}

__global__ void item_boxes(const DItem *items, int n_items, const DSphere *spheres, const DQuad *quads,
                           const DXform *xforms, double *boxes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const rt_refit::Bx b = rt_refit::item_box(items[i], spheres, quads, xforms);
  for (int a = 0; a < 3; ++a) {
    boxes[6 * (size_t)i + a] = b.lo[a];
    boxes[6 * (size_t)i + 3 + a] = b.hi[a];
  }
}

__device__ __forceinline__ bool move_entry_ok(const RefitMove &m, int j, int32_t &rec) {
  const int32_t id = m.ids[j];
  if (id < 0 || id >= m.n_objects) return false;
  rec = m.sphere_of[id];
  if (rec < 0) return false;
  const double *c = m.centres + 3 * (size_t)j;
  return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
}
// how often each movable object is named (named[] starts at 0): an id named
// twice is applied by neither entry, so the outcome is no race's
__global__ void move_count(RefitMove m) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m.n) return;
  int32_t rec;
  if (move_entry_ok(m, j, rec)) atomicAdd(&m.named[m.ids[j]], 1u);
}
__global__ void move_apply(RefitMove m) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m.n) return;
  int32_t rec;
  if (!move_entry_ok(m, j, rec) || m.named[m.ids[j]] != 1u) return;
  const double *c = m.centres + 3 * (size_t)j;
  for (int a = 0; a < 3; ++a) m.spheres[rec].c0[a] = c[a];
  for (int r = 0; r < m.n_roots; ++r) // a flat world's packed copy (at most RT_FLAT_MAX records)
    if (m.root_items[r].kind == I_SPHERE && m.root_items[r].idx == rec)
      for (int a = 0; a < 3; ++a) m.roots[r].test.c0[a] = c[a];
}

// Live transforms and quads (rt_live.h): count, then apply, as the sphere move
// does; an object named by two acceptable entries is written by neither.
__global__ void xform_count(LiveEdit e) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= e.n) return;
  if (rt_live::transform_entry(e.index, e.ids[j], e.values + 3 * (size_t)j) == rt_live::LIVE_OK)
    atomicAdd(&e.named[e.ids[j]], 1u);
}
__global__ void xform_apply(LiveEdit e) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= e.n) return;
  const double *v = e.values + 3 * (size_t)j;
  if (rt_live::transform_entry(e.index, e.ids[j], v) != rt_live::LIVE_OK || e.named[e.ids[j]] != 1u) return;
  rt_live::apply_transform(e.index, e.ids[j], v, e.xforms);
}
// DQuad::n read in place: record r's normal is normals_of(quads) + kQuadStride * r
const int kQuadStride = sizeof(DQuad) / sizeof(double);
static_assert(sizeof(DQuad) % sizeof(double) == 0 && offsetof(DQuad, n) % sizeof(double) == 0, "DQuad is a row of doubles");
__device__ __forceinline__ const double *normals_of(const DQuad *quads) {
  return reinterpret_cast<const double *>(quads) + offsetof(DQuad, n) / sizeof(double);
}
__global__ void quad_count(LiveEdit e) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= e.n) return;
  double D;
  if (rt_live::quad_entry(e.index, e.ids[j], e.values + 3 * (size_t)j, normals_of(e.quads), kQuadStride, D) == rt_live::LIVE_OK)
    atomicAdd(&e.named[e.ids[j]], 1u);
}
__global__ void quad_apply(LiveEdit e) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= e.n) return;
  const double *c = e.values + 3 * (size_t)j;
  double D;
  if (rt_live::quad_entry(e.index, e.ids[j], c, normals_of(e.quads), kQuadStride, D) != rt_live::LIVE_OK ||
      e.named[e.ids[j]] != 1u)
    return;
  rt_live::apply_quad(e.quads[e.index.quad_of[e.ids[j]]], c, D);
}

// A pose (rt_live.h): one thread per table record, three plain 8-B stores.
__global__ void pose_pack(rt_live::PoseCounts c, const DXform *xforms, const DSphere *spheres, const DQuad *quads,
                          double *pose) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= rt_live::pose_records(c)) return;
  double v[3];
  rt_live::pose_pack(c, k, xforms, spheres, quads, v);
  for (int a = 0; a < 3; ++a) pose[3 * k + a] = v[a];
}

__global__ void medium_boxes(const DItem *mitems, int n_mitems, const DMedium *media, const DItem *bitems,
                             const DSphere *spheres, const DQuad *quads, const DXform *xforms, float *mbox) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_mitems) return;
  float six[6];
  rt_refit::medium_box(mitems[m], media, bitems, spheres, quads, xforms, six);
  for (int a = 0; a < 6; ++a) mbox[6 * (size_t)m + a] = six[a];
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

struct Temp {
  size_t parent, n_child, arrived, total;
};
Temp layout(int n_nodes) {
  const size_t each = align256(sizeof(int32_t) * (size_t)(n_nodes > 0 ? n_nodes : 1));
  return Temp{0, each, 2 * each, 3 * each};
}

const int B = 256;
int grid(size_t n) { return (int)((n + B - 1) / B); }

template <int A>
hipError_t links(const void *nodes, int n_nodes, void *temp, hipStream_t st) {
  const Temp t = layout(n_nodes);
  char *base = (char *)temp;
  hipError_t e = hipMemsetAsync(base + t.parent, 0xFF, sizeof(int32_t) * (size_t)n_nodes, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(refit_links<A>, dim3(grid(n_nodes)), dim3(B), 0, st, (const NodeOf<A> *)nodes, n_nodes,
                     (int32_t *)(base + t.parent), (int32_t *)(base + t.n_child));
  return hipGetLastError();
}

template <int A>
hipError_t refit(void *nodes, int n_nodes, int n_items, const double *boxes, void *temp, hipStream_t st) {
  const Temp t = layout(n_nodes);
  char *base = (char *)temp;
  hipError_t e = hipMemsetAsync(base + t.arrived, 0, sizeof(unsigned) * (size_t)n_nodes, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(refit_slots<A>, dim3(grid((size_t)n_nodes * A)), dim3(B), 0, st, (NodeOf<A> *)nodes, n_nodes,
                     n_items, boxes, (const int32_t *)(base + t.parent), (const int32_t *)(base + t.n_child),
                     (unsigned *)(base + t.arrived));
  return hipGetLastError();
}

bool tree_ok(int arity, int n_nodes, int n_items) {
  // a node index shares an int with its slot (parent links, the slot threads' index), a leaf's
  // first item with its count
  return (arity == 2 || arity == 4) && n_nodes >= 0 && n_nodes < (1 << 28) && n_items >= 0 && n_items < (1 << 28);
}

} // namespace

extern "C" size_t rtk_refit_temp_bytes(int n_items, int n_nodes) {
  (void)n_items;
  return layout(n_nodes).total;
}

extern "C" hipError_t rtk_refit_links(const void *nodes, int arity, int n_nodes, void *temp, size_t temp_bytes,
                                      hipStream_t st) {
  if (!tree_ok(arity, n_nodes, 0) || !nodes || !temp || temp_bytes < layout(n_nodes).total)
    return hipErrorInvalidValue;
  if (n_nodes == 0) return hipSuccess;
  return arity == 4 ? links<4>(nodes, n_nodes, temp, st) : links<2>(nodes, n_nodes, temp, st);
}

extern "C" hipError_t rtk_refit_boxes(void *nodes, int arity, int n_nodes, int n_items, const double *boxes,
                                      void *temp, size_t temp_bytes, hipStream_t st) {
  if (!tree_ok(arity, n_nodes, n_items) || !nodes || !boxes || !temp || temp_bytes < layout(n_nodes).total)
    return hipErrorInvalidValue;
  if (n_nodes == 0) return hipSuccess;
  return arity == 4 ? refit<4>(nodes, n_nodes, n_items, boxes, temp, st)
                    : refit<2>(nodes, n_nodes, n_items, boxes, temp, st);
}

// The link build and one refit from the caller's boxes (n_items x (lo xyz,
// hi xyz) fp64, in leaf order), over caller buffers: what the tests drive.
// A root leaf (root_leaf > 0) has no nodes: nothing to do.
extern "C" hipError_t rtk_refit(void *nodes, int arity, int n_nodes, int root_leaf, const DItem *items, int n_items,
                                const double *boxes, void *temp, size_t temp_bytes, hipStream_t st) {
  (void)items; // the boxes are given: the item records are not read
  if (root_leaf < 0) return hipErrorInvalidValue;
  if (root_leaf > 0 || n_nodes == 0) return tree_ok(arity, n_nodes, n_items) ? hipSuccess : hipErrorInvalidValue;
  hipError_t e = rtk_refit_links(nodes, arity, n_nodes, temp, temp_bytes, st);
  if (e != hipSuccess) return e;
  return rtk_refit_boxes(nodes, arity, n_nodes, n_items, boxes, temp, temp_bytes, st);
}

extern "C" hipError_t rtk_item_boxes(const DItem *items, int n_items, const DSphere *spheres, const DQuad *quads,
                                     const DXform *xforms, double *boxes, hipStream_t st) {
  if (n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(item_boxes, dim3(grid(n_items)), dim3(B), 0, st, items, n_items, spheres, quads, xforms, boxes);
  return hipGetLastError();
}

extern "C" hipError_t rtk_move_spheres(const RefitMove *m, hipStream_t st) {
  if (m->n <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(m->named, 0, sizeof(unsigned) * (size_t)m->n_objects, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(move_count, dim3(grid(m->n)), dim3(B), 0, st, *m);
  hipLaunchKernelGGL(move_apply, dim3(grid(m->n)), dim3(B), 0, st, *m);
  return hipGetLastError();
}

extern "C" hipError_t rtk_set_transforms(const LiveEdit *e, hipStream_t st) {
  if (e->n <= 0) return hipSuccess;
  hipError_t err = hipMemsetAsync(e->named, 0, sizeof(unsigned) * (size_t)e->index.n_objects, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(xform_count, dim3(grid(e->n)), dim3(B), 0, st, *e);
  hipLaunchKernelGGL(xform_apply, dim3(grid(e->n)), dim3(B), 0, st, *e);
  return hipGetLastError();
}

extern "C" hipError_t rtk_move_quads(const LiveEdit *e, hipStream_t st) {
  if (e->n <= 0) return hipSuccess;
  hipError_t err = hipMemsetAsync(e->named, 0, sizeof(unsigned) * (size_t)e->index.n_objects, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(quad_count, dim3(grid(e->n)), dim3(B), 0, st, *e);
  hipLaunchKernelGGL(quad_apply, dim3(grid(e->n)), dim3(B), 0, st, *e);
  return hipGetLastError();
}

extern "C" hipError_t rtk_pose(const rt_live::PoseCounts *c, const DXform *xforms, const DSphere *spheres,
                               const DQuad *quads, double *pose, hipStream_t st) {
  const int64_t n = rt_live::pose_records(*c);
  if (n <= 0) return hipSuccess;
  if (n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pose_pack, dim3(grid((size_t)n)), dim3(B), 0, st, *c, xforms, spheres, quads, pose);
  return hipGetLastError();
}

extern "C" hipError_t rtk_medium_boxes(const DItem *mitems, int n_mitems, const DMedium *media, const DItem *bitems,
                                       const DSphere *spheres, const DQuad *quads, const DXform *xforms, float *mbox,
                                       hipStream_t st) {
  if (n_mitems <= 0) return hipSuccess;
  hipLaunchKernelGGL(medium_boxes, dim3(grid(n_mitems)), dim3(B), 0, st, mitems, n_mitems, media, bitems, spheres,
                     quads, xforms, mbox);
  return hipGetLastError();
}
