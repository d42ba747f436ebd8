// rt_api.cpp — implementation of include/rt_api.h on the HIP runtime.
//
// Ownership model (replaces the reference's singleton CudaSceneContext with its
// __device__ d_scene_context symbol, CudaSceneContext.cuh:25-181 / .cu:9-38):
// every rt_scene owns one device allocation holding all of its tables, a HIP
// stream, two timing events and a lazily grown output buffer.  Nothing is global,
// so several scenes (and several devices) coexist.  Errors never exit() or throw
// across the ABI: they return a negative code and set a thread-local message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_kernels.h"
#include "rt_layout.h"
#include "rt_lds_plan.h"
#include "rt_plan.h"
#include "rt_live_check.h"
#include "rt_scene.h"
// radiance_camera; rt_path.h's few non-inline host functions are rt_kernel.o's to export
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "rt_radiance.h"
#pragma clang attribute pop

struct rt_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  char *block = nullptr; // all scene tables
  size_t block_bytes = 0;
  DScene ds;
  rt_scene_info info;
  double *out_buf = nullptr; // rt_render staging
  size_t out_bytes = 0;
  unsigned long long *stats = nullptr;
  int32_t *unit_ctr = nullptr; // work-unit counter of persistent launches (scene block)
  double *scratch = nullptr; // chunk partials of chunked frame launches
  size_t scratch_bytes = 0;
  double *probe_buf = nullptr; // output of the tile-order probe (tile_order_probe)
  size_t probe_bytes = 0;
  int wave_slots = 0;        // resident waves of the render instance on this device
  int pc_grid = 0;           // resident blocks of the persistent instance on this device
  double binary_cost = -1.0; // SAH cost of the binary tree when the device holds the 4-wide one
  rt_tuning tune{};          // explicit tuning (rt_scene_create_tuned; zero: the default plan)
  // cost-ordered dispatch ("tile order", launch()): per-tile unit costs
  // measured by the shape's probe launch (or, in the launches that measure
  // their own, by the last launch) and two order buffers: the one a launch
  // reads, the one the sort after a measuring launch writes for the next
  // ... one slot per launch shape (signature), least recently used replaced:
  // a scene that alternates tile subsets (several ranks' shares on one
  // device) keeps an order for each instead of probing one slot again
  struct OrderSlot {
    uint32_t *tile_cost = nullptr; // one allocation: the costs, then the two orders
    int32_t *tile_order[2] = {nullptr, nullptr};
    size_t bytes = 0;
    int cur = 0;
    bool ready = false;
    int32_t sig[10] = {};
    uint64_t used = 0; // launch counter at the slot's last use
  };
  static constexpr int kOrderSlots = 4;
  OrderSlot order[kOrderSlots];
  uint64_t order_clock = 0;
  // the caller's tile list of a tile-list launch (rt_render_tiles_device),
  // copied and clamped on the device: that launch's dispatch order.  Its own
  // buffer, outside the order slots: a list changes at every reselection
  int32_t *list_order = nullptr;
  size_t list_bytes = 0;
  // The scene's launches form one chain across streams: `last` is recorded
  // after each call's last kernel on its stream, and a launch on another
  // stream first waits for it (order_after_last) -- the launches share the
  // work-unit counter, the scratch and the order slots, so two of them must
  // never overlap, whichever streams the caller passes.  The last launch's
  // completion therefore implies all earlier ones': destroy and buffer growth
  // wait for `last` and the scene's own stream -- not for the whole device.
  hipEvent_t last = nullptr;
  hipStream_t last_st = nullptr;
  bool has_last = false;
  // Moving spheres (rt_scene_move_spheres*).  Kept from creation: per object of
  // the description its sphere record when it is a movable world sphere, -1
  // when it is not among the world's primitive items as a sphere, -2 when it
  // (also) bounds a medium; the world items' count and the tree's width.  The
  // first move allocates `refit` -- that table, the per-object counters of a
  // move, the items' fp64 boxes and rt_refit.hip's links and arrival counters
  // -- and builds the links; `move_buf` stages the host variant's arrays.
  std::vector<int32_t> sphere_of;
  int32_t n_items = 0, bvh_arity = 2;
  char *refit = nullptr;
  size_t refit_named = 0, refit_boxes = 0, refit_temp = 0, refit_temp_bytes = 0;
  // Live transforms and quads (rt_scene_set_transforms*, rt_scene_move_quads*).  Kept from
  // creation: the compiler's per-object index (HostScene::xf_kind, xf_first, xf_recs, quad_of)
  // and each quad record's unit normal (3 doubles), which the host variants' checks read.
  // `refit` holds the index's device copy at these offsets, `named` serves every kind of edit.
  std::vector<int32_t> xf_kind, xf_first, xf_recs, quad_of;
  std::vector<double> quad_n;
  size_t refit_xf_kind = 0, refit_xf_first = 0, refit_xf_recs = 0, refit_quad_of = 0;
  char *move_buf = nullptr;
  size_t move_bytes = 0;
  // Rebuilding the world tree (rt_scene_rebuild_bvh).  Kept from creation: the
  // world items in compile order -- what a device build starts from, whatever
  // order the live table's leaves have put them in -- the counts the
  // residency plan reads, the binary tree's depth and the 4-wide tree's levels,
  // and the room of the block's node range.  The first rebuild allocates
  // `rebuild` (the Rebuild offsets: those items, their boxes, the staged binary
  // tree, 4-wide tree and leaf-ordered items, the builder's and the collapse's
  // temp) and keeps it; `own_nodes` is the node range of a host-built scene,
  // whose block holds its creation tree and no more.
  std::vector<DItem> compile_items;
  int32_t n_spheres = 0, n_perlin = 0;
  int32_t n_xforms = 0, n_quads = 0; // with n_spheres: a pose's layout (rt_live.h PoseCounts)
  int32_t bvh_depth = 0, bvh_depth4 = 0;
  size_t node_room = 0; // bytes of the node range d.nodes points into
  struct Rebuild { // offsets into `rebuild`; the builder and the collapse run in turn and share temp
    size_t items = 0, boxes = 0, nodes = 0, nodes4 = 0, sorted = 0, temp = 0, temp_bytes = 0;
  } rb;
  char *rebuild = nullptr;
  char *own_nodes = nullptr;
  // Ray queries (rt_trace*).  `xf_obj`: per xforms[] record the object it came
  // from (rtx::xform_objects), uploaded at creation -- its own allocation, so
  // the block and the DScene are what they were; `trace_buf` stages the host
  // variants' rays and results (query_from_host).
  int32_t *xf_obj = nullptr;
  char *trace_buf = nullptr;
  size_t trace_bytes = 0;
};

namespace {

thread_local std::string g_err;

int set_err(int code, const std::string &m) {
  g_err = m;
  return code;
}

int hip_err(hipError_t e, const char *what) {
  return set_err(RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

struct DeviceGuard { // restore the caller's current device
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// Scene memory is stream-ordered: hipMallocFromPoolAsync / hipFreeAsync on the
// scene's own stream.  A plain hipFree -- and hipFreeAsync of hipMalloc'd memory --
// waits for every stream of the device (tools/free_probe.hip on gfx950: 300 ms
// behind another stream's 300 ms kernel); hipFreeAsync of pool memory returns
// at once.  So destroying or growing one scene waits only for that scene's own
// work (wait_scene), never for other scenes or threads on the device.
// The allocations come from the library's own pool on the scene's device,
// which keeps freed memory reserved for the next scene or buffer (release
// threshold UINT64_MAX): with the device's default pool (threshold 0) the
// synchronisation after the frees handed the memory back to the system and
// waited for the whole device to do so (tests/test_scene_lifetime.py: a
// destroy waited out another scene's 300 ms render that way).
hipMemPool_t scene_pool(int device) {
  static std::mutex mu;
  static std::vector<hipMemPool_t> pools;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)pools.size() <= device) pools.resize(device + 1, nullptr);
  if (!pools[device]) {
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = device;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) return nullptr;
    uint64_t keep = ~0ull;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    pools[device] = pool;
  }
  return pools[device];
}
// A destroyed scene's buffers, idle (the destroy waited for the scene's last
// launch) but not yet freed: destroy enqueues nothing on any stream, since a
// HIP stream may share one of the device's few hardware queues
// (GPU_MAX_HW_QUEUES) with another scene's busy stream, and anything queued
// behind that stream's kernel -- a free, a synchronisation -- waits for it
// (tests/test_scene_lifetime.py measured exactly that).  The next allocation
// on the device frees them on its own stream, stream-ordered, before it
// allocates; what no later allocation reaps is released at process exit.
struct Graveyard {
  std::mutex mu;
  std::vector<std::pair<int, void *>> ptrs; // (device, pool allocation)
};
Graveyard &graveyard() {
  static Graveyard *g = new Graveyard(); // never destroyed: usable from any static destructor
  return *g;
}
template <class T>
void bury(rt_scene *s, T *&p) {
  if (p) {
    Graveyard &g = graveyard();
    std::lock_guard<std::mutex> lock(g.mu);
    g.ptrs.emplace_back(s->device, (void *)p);
  }
  p = nullptr;
}
void reap(rt_scene *s) {
  Graveyard &g = graveyard();
  std::lock_guard<std::mutex> lock(g.mu);
  auto keep = g.ptrs.begin();
  for (auto &e : g.ptrs) {
    if (e.first == s->device) (void)hipFreeAsync(e.second, s->stream);
    else *keep++ = e;
  }
  g.ptrs.erase(keep, g.ptrs.end());
}
hipError_t scene_alloc(rt_scene *s, void **p, size_t bytes) {
  *p = nullptr;
  reap(s); // earlier scenes' idle buffers back into the pool first
  hipMemPool_t pool = scene_pool(s->device);
  if (!pool) return hipErrorOutOfMemory;
  hipError_t e = hipMallocFromPoolAsync(p, std::max<size_t>(bytes, 1), pool, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream); // usable from any stream from here on
  if (e != hipSuccess) *p = nullptr;
  return e;
}
template <class T>
void scene_free(rt_scene *s, T *&p) { // after wait_scene: nothing still reads p
  if (p) (void)hipFreeAsync((void *)p, s->stream);
  p = nullptr;
}
hipError_t upload(rt_scene *s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s->stream);
  return e == hipSuccess ? hipStreamSynchronize(s->stream) : e;
}
// everything this scene has launched has completed: its own stream, and its
// last launch (which every earlier launch precedes: order_after_last)
void wait_scene(rt_scene *s) {
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->has_last) (void)hipEventSynchronize(s->last);
}
// Grows one of the scene's buffers to `bytes` (its contents are not kept).
// `idle` says what to wait for before the old buffer is freed -- where the
// buffers differ: the scene's launches on any stream (what every launch reads:
// scratch, probe output, tile list, order slots), the scene's own stream only
// (out_buf, which no other stream writes), or nothing (rt_multi's staging:
// the last rt_multi_render synchronised every stream that used it).
enum class Idle { AfterScene, AfterStream, Already };
template <class T>
int grow(rt_scene *s, T *&buf, size_t &have, size_t bytes, Idle idle, const char *what) {
  if (have >= bytes) return RT_OK;
  if (buf && idle == Idle::AfterScene) wait_scene(s);
  if (buf && idle == Idle::AfterStream) (void)hipStreamSynchronize(s->stream);
  scene_free(s, buf);
  have = 0;
  hipError_t e = scene_alloc(s, (void **)&buf, bytes);
  if (e != hipSuccess) return set_err(RT_ERR_OOM, std::string(what) + ": " + hipGetErrorString(e));
  have = bytes;
  return RT_OK;
}
// before a call's first kernel on st: after the scene's previous launch
int order_after_last(rt_scene *s, hipStream_t st) {
  if (!s->has_last || s->last_st == st) return RT_OK;
  hipError_t e = hipStreamWaitEvent(st, s->last, 0);
  return e == hipSuccess ? RT_OK : hip_err(e, "hipStreamWaitEvent");
}
// after a call's last kernel on st
int mark_last(rt_scene *s, hipStream_t st) {
  hipError_t e = hipEventRecord(s->last, st);
  if (e != hipSuccess) return hip_err(e, "hipEventRecord");
  s->last_st = st;
  s->has_last = true;
  return RT_OK;
}

// the shared launch validation (rt_scene.cpp; the CPU backend applies the same)
int to_device_camera(const rt_frame *f, DCamera &c) {
  std::string err;
  int rc = rtx::device_camera(f, c, err);
  return rc ? set_err(rc, err) : RT_OK;
}

int to_launch(const rt_frame *f, const rt_render_params *p, DLaunch &L) {
  std::string err;
  int rc = rtx::launch_geometry(f, p, L, err);
  return rc ? set_err(rc, err) : RT_OK;
}

// doubles an output of this launch covers
size_t out_doubles(const rt_frame *f, const DLaunch &L) {
  if (L.compact) return (size_t)L.n_local_tiles * L.n_chunks * 64 * 3;
  return (size_t)f->image_width * (L.row_end - L.row_begin) * 3;
}

} // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char *rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(int32_t *count) {
  if (!count) return set_err(RT_ERR_INVALID, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return hip_err(e, "hipGetDeviceCount");
  }
  *count = n;
  return RT_OK;
}

int rt_camera_setup(const rt_camera_desc *camera, rt_frame *frame) {
  std::string err;
  int rc = rtx::camera_setup(camera, frame, err);
  if (rc != RT_OK) return set_err(rc, err);
  return RT_OK;
}

// Builds the world BVH on the device over the scene's world items (uploaded in
// scene order at `items`): the binned-SAH builder (rt_bvh_sah.hip) or the linear
// BVH (rt_bvh_build.hip); writes the nodes and the items in leaf order in place.
// Depth at which the device SAH builder switches to balanced splits (the host
// builder's force_median bound); rt_tuning.sah_stack_budget lowers it in tests.
static int sah_stack_budget(const rt_tuning &t) {
  int b = RT_STACK_DEPTH - 2;
  if (t.sah_stack_budget > 0) b = std::max(1, std::min(b, (int)t.sah_stack_budget));
  return b;
}
struct DeviceTree {
  int n_nodes = 0, depth = -1, root_leaf = 0;
};
static hipError_t device_bvh_build(rt_scene *s, const rtx::HostScene &H, DNode *nodes,
                                   DItem *items, DeviceTree &tree) {
  const int n = (int)H.items.size();
  const bool sah = H.device_bvh == RT_BVH_DEVICE_SAH;
  const size_t a_box = (6 * sizeof(double) * n + 255) & ~size_t(255);
  const size_t a_items = (sizeof(DItem) * n + 255) & ~size_t(255);
  const size_t lb = sah ? rtk_sah_temp_bytes(n) : rtk_lbvh_temp_bytes(n);
  const size_t total = a_box + a_items + 256 + lb;
  char *tmp = nullptr;
  hipError_t e = scene_alloc(s, (void **)&tmp, total);
  if (e != hipSuccess) return e;
  double *d_box = (double *)tmp;
  DItem *d_sorted = (DItem *)(tmp + a_box);
  int *d_depth = (int *)(tmp + a_box + a_items);
  void *d_lb = tmp + a_box + a_items + 256;
  e = hipMemcpyAsync(d_box, H.item_boxes.data(), 6 * sizeof(double) * n, hipMemcpyHostToDevice,
                     s->stream);
  if (sah) {
    if (e == hipSuccess)
      e = rtk_build_sah(d_box, items, n, nodes, d_sorted, d_lb, lb, sah_stack_budget(s->tune),
                        &tree.n_nodes, &tree.depth, &tree.root_leaf, s->stream);
  } else {
    tree.n_nodes = n - 1;
    if (e == hipSuccess)
      e = rtk_build_lbvh(d_box, items, n, H.scene_lo, H.scene_hi, nodes, d_sorted, d_depth, d_lb,
                         lb, s->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(&tree.depth, d_depth, sizeof(int), hipMemcpyDeviceToHost, s->stream);
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(items, d_sorted, sizeof(DItem) * n, hipMemcpyDeviceToDevice, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) (void)hipStreamSynchronize(s->stream); // nothing may still use tmp
  scene_free(s, tmp);
  return e;
}

int rt_scene_create(const rt_scene_desc *desc, int32_t device, rt_scene **out) {
  return rt_scene_create_tuned(desc, device, nullptr, out);
}

// ---- rt_scene_create_tuned, step by step.  The half-built scene belongs to a
// ScenePtr: any early return destroys it.
struct SceneDeleter {
  void operator()(rt_scene *s) const { (void)rt_scene_destroy(s); }
};
using ScenePtr = std::unique_ptr<rt_scene, SceneDeleter>;

static int compile_and_validate(const rt_scene_desc *desc, int32_t device, const rt_tuning &tune,
                                rtx::HostScene &H) {
  H.sah_leaf_max = tune.sah_leaf_max;
  H.sah_leaf_split = tune.sah_leaf_split;
  H.sah_trav_x4 = tune.sah_trav_x4;
  H.sah_bins = tune.sah_bins;
  std::string err;
  int rc = rtx::compile_scene(desc, H, err);
  if (rc != RT_OK) return set_err(rc, err);
  // the compacted leaf tests pack (item << 6 | lane) into an int (rt_path.h leaf_share)
  if (H.items.size() >= ((size_t)1 << 25))
    return set_err(RT_ERR_UNSUPPORTED, "more than 2^25 - 1 world primitives");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return hip_err(e, "hipGetDeviceCount");
  if (device < 0 || device >= ndev) return set_err(RT_ERR_INVALID, "device index out of range");
  return RT_OK;
}

// One device allocation, 256-B aligned sub-ranges: the scene's tables
// (rtx::for_each_table, in its order), then the STATS instance's counters and
// the persistent launches' work-unit counter.
struct BlockLayout {
  std::vector<size_t> table_off;
  size_t stats_off = 0, unit_ctr_off = 0, bytes = 0;
};
static BlockLayout layout_block(const rtx::HostScene &H, bool want4) {
  BlockLayout L;
  auto add = [&](size_t bytes) {
    const size_t off = L.bytes;
    L.bytes += align256(bytes ? bytes : 1);
    return off;
  };
  rtx::for_each_table([&](auto, auto hm) {
    using T = typename std::decay_t<decltype(H.*hm)>::value_type;
    // the node range also takes the 4-wide collapse of the binary tree
    // (RT_FEAT_BVH4; <= one 4-wide node per binary node)
    const size_t each = std::is_same<T, DNode>::value && want4 ? sizeof(DNode4) : sizeof(T);
    L.table_off.push_back(add((H.*hm).size() * each));
  });
  L.stats_off = add(RT_N_STATS * sizeof(unsigned long long));
  L.unit_ctr_off = add(sizeof(int32_t));
  return L;
}

// The scene's stream and events, its block, the tables uploaded into it and
// bound to the DScene (the nodes of a device-built tree: the range only).
static int open_scene(int32_t device, const rt_tuning &tune, const rtx::HostScene &H, const BlockLayout &L,
                      ScenePtr &s) {
  s.reset(new rt_scene());
  s->device = device;
  s->tune = tune;
  s->block_bytes = L.bytes;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&s->ev0)) != hipSuccess || (e = hipEventCreate(&s->ev1)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming)) != hipSuccess)
    return hip_err(e, "stream/event create");
  e = scene_alloc(s.get(), (void **)&s->block, L.bytes);
  if (e != hipSuccess)
    return set_err(RT_ERR_OOM, std::string("hipMallocFromPoolAsync scene: ") + hipGetErrorString(e));
  size_t i = 0;
  rtx::for_each_table([&](auto dm, auto hm) {
    const auto &v = H.*hm;
    using T = typename std::decay_t<decltype(v)>::value_type;
    char *dst = s->block + L.table_off[i++];
    s->ds.*dm = (const T *)dst;
    if (std::is_same<T, DNode>::value) // the range's room, to the next table (rt_scene_rebuild_bvh)
      s->node_room = (i < L.table_off.size() ? L.table_off[i] : L.stats_off) - L.table_off[i - 1];
    const bool on_device = std::is_same<T, DNode>::value && H.device_bvh; // built there, below
    if (e == hipSuccess && !v.empty() && !on_device)
      e = upload(s.get(), dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  });
  if (e != hipSuccess) return hip_err(e, "upload scene");
  s->stats = (unsigned long long *)(s->block + L.stats_off);
  s->unit_ctr = (int32_t *)(s->block + L.unit_ctr_off);
  return RT_OK;
}

// The binary world tree: the host's (compile_scene), or built on the device
// in place (rt_bvh_build.hip, rt_bvh_sah.hip) -- rebuilt on the host if the
// device's is deeper than the traversal stack -- and downloaded if it is to be
// collapsed.  Then the scene's counts and instance key (rtx::bind_counts).
static int build_world_tree(rt_scene *s, rtx::HostScene &H, bool want4, int &builder) {
  DScene &d = s->ds;
  DNode *nodes = const_cast<DNode *>(d.nodes);
  DItem *items = const_cast<DItem *>(d.items);
  builder = RT_BVH_HOST;
  if (H.device_bvh) {
    DeviceTree tree;
    hipError_t e = device_bvh_build(s, H, nodes, items, tree);
    if (e != hipSuccess) return hip_err(e, "device BVH build");
    const int max_depth = s->tune.lbvh_max_depth > 0 ? (int)s->tune.lbvh_max_depth : RT_STACK_DEPTH - 1;
    if (tree.depth >= 0 && tree.depth <= max_depth) {
      H.bvh_depth = tree.depth;
      H.nodes.resize(tree.n_nodes); // the device arrays hold the tree; sizes only
      H.root_is_leaf = tree.root_leaf > 0;
      H.n_root_items = tree.root_leaf;
      builder = H.device_bvh;
      if (want4 && !H.root_is_leaf) { // the collapse runs on the host copy
        e = upload(s, H.nodes.data(), nodes, H.nodes.size() * sizeof(DNode), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_err(e, "BVH download");
      }
    } else { // too deep for the per-lane stack: rebuild on the host (depth-capped SAH)
      rtx::build_world_bvh_host(H);
      e = upload(s, nodes, H.nodes.data(), H.nodes.size() * sizeof(DNode), hipMemcpyHostToDevice);
      if (e == hipSuccess) e = upload(s, items, H.items.data(), H.items.size() * sizeof(DItem), hipMemcpyHostToDevice);
      if (e != hipSuccess) return hip_err(e, "BVH upload");
    }
  }
  rtx::bind_counts(d, H);
  d.features |= s->tune.extra_features & 15; // debug: widen the instance
  return RT_OK;
}

// 4-wide world BVH (RT_FEAT_BVH4; want4: asked for, or automatic from
// kBvh4Min primitives): with H.nodes holding the final binary tree, collapse
// it and upload the 4-wide one over the node range -- or keep the binary one
// (collapse4_verdict, rt_lds_plan.h).
static int collapse_world_tree(rt_scene *s, rtx::HostScene &H, bool want4) {
  if (!want4 || H.root_is_leaf || H.nodes.empty()) return RT_OK;
  DScene &d = s->ds;
  const int d4 = rtx::collapse_bvh4(H.nodes, H.nodes4);
  KernelAttrs a4;
  hipError_t e = rtk_instance_attrs(d.features | RT_FEAT_BVH4, 0, &a4);
  if (e != hipSuccess) return hip_err(e, "4-wide BVH upload");
  if (collapse4_verdict(a4, d.features, d4, s->tune.lds_cap) != COLLAPSE4_FITS) {
    H.nodes4.clear();
    return RT_OK;
  }
  s->binary_cost = rtx::bvh_sah_cost(H.nodes);
  H.bvh_arity = 4;
  H.bvh_depth4 = d4;
  e = upload(s, const_cast<DNode *>(d.nodes), H.nodes4.data(), H.nodes4.size() * sizeof(DNode4),
             hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_err(e, "4-wide BVH upload");
  d.features |= RT_FEAT_BVH4;
  d.n_nodes = (int32_t)H.nodes4.size();
  return RT_OK;
}

// The traversal stack and what the scene's blocks keep in LDS: the attributes
// of the instances the scene runs and the device's CU count into the residency
// plan (rt_lds_plan.h), its outcome into the DScene and the wave-slot counts.
// In two steps: plan_residency computes it for a tree of `n_nodes` nodes and
// the depths s->bvh_depth / bvh_depth4 (creation's tree, or the one a rebuild
// has staged) and touches nothing; commit_residency makes it the scene's.
struct Residency {
  int32_t stack_depth = 0;
  SceneLdsPlan p{};
};
static int plan_residency(const rt_scene *s, int32_t n_nodes, int32_t bvh_depth, int32_t bvh_depth4, Residency &r) {
  const DScene &d = s->ds;
  std::string err;
  rtx::HostScene shape; // traversal_stack_depth reads the tree's shape only
  shape.bvh_depth = bvh_depth;
  shape.bvh_arity = s->bvh_arity;
  shape.bvh_depth4 = bvh_depth4;
  r.stack_depth = rtx::traversal_stack_depth(shape, err);
  if (!r.stack_depth) return set_err(RT_ERR_UNSUPPORTED, err);
  LdsPlanInput in{};
  hipError_t e = rtk_instance_attrs(d.features, 0, &in.render);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&in.cus, hipDeviceAttributeMultiprocessorCount, s->device);
  if (RT_PERSIST_F((unsigned)d.features & 63u)) {
    if (e == hipSuccess) e = rtk_instance_attrs(d.features, kPcWaves, &in.pc16);
    if (e == hipSuccess) e = rtk_instance_attrs(d.features, kWaves, &in.pc4);
  }
  // (a failed CU-count query is reported under the same name, as it always was)
  if (e != hipSuccess) return set_err(RT_ERR_DEVICE, std::string("hipFuncGetAttributes: ") + hipGetErrorString(e));
  in.features = d.features;
  in.stack_depth = r.stack_depth;
  in.n_nodes = n_nodes;
  in.n_items = s->n_items;
  in.n_spheres = s->n_spheres;
  in.n_perlin = s->n_perlin;
  r.p = plan_scene_lds(in, s->tune);
  if (r.p.outcome == LDS_UNSUPPORTED)
    return set_err(RT_ERR_UNSUPPORTED, "BVH traversal stacks exceed the per-block LDS limit");
  return RT_OK;
}
static void commit_residency(rt_scene *s, const Residency &r, RtkLdsPlan &plan) {
  DScene &d = s->ds;
  const SceneLdsPlan &p = r.p;
  plan = p.render;
  d.stack_depth = r.stack_depth;
  if (p.outcome == LDS_STACKS_OVER_SHARE)
    std::fprintf(stderr,
                 "rtx: traversal stacks need %d B of LDS per block, above the %d B share at %d "
                 "waves/SIMD: no BVH nodes staged, lower occupancy\n",
                 (int)plan.fixed_bytes, (int)plan.block_budget, (int)plan.waves_per_simd);
  s->wave_slots = p.wave_slots;
  s->pc_grid = p.pc_grid;
  d.n_lds_nodes = p.n_lds_nodes;
  d.pc_waves = p.pc_waves;
  d.n_lds_nodes_pc = p.n_lds_nodes_pc;
  d.lds_items_pc = p.lds_items_pc;
  d.lds_spheres_pc = p.lds_spheres_pc;
  d.lds_perlin = p.lds_perlin;
}

// What a move and a rebuild need of the description after creation
// (rt_scene::sphere_of, compile_items and the counts beside them).  Takes the
// compile-order items out of H: the last reader of H.items is gone by then.
static void keep_movable(rt_scene *s, const rt_scene_desc *desc, rtx::HostScene &H) {
  s->n_items = (int32_t)H.items.size();
  s->n_spheres = (int32_t)H.spheres.size();
  s->n_perlin = (int32_t)H.perlin.size();
  s->n_xforms = (int32_t)H.xforms.size();
  s->n_quads = (int32_t)H.quads.size();
  s->bvh_arity = H.bvh_arity;
  s->bvh_depth = H.bvh_depth;
  s->bvh_depth4 = H.bvh_depth4;
  s->sphere_of.assign(desc->n_objects, -1);
  for (const DItem &it : H.items)
    if (it.kind == I_SPHERE) s->sphere_of[it.id] = it.idx;
  for (const DItem &it : H.bitems)
    if (it.kind == I_SPHERE) s->sphere_of[it.id] = -2;
  s->xf_kind = std::move(H.xf_kind);
  s->xf_first = std::move(H.xf_first);
  s->xf_recs = std::move(H.xf_recs);
  s->quad_of = std::move(H.quad_of);
  s->quad_n.resize(3 * H.quads.size());
  for (size_t q = 0; q < H.quads.size(); ++q)
    for (int a = 0; a < 3; ++a) s->quad_n[3 * q + a] = H.quads[q].n[a];
  // a host build left H.items in leaf order and handed the compile order over;
  // a device build sorted the device's copy only
  s->compile_items = std::move(H.compile_items.empty() ? H.items : H.compile_items);
}

// The ray queries' table (rt_scene::xf_obj), from the live index keep_movable kept.
static int upload_xform_objects(rt_scene *s) {
  const std::vector<int32_t> obj = rtx::xform_objects(s->xf_first, s->xf_recs);
  hipError_t e = scene_alloc(s, (void **)&s->xf_obj, sizeof(int32_t) * obj.size());
  if (e != hipSuccess)
    return set_err(RT_ERR_OOM, std::string("hipMallocFromPoolAsync transform objects: ") + hipGetErrorString(e));
  if (!obj.empty()) e = upload(s, s->xf_obj, obj.data(), sizeof(int32_t) * obj.size(), hipMemcpyHostToDevice);
  return e == hipSuccess ? RT_OK : hip_err(e, "upload transform objects");
}

// The part of rt_scene_info a rebuild changes: the tree's size and depth, who
// built it, and the residency plan that follows from them.
static void fill_tree_info(rt_scene *s, const RtkLdsPlan &plan, int builder) {
  const DScene &d = s->ds;
  rt_scene_info &in = s->info;
  in.n_nodes = d.n_nodes;
  in.bvh_depth = s->bvh_depth;
  in.device_bytes = (int64_t)(s->block_bytes + (s->own_nodes ? s->node_room : 0));
  in.lds_nodes = d.n_lds_nodes;
  in.bvh_builder = builder;
  in.stack_depth = d.stack_depth;
  in.lds_fixed_bytes = plan.fixed_bytes;
  in.lds_block_budget = plan.block_budget;
  in.waves_per_simd = plan.waves_per_simd;
  in.lds_nodes_persistent = d.n_lds_nodes_pc;
  in.lds_prims_persistent = d.lds_items_pc > 0;
  in.persistent_block_waves = d.pc_waves;
  in.lds_perlin = d.lds_perlin;
}

static void fill_info(rt_scene *s, const rtx::HostScene &H, const RtkLdsPlan &plan, int builder) {
  const DScene &d = s->ds;
  rt_scene_info &in = s->info;
  std::memset(&in, 0, sizeof in);
  in.n_leaf_refs = s->n_items; // leaves are item ranges
  in.n_spheres = (int32_t)H.spheres.size();
  in.n_quads = (int32_t)H.quads.size();
  in.n_objects = (int32_t)(s->n_items + H.mitems.size());
  in.n_light_leaves = (int32_t)H.lights.size();
  in.node_bytes = (int32_t)(H.bvh_arity == 4 ? sizeof(DNode4) : sizeof(DNode));
  in.sphere_bytes = (int32_t)sizeof(DSphere);
  in.quad_bytes = (int32_t)sizeof(DQuad);
  in.features = d.features;
  in.bvh_arity = H.bvh_arity;
  in.lds_node_bytes = RT_LDS_NODE_BYTES(d.features);
  fill_tree_info(s, plan, builder);
}

int rt_scene_create_tuned(const rt_scene_desc *desc, int32_t device, const rt_tuning *tuning,
                          rt_scene **out) {
  if (!out) return set_err(RT_ERR_INVALID, "null output pointer");
  *out = nullptr;
  rt_tuning tune{};
  if (tuning) tune = *tuning;
  rtx::HostScene H;
  int rc = compile_and_validate(desc, device, tune, H);
  if (rc != RT_OK) return rc;
  DeviceGuard g(device);
  const bool want4 = rtx::wants_bvh4(desc, H);
  ScenePtr s;
  int builder = RT_BVH_HOST;
  RtkLdsPlan plan{};
  rc = open_scene(device, tune, H, layout_block(H, want4), s);
  if (rc == RT_OK) rc = build_world_tree(s.get(), H, want4, builder);
  if (rc == RT_OK) rc = collapse_world_tree(s.get(), H, want4);
  if (rc != RT_OK) return rc;
  keep_movable(s.get(), desc, H);
  if ((rc = upload_xform_objects(s.get())) != RT_OK) return rc;
  Residency res;
  if ((rc = plan_residency(s.get(), s->ds.n_nodes, s->bvh_depth, s->bvh_depth4, res)) != RT_OK) return rc;
  commit_residency(s.get(), res, plan);
  fill_info(s.get(), H, plan, builder);
  *out = s.release();
  return RT_OK;
}

int rt_scene_info_get(const rt_scene *s, rt_scene_info *info) {
  if (!s || !info) return set_err(RT_ERR_INVALID, "null argument");
  *info = s->info;
  return RT_OK;
}

int rt_scene_destroy(rt_scene *s) {
  if (!s) return RT_OK;
  DeviceGuard g(s->device);
  // launches on caller streams (rt_render_device) may still read the scene's
  // tables and use its scratch / tile-order buffers: wait for this scene's
  // work -- its stream and its last launch on each caller stream -- and no
  // other (stream-ordered frees, scene_alloc)
  wait_scene(s);
  // ... then hand its buffers to the graveyard (no stream operation here:
  // see Graveyard)
  bury(s, s->out_buf);
  bury(s, s->scratch);
  bury(s, s->probe_buf);
  bury(s, s->list_order);
  bury(s, s->refit);
  bury(s, s->move_buf);
  bury(s, s->rebuild);
  bury(s, s->own_nodes);
  bury(s, s->xf_obj);
  bury(s, s->trace_buf);
  for (auto &o : s->order) bury(s, o.tile_cost); // the slot's one allocation
  bury(s, s->block);
  if (s->last) (void)hipEventDestroy(s->last);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
  return RT_OK;
}

// what the planners (rt_plan.cpp) read of the scene's device
static PlanDevice plan_device(const rt_scene *s) { return PlanDevice{s->wave_slots, s->pc_grid, s->ds.pc_waves}; }

// Cost-ordered dispatch ("tile order"): a launch's work units are taken in
// plan order (head units, then the finer tail chunks -- unit index order is
// the dispatcher's and the persistent counter's order), so the launch ends on
// whatever tiles come last.  Tiles differ several-fold in cost (sky vs glass,
// r05t: C2's units 0.2-2.5 ms at one device), and a costly tile met last
// keeps its wave slot busy while the others idle: the one-device C2 frame
// spent 7.7 % of its slot-time idle, an 8-way rank's share 14.5 %.  So the
// first launch of a shape is preceded by a probe that measures its tiles'
// costs (tile_order_probe) and a one-block sort that orders the tiles most
// expensive first (longest processing time first); every launch of the shape
// takes that order: the plan's k-th tile is tile_order[k].  The head tiles are ordered among themselves and
// the tail tiles among themselves (the tail still last), so every tile keeps
// its own split into units -- whole, head chunks or tail chunks -- and so its
// summation grouping: only the schedule moves, and the frames are
// bit-identical with and without it (rt_tuning.no_tile_order,
// tests/test_tile_order.py).  (Ordering across the split, so the cheapest
// tiles became the tail, regrouped those tiles' sums: not bit-identical.)
// The slot of a launch shape: the one holding its signature, else the least
// recently used (its order reset), with room for n tiles.
static int order_slot(rt_scene *s, const int32_t sig[10], int n, rt_scene::OrderSlot *&slot) {
  slot = nullptr;
  for (auto &o : s->order)
    if (o.ready && std::equal(sig, sig + 10, o.sig)) slot = &o;
  if (!slot) {
    slot = &s->order[0];
    for (auto &o : s->order)
      if (o.used < slot->used) slot = &o;
    slot->ready = false;
    std::copy(sig, sig + 10, slot->sig);
  }
  slot->used = ++s->order_clock;
  const size_t each = align256((size_t)n * sizeof(int32_t)); // costs, order 0, order 1
  if (slot->bytes >= 3 * each) return RT_OK;
  slot->ready = false;
  if (int rc = grow(s, slot->tile_cost, slot->bytes, 3 * each, Idle::AfterScene, "hipMallocFromPoolAsync tile order"))
    return rc;
  slot->tile_order[0] = (int32_t *)((char *)slot->tile_cost + each);
  slot->tile_order[1] = (int32_t *)((char *)slot->tile_cost + 2 * each);
  return RT_OK;
}

// The order of a launch shape: one launch of the STATS instance over the same
// tiles -- whole tiles of at most kProbeStrata strata each (rt_tuning
// probe_strata), into a scratch buffer -- adds each tile's duration to the
// slot's cost counters, and the sort orders the plan's head and tail tiles by
// them.  Once per launch shape (order slot); the launches of the shape then
// take the order.  The render instances measure nothing themselves: the cost
// bookkeeping compiled into them cost C4 12.5 % (r05u_ab.log) and C2 / C3 / C5
// 0.9 % (r06y_ab_C*.log), while a once-per-shape order ranks the tiles as well
// as one re-measured after every launch (r06x / r06y).
// L: the launch with its plan applied (the sort keeps its head and tail apart).
static int tile_order_probe(rt_scene *s, const DCamera &C, const DLaunch &L, rt_scene::OrderSlot *os,
                            hipStream_t st) {
  // 16 strata: C4 +0.2 % over 4 (r06u), C2 +0.6 % / C3 +0.9 % over 4 and 1 (r06aa)
  constexpr int kProbeStrata = 16;
  const size_t bytes = std::max<size_t>(1, (size_t)L.n_local_tiles * 64 * 3) * sizeof(double);
  if (int rc = grow(s, s->probe_buf, s->probe_bytes, bytes, Idle::AfterScene, "hipMallocFromPoolAsync probe"))
    return rc;
  DLaunch Q = L;
  Q.sample_count = std::min(L.sample_count, s->tune.probe_strata > 0 ? s->tune.probe_strata : kProbeStrata);
  Q.output = RT_OUT_SUM;
  Q.accumulate = 0;
  Q.compact = 1;
  apply_plan(Q, whole_plan(L.n_local_tiles), nullptr, 0);
  Q.unit_ctr = nullptr;
  Q.grid_cap = 0;
  Q.tile_order = nullptr;
  Q.tile_cost = os->tile_cost;
  hipError_t e = hipMemsetAsync(os->tile_cost, 0, (size_t)L.n_local_tiles * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(s->stats, 0, RT_N_STATS * sizeof(unsigned long long), st);
  if (e == hipSuccess) e = rtk_launch_render(&s->ds, &C, &Q, s->probe_buf, s->stats, st);
  if (e == hipSuccess)
    e = rtk_launch_tile_order(os->tile_cost, L.n_local_tiles, std::min(L.n_head, L.n_local_tiles),
                              os->tile_order[os->cur], st);
  if (e != hipSuccess) return hip_err(e, "tile order probe");
  os->ready = true;
  return RT_OK;
}

// forced: the split plan of a tile-layout launch whose whole tiles go to
// dev_out (compact) and split tiles' raw partials to the scene's scratch
// (rt_multi_render's shards, reproducing the one-device frame's units).
// *launched: the launch as the render kernel got it -- its plan, its partials
// and the dispatch order it used (null: plan order), what a finish kernel run
// after it must read.
// list: a tile-list launch (rt_render_tiles_device) -- the plan's k-th tile is
// list[k] (the scene's clamped copy of the caller's list), which takes the
// place of a dispatch order: no probe, no order slot.
static int launch(rt_scene *s, const DCamera &C, const DLaunch &L, double *dev_out,
                  unsigned long long *stats, hipStream_t st, const UnitPlan *forced = nullptr,
                  DLaunch *launched = nullptr, const int32_t *list = nullptr) {
  const UnitPlan sp = forced ? *forced
                      : stats ? whole_plan(L.n_local_tiles)
                              : frame_plan(plan_device(s), s->tune, L);
  // forced plans and frame launches take sp (a frame launch's chunk partials
  // go through the scratch: split); any other tile-layout launch keeps
  // launch_geometry's plan, its chunk partials being the caller's output
  DLaunch Lp = L;
  if (forced || !L.compact) apply_plan(Lp, sp, nullptr, 0);
  const bool split = !L.compact && plan_parts(Lp) > 0;
  if (split || forced) {
    const size_t bytes = std::max<size_t>(1, (size_t)plan_parts(Lp) * 64 * 3) * sizeof(double);
    if (int rc = grow(s, s->scratch, s->scratch_bytes, bytes, Idle::AfterScene, "hipMallocFromPoolAsync scratch"))
      return rc;
    apply_plan(Lp, sp, s->scratch, 0);
  } else if (L.parts_final) {
    apply_plan(Lp, plan_of(L), dev_out, 1); // tile layout, strata_chunks > 1
  }
  // persistent waves pulling work units (rt_tuning.no_persistent: one unit
  // per wave, for A/B runs)
  const bool persistent = !s->tune.no_persistent;
  if (persistent && s->wave_slots > 0) {
    Lp.unit_ctr = s->unit_ctr;
    Lp.grid_cap = s->pc_grid > 0 ? s->pc_grid // resident persistent blocks
                                 : std::max(1, s->wave_slots / std::max(1, s->ds.pc_waves));
    // rt_tuning.grid_cap: fewer resident blocks (tests: many units per wave)
    if (s->tune.grid_cap > 0) Lp.grid_cap = s->tune.grid_cap;
  }
  // cost-ordered dispatch: frame launches and forced / library plans, not the
  // STATS instance nor a caller's explicit chunk layout (its partials are the
  // output, by plan tile).  Progressive frames too (one stratum per pixel:
  // C4 0.90 -> 0.81 ms per frame, C2 0.222 -> 0.212, r06aa_ab_progressive.log),
  // now that the costs are measured once per shape, not by every launch.
  const bool ordered = !s->tune.no_tile_order && stats == nullptr && (forced || !L.parts_final) &&
                       L.n_local_tiles > 1 && list == nullptr;
  const int32_t sig[10] = {L.n_local_tiles, L.tile_first, L.tile_stride, L.tiles_x, L.row_begin,
                           L.row_end,       L.sample_count, sp.n_head,   sp.head_chunks, sp.n_chunks};
  // after the scene's previous launch, whichever stream it ran on
  if (int rc = order_after_last(s, st)) return rc;
  rt_scene::OrderSlot *os = nullptr;
  // The first tile-subset launch of a shape (a multi-GPU rank's share) in the
  // flat world runs in plan order in the COST instance (rt_kernel.hip), which
  // measures its own units, and the sort after it gives the order every later
  // launch of the shape takes in the plain instance: an 8-way C2 share 0.81 ms
  // against 0.85 with the probe's order or with costs re-measured after every
  // launch (r06ag: an order measured under cost order itself ranks worse).
  // Every other shape takes its probe's order.
  // (Frame launches ordered this way measured the same as with the probe:
  // r06ah_first_measure_frames_ab_C2.log.)
  bool kernel_costs = ordered && forced != nullptr && rtk_cost_f(s->ds.features);
  if (ordered) {
    int rc = order_slot(s, sig, L.n_local_tiles, os);
    if (rc) return rc;
    if (os->ready) kernel_costs = false;
    if (!kernel_costs && !os->ready && (rc = tile_order_probe(s, C, Lp, os, st))) return rc;
    Lp.tile_order = os->ready ? os->tile_order[os->cur] : nullptr;
  } else {
    Lp.tile_order = list;
  }
  Lp.tile_cost = nullptr;
  if (kernel_costs) {
    hipError_t me = hipMemsetAsync(os->tile_cost, 0, (size_t)L.n_local_tiles * sizeof(uint32_t), st);
    if (me != hipSuccess) return hip_err(me, "hipMemsetAsync tile cost");
    Lp.tile_cost = os->tile_cost;
  }
  hipError_t e = hipEventRecord(s->ev0, st);
  if (e != hipSuccess) return hip_err(e, "hipEventRecord");
  e = rtk_launch_render(&s->ds, &C, &Lp, dev_out, stats, st);
  if (e == hipSuccess && split) e = rtk_launch_split_sum(&C, &Lp, dev_out, st); // chunk partials into the frame
  if (e != hipSuccess) return hip_err(e, "render kernel launch");
  e = hipEventRecord(s->ev1, st);
  if (e != hipSuccess) return hip_err(e, "hipEventRecord");
  s->timed = true;
  if (launched) *launched = Lp;
  if (kernel_costs) { // the next launch's order, into the buffer this one did not read
    const int next = os->cur ^ 1;
    e = rtk_launch_tile_order(os->tile_cost, L.n_local_tiles, std::min(sp.n_head, L.n_local_tiles),
                              os->tile_order[next], st);
    if (e != hipSuccess) return hip_err(e, "tile order");
    os->cur = next;
    os->ready = true;
  }
  return mark_last(s, st);
}

static int ensure_out(rt_scene *s, size_t bytes) { // only the scene's own stream writes out_buf
  return grow(s, s->out_buf, s->out_bytes, bytes, Idle::AfterStream, "hipMallocFromPoolAsync output");
}

int rt_render(rt_scene *s, const rt_frame *f, const rt_render_params *p, double *host_rgb) {
  if (!s || !host_rgb) return set_err(RT_ERR_INVALID, "null argument");
  DCamera C;
  DLaunch L;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if ((rc = to_launch(f, p, L))) return rc;
  DeviceGuard g(s->device);
  rt_render_params q = *p;
  q.accumulate = 0;
  L.accumulate = 0;
  size_t n = out_doubles(f, L);
  if ((rc = ensure_out(s, n * sizeof(double)))) return rc;
  if ((rc = launch(s, C, L, s->out_buf, nullptr, s->stream))) return rc;
  hipError_t e = hipMemcpyAsync(host_rgb, s->out_buf, n * sizeof(double), hipMemcpyDeviceToHost,
                                s->stream);
  if (e != hipSuccess) return hip_err(e, "hipMemcpyAsync D2H");
  e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return hip_err(e, "render kernel");
  return RT_OK;
}

int rt_render_device(rt_scene *s, const rt_frame *f, const rt_render_params *p, double *dev_rgb,
                     void *hip_stream) {
  if (!s || !dev_rgb || !p) return set_err(RT_ERR_INVALID, "null argument");
  DCamera C;
  DLaunch L;
  const bool auto_units = p->strata_chunks == RT_CHUNKS_AUTO;
  if (auto_units && (p->layout != RT_LAYOUT_TILES || p->output != RT_OUT_SUM || p->accumulate))
    return set_err(RT_ERR_INVALID, "RT_CHUNKS_AUTO returns raw tile sums: RT_LAYOUT_TILES, "
                                   "RT_OUT_SUM, accumulate 0");
  rt_render_params q = *p;
  if (auto_units) q.strata_chunks = 0;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if ((rc = to_launch(f, &q, L))) return rc;
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)hip_stream; // NULL = the HIP null stream (HIP convention)
  if (!auto_units) return launch(s, C, L, dev_rgb, nullptr, st);
  // the subset's own units: whole head tiles straight into dev_rgb, chunk
  // partials into the scratch, added in chunk order into dev_rgb (the
  // rt_multi shards' finish), all on `st`
  const UnitPlan sp = subset_plan(plan_device(s), s->tune, L);
  DLaunch done;
  if ((rc = launch(s, C, L, dev_rgb, nullptr, st, &sp, &done))) return rc;
  hipError_t e = rtk_launch_shard_finish(&done, dev_rgb, st);
  if (e != hipSuccess) return hip_err(e, "tile chunk sum");
  return mark_last(s, st); // the chunk sum reads the scratch: the chain ends after it
}

// ---------------------------------------------------------------- adaptive sampling
// A frame-layout launch over the tiles of a device-resident list: the frame
// launch over n_tiles tiles whose k-th tile is list[k] -- the render kernel's
// and split_sum_kernel's own tile indirection (DLaunch.tile_order), fed with
// the scene's clamped copy of the list instead of a measured dispatch order.
int rt_render_tiles_device(rt_scene *s, const rt_frame *f, const rt_render_params *p,
                           const int32_t *device_tiles, int32_t n_tiles, double *dev_rgb,
                           void *hip_stream) {
  if (!s || !dev_rgb || !p || !f) return set_err(RT_ERR_INVALID, "null argument");
  if (p->tile_first != 0 || (p->tile_stride != 0 && p->tile_stride != 1) || p->layout != RT_LAYOUT_FRAME ||
      p->strata_chunks != 0)
    return set_err(RT_ERR_INVALID, "a tile-list launch takes tile_first 0, tile_stride 0 or 1, "
                                   "RT_LAYOUT_FRAME, strata_chunks 0");
  DCamera C;
  DLaunch L;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if ((rc = to_launch(f, p, L))) return rc;
  const int64_t tiles = (int64_t)L.tiles_x * L.tiles_y;
  if (n_tiles < 0 || n_tiles > tiles) return set_err(RT_ERR_INVALID, "n_tiles outside [0, tiles of the row range]");
  if (n_tiles == 0) return RT_OK; // nothing listed: nothing queued
  if (!device_tiles) return set_err(RT_ERR_INVALID, "null tile list");
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)hip_stream;
  // sized for the whole range: the lists of a frame only shrink
  if ((rc = grow(s, s->list_order, s->list_bytes, (size_t)tiles * sizeof(int32_t), Idle::AfterScene,
                 "hipMallocFromPoolAsync tile list")))
    return rc;
  // the copy overwrites what the scene's previous tile-list launch may still read
  if ((rc = order_after_last(s, st))) return rc;
  hipError_t e = rtk_launch_tile_list_copy(device_tiles, n_tiles, (int)tiles, s->list_order, st);
  if (e != hipSuccess) return hip_err(e, "tile list copy");
  L.n_local_tiles = n_tiles; // tile_first 0, tile_stride 1: the mapped tile is the frame's
  apply_plan(L, whole_plan(n_tiles), nullptr, 0);
  return launch(s, C, L, dev_rgb, nullptr, st, nullptr, nullptr, s->list_order);
}

static int frame_tiles(const rt_frame *f, int64_t &tiles) {
  if (!f || f->image_width < 1 || f->image_height < 1) return set_err(RT_ERR_INVALID, "invalid frame");
  tiles = (int64_t)((f->image_width + 7) / 8) * ((f->image_height + 7) / 8);
  if (tiles > 0x7FFFFFFF) return set_err(RT_ERR_UNSUPPORTED, "too many tiles");
  return RT_OK;
}

int rt_adaptive_update_device(const double *device_delta, int32_t batch_strata, const int32_t *device_tiles,
                              int32_t n_tiles, const rt_frame *f, double *device_acc, double *device_s1,
                              double *device_s2, int32_t *device_tile_strata, void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!device_delta || !device_acc || !device_s1 || !device_s2 || !device_tile_strata)
    return set_err(RT_ERR_INVALID, "null argument");
  if (batch_strata < 1) return set_err(RT_ERR_INVALID, "batch_strata must be >= 1");
  if (n_tiles < 0 || n_tiles > tiles) return set_err(RT_ERR_INVALID, "n_tiles outside [0, tiles of the frame]");
  if (n_tiles == 0) return RT_OK;
  if (!device_tiles) return set_err(RT_ERR_INVALID, "null tile list");
  hipError_t e = rtk_launch_adaptive_update(device_delta, batch_strata, device_tiles, n_tiles, f->image_width,
                                            f->image_height, device_acc, device_s1, device_s2,
                                            device_tile_strata, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "adaptive update launch");
  return RT_OK;
}

int rt_adaptive_select_device(const double *device_s1, const double *device_s2,
                              const int32_t *device_tile_strata, int32_t batch_strata, const rt_frame *f,
                              double threshold, double floor, int32_t min_batches,
                              const int32_t *device_tiles_in, int32_t n_in, int32_t *device_tiles_out,
                              int32_t *device_count_out, double *device_tile_error, void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!device_s1 || !device_s2 || !device_tile_strata || !device_tiles_out || !device_count_out)
    return set_err(RT_ERR_INVALID, "null argument");
  if (batch_strata < 1) return set_err(RT_ERR_INVALID, "batch_strata must be >= 1");
  if (n_in < 0 || n_in > tiles) return set_err(RT_ERR_INVALID, "n_in outside [0, tiles of the frame]");
  if (n_in > 0 && !device_tiles_in) return set_err(RT_ERR_INVALID, "null tile list");
  if (device_tiles_in == device_tiles_out) return set_err(RT_ERR_INVALID, "tiles_out must not alias tiles_in");
  hipError_t e = rtk_launch_adaptive_select(device_s1, device_s2, device_tile_strata, batch_strata,
                                            f->image_width, f->image_height, threshold, floor, min_batches,
                                            device_tiles_in, n_in, device_tiles_out, device_count_out,
                                            device_tile_error, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "adaptive select launch");
  return RT_OK;
}

int rt_guided_select_device(const rt_frame *f, const void *device_history, const double *device_variance,
                            const int32_t *device_tile_strata, int32_t strata_now, double threshold, double floor,
                            double min_count, const int32_t *device_tiles_in, int32_t n_in,
                            int32_t *device_tiles_out, int32_t *device_count_out, double *device_tile_error,
                            double *device_tile_count, void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!device_history || !device_variance || !device_tiles_out || !device_count_out)
    return set_err(RT_ERR_INVALID, "null argument");
  if (n_in < 0 || n_in > tiles) return set_err(RT_ERR_INVALID, "n_in outside [0, tiles of the frame]");
  if (n_in > 0 && !device_tiles_in) return set_err(RT_ERR_INVALID, "null tile list");
  if (((uintptr_t)device_history & 255) != 0) return set_err(RT_ERR_INVALID, "a history must be 256-B aligned");
  if (device_tiles_in == device_tiles_out) return set_err(RT_ERR_INVALID, "tiles_out must not alias tiles_in");
  if (threshold != threshold || floor != floor || min_count != min_count)
    return set_err(RT_ERR_INVALID, "a guided-selection parameter is NaN");
  if (!(floor > 0.0)) return set_err(RT_ERR_INVALID, "floor must be > 0");
  if (strata_now < 0) return set_err(RT_ERR_INVALID, "strata_now must be >= 0");
  hipError_t e = rtk_launch_guided_select(device_history, device_variance, device_tile_strata, strata_now,
                                          f->image_width, f->image_height, threshold, floor, min_count,
                                          device_tiles_in, n_in, device_tiles_out, device_count_out,
                                          device_tile_error, device_tile_count, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "guided select launch");
  return RT_OK;
}

int rt_to_bytes_tiles_device(const double *device_rgb, const int32_t *device_tile_strata, const rt_frame *f,
                             uint8_t *device_bytes, void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!device_rgb || !device_tile_strata || !device_bytes) return set_err(RT_ERR_INVALID, "null argument");
  hipError_t e = rtk_launch_to_bytes_tiles(device_rgb, device_tile_strata, f->image_width, f->image_height,
                                           device_bytes, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "to_bytes_tiles launch");
  return RT_OK;
}

// ---------------------------------------------------------------- denoised display
// The guide launch: launch_geometry's row / stratum / seed fields, one
// wavefront per tile of the row range, nothing of the render's plan (no
// units, no order slot, no scratch).  It joins the scene's chain only so that
// destroy waits for it: the kernel reads the scene tables.
int rt_render_guides_device(rt_scene *s, const rt_frame *f, const rt_render_params *p, double *dev_guides,
                            void *hip_stream) {
  if (!s || !dev_guides || !p || !f) return set_err(RT_ERR_INVALID, "null argument");
  if (p->output != RT_OUT_SUM) return set_err(RT_ERR_INVALID, "guides are raw sums: output must be RT_OUT_SUM");
  if (p->tile_first != 0 || (p->tile_stride != 0 && p->tile_stride != 1) || p->layout != RT_LAYOUT_FRAME ||
      p->strata_chunks != 0)
    return set_err(RT_ERR_INVALID, "a guide launch takes tile_first 0, tile_stride 0 or 1, "
                                   "RT_LAYOUT_FRAME, strata_chunks 0");
  DCamera C;
  DLaunch L;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if ((rc = to_launch(f, p, L))) return rc;
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)hip_stream;
  if ((rc = order_after_last(s, st))) return rc;
  hipError_t e = rtk_launch_guides(&s->ds, &C, &L, dev_guides, st);
  if (e != hipSuccess) return hip_err(e, "guide kernel launch");
  return mark_last(s, st);
}

// ---------------------------------------------------------------- ray queries
// The query family: closest hits, occlusion and radiance differ in their kernel, their
// output element and radiance's parameters; the rest is stated once (templates: outside the C block).
} // extern "C"

namespace {

// The count and the arrays, the scene last: every other refusal needs no scene.
int query_check(const rt_scene *s, int64_t n, const void *rays, const void *out, int64_t max_rays,
                const char *too_many, const char *null_array) {
  if (n < 0) return set_err(RT_ERR_INVALID, "negative ray count");
  if (n > max_rays) return set_err(RT_ERR_INVALID, too_many);
  if (n > 0 && (!rays || !out)) return set_err(RT_ERR_INVALID, null_array);
  if (!s) return set_err(RT_ERR_INVALID, "null scene");
  return RT_OK;
}
int trace_check(const rt_scene *s, int64_t n, const void *rays, const void *out) {
  return query_check(s, n, rays, out, (int64_t)1 << 36, "more than 2^36 rays in one call", "null ray or hit array");
}
struct QueryName { // what the errors of a query kind call its kernel and its call
  const char *kernel, *call;
};
constexpr QueryName kTrace{"query", "query"}, kOcclusion{"occlusion", "occlusion query"},
    kRadiance{"radiance", "radiance query"};
std::string text(const char *a, const char *b) { return std::string(a) + b; }
// One launch of a query kernel on `st`: a link of the scene's chain like the
// guide launch -- it reads the tables the edits write, so it runs after
// whatever was queued before it, and destroy waits for it.
template <class Launch>
int query_on_stream(rt_scene *s, hipStream_t st, const QueryName &what, const void *d_rays, void *d_out,
                    Launch launch) {
  DeviceGuard g(s->device);
  int rc = order_after_last(s, st);
  if (rc) return rc;
  hipError_t e = launch((const rt_ray *)d_rays, d_out, st);
  if (e != hipSuccess) return hip_err(e, text(what.kernel, " kernel launch").c_str());
  return mark_last(s, st);
}
// The host variants: n rays up, the launch on the scene's stream, out_bytes of
// results down (and up first when `preload`: radiance's accumulate).  Only
// this function uses trace_buf, on the scene's stream, and it synchronises
// before it returns: the buffer is idle on entry, so it grows without a wait.
template <class Launch>
int query_from_host(rt_scene *s, int64_t n, const rt_ray *rays, void *out, size_t out_bytes, bool preload,
                    const QueryName &what, Launch launch) {
  DeviceGuard g(s->device);
  const size_t ray_bytes = sizeof(rt_ray) * (size_t)n;
  int rc = grow(s, s->trace_buf, s->trace_bytes, align256(ray_bytes) + out_bytes, Idle::Already,
                text("hipMallocFromPoolAsync ", what.call).c_str());
  if (rc) return rc;
  void *d_out = s->trace_buf + align256(ray_bytes);
  hipError_t e = hipMemcpyAsync(s->trace_buf, rays, ray_bytes, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess && preload) e = hipMemcpyAsync(d_out, out, out_bytes, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) {
    rc = query_on_stream(s, s->stream, what, s->trace_buf, d_out, launch);
    if (rc == RT_OK) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s->stream);
  }
  const hipError_t es = hipStreamSynchronize(s->stream);
  if (rc) return rc;
  if (e != hipSuccess) return hip_err(e, text(what.call, " copy").c_str());
  return es == hipSuccess ? RT_OK : hip_err(es, text(what.kernel, " kernel").c_str());
}

// The three launches: (device rays, device results, stream) -> hipError_t.
auto trace_launch(rt_scene *s, int64_t n) {
  return [s, n](const rt_ray *d_rays, void *d_hits, hipStream_t st) {
    return rtk_launch_trace(&s->ds, s->xf_obj, n, d_rays, (rt_ray_hit *)d_hits, st);
  };
}
auto occluded_launch(rt_scene *s, int64_t n) {
  return [s, n](const rt_ray *d_rays, void *d_occ, hipStream_t st) {
    return rtk_launch_occluded(&s->ds, n, d_rays, (uint8_t *)d_occ, st);
  };
}

// The parameters first, then the family's checks with radiance's ray limit.
int radiance_check(const rt_scene *s, int64_t n, const void *rays, const rt_radiance_params *p, const void *rgb) {
  if (!p) return set_err(RT_ERR_INVALID, "null radiance params");
  if (p->_reserved != 0) return set_err(RT_ERR_INVALID, "rt_radiance_params._reserved must be 0");
  if (p->samples < 0) return set_err(RT_ERR_INVALID, "negative sample count");
  if (p->first_sample < 0) return set_err(RT_ERR_INVALID, "negative first_sample");
  if ((int64_t)p->first_sample + p->samples > 0x7fffffffll)
    return set_err(RT_ERR_INVALID, "first_sample + samples overflows int32");
  return query_check(s, n, rays, rgb, (int64_t)1 << 32, "more than 2^32 rays in one call: their keys would repeat",
                     "null ray or rgb array");
}
// nothing to queue: no ray, or nothing to add onto what the buffer holds
bool radiance_empty(int64_t n, const rt_radiance_params *p) {
  return n == 0 || (p->samples == 0 && p->accumulate);
}
auto radiance_launch(rt_scene *s, int64_t n, const rt_radiance_params *p) {
  return [s, n, p, C = rtr::radiance_camera(*p)](const rt_ray *d_rays, void *d_rgb, hipStream_t st) {
    return rtk_launch_radiance(&s->ds, &C, p, n, d_rays, (double *)d_rgb, st);
  };
}

} // namespace

extern "C" {

int rt_trace_device(rt_scene *s, int64_t n, const rt_ray *device_rays, rt_ray_hit *device_hits, void *hip_stream) {
  int rc = trace_check(s, n, device_rays, device_hits);
  if (rc || n == 0) return rc;
  return query_on_stream(s, (hipStream_t)hip_stream, kTrace, device_rays, device_hits, trace_launch(s, n));
}

int rt_trace(rt_scene *s, int64_t n, const rt_ray *rays, rt_ray_hit *hits) {
  int rc = trace_check(s, n, rays, hits);
  if (rc || n == 0) return rc;
  return query_from_host(s, n, rays, hits, sizeof(rt_ray_hit) * (size_t)n, false, kTrace, trace_launch(s, n));
}

int rt_pixel_ray(const rt_frame *f, double x, double y, rt_ray *ray) {
  if (!f || !ray) return set_err(RT_ERR_INVALID, "null argument");
  const double c[3] = {f->center.x, f->center.y, f->center.z};
  const double p00[3] = {f->pixel00_loc.x, f->pixel00_loc.y, f->pixel00_loc.z};
  const double du[3] = {f->pixel_delta_u.x, f->pixel_delta_u.y, f->pixel_delta_u.z};
  const double dv[3] = {f->pixel_delta_v.x, f->pixel_delta_v.y, f->pixel_delta_v.z};
  for (int a = 0; a < 3; ++a) { // rt_temporal.h centre_point's ray, at any (x, y)
    ray->origin[a] = c[a];
    ray->direction[a] = p00[a] + x * du[a] + y * dv[a] - c[a];
  }
  ray->time = 0.0;
  ray->t_max = HUGE_VAL;
  return RT_OK;
}

// ---------------------------------------------------------- occlusion queries
int rt_occluded_device(rt_scene *s, int64_t n, const rt_ray *device_rays, uint8_t *device_occluded,
                       void *hip_stream) {
  int rc = trace_check(s, n, device_rays, device_occluded);
  if (rc || n == 0) return rc;
  return query_on_stream(s, (hipStream_t)hip_stream, kOcclusion, device_rays, device_occluded,
                         occluded_launch(s, n));
}

int rt_occluded(rt_scene *s, int64_t n, const rt_ray *rays, uint8_t *occluded) {
  int rc = trace_check(s, n, rays, occluded);
  if (rc || n == 0) return rc;
  return query_from_host(s, n, rays, occluded, (size_t)n, false, kOcclusion, occluded_launch(s, n));
}

int rt_segment_ray(const double a[3], const double b[3], double time, rt_ray *ray) {
  if (!a || !b || !ray) return set_err(RT_ERR_INVALID, "null argument");
  for (int k = 0; k < 3; ++k) {
    ray->origin[k] = a[k];
    ray->direction[k] = b[k] - a[k];
  }
  ray->time = time;
  ray->t_max = 0.999; // the search starts at 0.001: both ends' own surfaces are skipped alike
  return RT_OK;
}

// ----------------------------------------------------------- radiance queries
int rt_radiance_device(rt_scene *s, int64_t n, const rt_ray *device_rays, const rt_radiance_params *p,
                       double *device_rgb, void *hip_stream) {
  int rc = radiance_check(s, n, device_rays, p, device_rgb);
  if (rc || radiance_empty(n, p)) return rc;
  return query_on_stream(s, (hipStream_t)hip_stream, kRadiance, device_rays, device_rgb, radiance_launch(s, n, p));
}

int rt_radiance(rt_scene *s, int64_t n, const rt_ray *rays, const rt_radiance_params *p, double *rgb) {
  int rc = radiance_check(s, n, rays, p, rgb);
  if (rc || radiance_empty(n, p)) return rc;
  return query_from_host(s, n, rays, rgb, 3 * sizeof(double) * (size_t)n, p->accumulate != 0, kRadiance,
                         radiance_launch(s, n, p));
}

int rt_camera_rays(const rt_frame *f, uint64_t seed, int32_t stratum, int32_t row_begin, int32_t row_end,
                   rt_ray *rays) {
  if (!rays) return set_err(RT_ERR_INVALID, "null ray array");
  DCamera C;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if (row_begin == 0 && row_end == 0) row_end = C.H; // rt_render_params' whole frame
  if (row_begin < 0 || row_end > C.H || row_end <= row_begin)
    return set_err(RT_ERR_INVALID, "row range outside the image");
  if (stratum < 0 || stratum >= (int64_t)C.sqrt_spp * C.sqrt_spp)
    return set_err(RT_ERR_INVALID, "stratum outside [0, sqrt_spp^2)");
  if ((int64_t)C.W * C.H > 0xFFFFFFFFll) return set_err(RT_ERR_UNSUPPORTED, "image too large for 32-bit pixel keys");
  rtk_camera_rays_host(&C, seed, stratum, row_begin, row_end, rays);
  return RT_OK;
}

// a byte range of device memory; a null pointer spans nothing
struct Span {
  uintptr_t begin, end;
  Span(const void *p, size_t bytes) : begin((uintptr_t)p), end(p ? begin + bytes : 0) {}
};
static bool overlaps(Span a, Span b) { return a.begin < b.end && b.begin < a.end; }

// the four *_bytes entry points: `size` of the frame's width and height
static int frame_bytes(const rt_frame *f, int64_t *bytes, size_t (*size)(int, int)) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!bytes) return set_err(RT_ERR_INVALID, "null argument");
  *bytes = (int64_t)size(f->image_width, f->image_height);
  return RT_OK;
}

int rt_denoise_workspace_bytes(const rt_frame *f, int64_t *bytes) {
  return frame_bytes(f, bytes, rtk_denoise_workspace_bytes);
}
int rt_denoise_variance_workspace_bytes(const rt_frame *f, int64_t *bytes) {
  return frame_bytes(f, bytes, rtk_denoise_variance_workspace_bytes);
}

// the launch's fields that every filter entry point takes as arguments; W, H: filter_check
static FilterLaunch filter_fields(int kind, const double *device_rgb, double rgb_scale,
                                  const int32_t *device_tile_strata, const double *device_guides,
                                  int32_t guide_strata, void *device_workspace, double *device_out,
                                  double *device_variance_out) {
  FilterLaunch a{};
  a.kind = kind;
  a.rgb = device_rgb;
  a.scale = rgb_scale;
  a.tile_strata = device_tile_strata;
  a.guides = device_guides;
  a.guide_strata = guide_strata;
  a.workspace = device_workspace;
  a.out = device_out;
  a.var_out = device_variance_out;
  return a;
}

// what the filter entry points refuse, in one order: frame, nulls, guide_strata, RTK_FILTER_VARIANCE's
// moments, workspace alignment, overlaps (a pointer a kind does not take is null and spans nothing)
static int filter_check(const rt_frame *f, FilterLaunch &a) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!a.rgb || !a.guides || !a.workspace || !a.out || (a.kind == RTK_FILTER_GIVEN && !a.variance))
    return set_err(RT_ERR_INVALID, "null argument");
  if (a.guide_strata < 1) return set_err(RT_ERR_INVALID, "guide_strata must be >= 1");
  if ((a.s1 == nullptr) != (a.s2 == nullptr))
    return set_err(RT_ERR_INVALID, "device_s1 and device_s2 go together: both or neither");
  if (a.s1 && !a.tile_strata) return set_err(RT_ERR_INVALID, "moments need device_tile_strata");
  if (a.s1 && a.batch_strata < 1) return set_err(RT_ERR_INVALID, "moments need batch_strata >= 1");
  if (((uintptr_t)a.workspace & 255) != 0) return set_err(RT_ERR_INVALID, "workspace must be 256-B aligned");
  a.W = f->image_width;
  a.H = f->image_height;
  const size_t px = (size_t)a.W * a.H;
  const Span ws(a.workspace, a.kind == RTK_FILTER_PLAIN ? rtk_denoise_workspace_bytes(a.W, a.H)
                                                        : rtk_denoise_variance_workspace_bytes(a.W, a.H));
  const Span out(a.out, px * 3 * sizeof(double)), vout(a.var_out, px * sizeof(double));
  const Span vin(a.variance, px * sizeof(double));
  if (overlaps(out, ws)) return set_err(RT_ERR_INVALID, "device_out overlaps the workspace");
  if (overlaps(vout, ws)) return set_err(RT_ERR_INVALID, "device_variance_out overlaps the workspace");
  if (overlaps(vout, out)) return set_err(RT_ERR_INVALID, "device_variance_out overlaps device_out");
  if (overlaps(vin, ws)) return set_err(RT_ERR_INVALID, "device_variance overlaps the workspace");
  if (overlaps(vin, out)) return set_err(RT_ERR_INVALID, "device_variance overlaps device_out");
  if (overlaps(vin, vout)) return set_err(RT_ERR_INVALID, "device_variance overlaps device_variance_out");
  return RT_OK;
}

// rt_denoise_params / rt_denoise_variance_params resolved into the launch: 0 = the default,
// a sigma < 0 stays (off); sigma_c: the colour sigma or sigma_lum, dflt_c its default
static int filter_params(int passes, int min_batches, double sigma_n, double sigma_z, double sigma_h,
                         double sigma_c, double dflt_c, FilterLaunch &a) {
  if (passes > RT_DENOISE_MAX_PASSES)
    return set_err(RT_ERR_INVALID, "passes must be at most " + std::to_string(RT_DENOISE_MAX_PASSES));
  const double sig[4] = {sigma_n, sigma_z, sigma_h, sigma_c};
  for (double v : sig)
    if (v != v) return set_err(RT_ERR_INVALID, "a sigma is NaN");
  auto pick = [](double v, double dflt) { return v == 0.0 ? dflt : v; }; // < 0: off
  a.passes = passes == 0 ? RT_DENOISE_PASSES : passes;
  a.min_batches = std::max(2, min_batches == 0 ? RT_DENOISE_MIN_BATCHES : min_batches);
  a.sigma_n = pick(sigma_n, RT_DENOISE_SIGMA_NORMAL);
  a.sigma_z = pick(sigma_z, RT_DENOISE_SIGMA_DEPTH);
  a.sigma_h = pick(sigma_h, RT_DENOISE_SIGMA_HIT);
  a.sigma_c = pick(sigma_c, dflt_c);
  return RT_OK;
}
static int filter_params(const rt_denoise_params *params, FilterLaunch &a) {
  rt_denoise_params q{};
  if (params) q = *params;
  return filter_params(q.passes, 0, q.sigma_normal, q.sigma_depth, q.sigma_hit, q.sigma_color,
                       RT_DENOISE_SIGMA_COLOR, a);
}
static int filter_params(const rt_denoise_variance_params *params, FilterLaunch &a) {
  rt_denoise_variance_params q{};
  if (params) q = *params;
  return filter_params(q.passes, q.min_batches, q.sigma_normal, q.sigma_depth, q.sigma_hit, q.sigma_lum,
                       RT_DENOISE_SIGMA_LUM, a);
}

static int filter_launch(const FilterLaunch &a, void *hip_stream, const char *what) {
  hipError_t e = rtk_launch_filter(&a, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, what);
  return RT_OK;
}

int rt_denoise_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                      const int32_t *device_tile_strata, const double *device_guides, int32_t guide_strata,
                      const rt_denoise_params *params, void *device_workspace, double *device_out,
                      void *hip_stream) {
  FilterLaunch a = filter_fields(RTK_FILTER_PLAIN, device_rgb, rgb_scale, device_tile_strata, device_guides,
                                 guide_strata, device_workspace, device_out, nullptr);
  if (int rc = filter_check(f, a)) return rc;
  if (int rc = filter_params(params, a)) return rc;
  return filter_launch(a, hip_stream, "denoise launch");
}

int rt_denoise_variance_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                               const int32_t *device_tile_strata, const double *device_guides,
                               int32_t guide_strata, const double *device_s1, const double *device_s2,
                               int32_t batch_strata, const rt_denoise_variance_params *params,
                               void *device_workspace, double *device_out, double *device_variance_out,
                               void *hip_stream) {
  FilterLaunch a = filter_fields(RTK_FILTER_VARIANCE, device_rgb, rgb_scale, device_tile_strata, device_guides,
                                 guide_strata, device_workspace, device_out, device_variance_out);
  a.s1 = device_s1;
  a.s2 = device_s2;
  a.batch_strata = batch_strata;
  if (int rc = filter_check(f, a)) return rc;
  if (int rc = filter_params(params, a)) return rc;
  return filter_launch(a, hip_stream, "variance-guided denoise launch");
}

int rt_denoise_given_variance_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                                     const int32_t *device_tile_strata, const double *device_guides,
                                     int32_t guide_strata, const double *device_variance,
                                     const rt_denoise_variance_params *params, void *device_workspace,
                                     double *device_out, double *device_variance_out, void *hip_stream) {
  FilterLaunch a = filter_fields(RTK_FILTER_GIVEN, device_rgb, rgb_scale, device_tile_strata, device_guides,
                                 guide_strata, device_workspace, device_out, device_variance_out);
  a.variance = device_variance;
  if (int rc = filter_check(f, a)) return rc;
  if (int rc = filter_params(params, a)) return rc;
  return filter_launch(a, hip_stream, "given-variance denoise launch");
}

// ---------------------------------------------------------------- temporal reprojection
int rt_history_bytes(const rt_frame *f, int64_t *bytes) { return frame_bytes(f, bytes, rtk_history_bytes); }

// what rt_temporal_device and rt_temporal_variance_device refuse alike; hb: the bytes of one history
static int temporal_args(const rt_frame *f, const double *device_rgb, const int32_t *device_tile_strata,
                         int32_t strata_now, const double *device_guides, int32_t guide_strata,
                         const rt_frame *frame_prev, const void *device_history_prev,
                         const rt_temporal_params *params, void *device_history_out, double *device_out, size_t hb,
                         rt_temporal_params &q) {
  if (!device_rgb || !device_guides || !device_history_out || !device_out)
    return set_err(RT_ERR_INVALID, "null argument");
  if (guide_strata < 1) return set_err(RT_ERR_INVALID, "guide_strata must be >= 1");
  if (!device_tile_strata && strata_now < 0) return set_err(RT_ERR_INVALID, "strata_now must be >= 0");
  if ((frame_prev == nullptr) != (device_history_prev == nullptr))
    return set_err(RT_ERR_INVALID, "frame_prev and device_history_prev go together: both or neither");
  if (frame_prev && (frame_prev->image_width != f->image_width || frame_prev->image_height != f->image_height))
    return set_err(RT_ERR_INVALID, "frame_prev has another size than frame_now");
  if (((uintptr_t)device_history_out & 255) != 0 || ((uintptr_t)device_history_prev & 255) != 0)
    return set_err(RT_ERR_INVALID, "a history must be 256-B aligned");
  const Span hout(device_history_out, hb), hprev(device_history_prev, hb);
  const Span out(device_out, (size_t)f->image_width * f->image_height * 3 * sizeof(double));
  if (overlaps(hout, hprev)) return set_err(RT_ERR_INVALID, "device_history_out overlaps device_history_prev");
  if (overlaps(out, hout) || overlaps(out, hprev)) return set_err(RT_ERR_INVALID, "device_out overlaps a history");
  q = rt_temporal_params{};
  if (params) q = *params;
  if (q.max_history < 0) return set_err(RT_ERR_INVALID, "max_history must be >= 0");
  const double par[3] = {q.sigma_depth, q.sigma_normal, q.hit_min};
  for (double v : par)
    if (v != v) return set_err(RT_ERR_INVALID, "a temporal parameter is NaN");
  return RT_OK;
}

int rt_temporal_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                       const int32_t *device_tile_strata, int32_t strata_now, const double *device_guides,
                       int32_t guide_strata, const rt_frame *frame_prev, const void *device_history_prev,
                       const rt_temporal_params *params, void *device_history_out, double *device_out,
                       void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  rt_temporal_params q{};
  if (int rc = temporal_args(f, device_rgb, device_tile_strata, strata_now, device_guides, guide_strata, frame_prev,
                             device_history_prev, params, device_history_out, device_out,
                             rtk_history_bytes(f->image_width, f->image_height), q))
    return rc;
  hipError_t e = rtk_launch_temporal(f, device_rgb, rgb_scale, device_tile_strata, strata_now, device_guides,
                                     guide_strata, frame_prev, device_history_prev, &q, device_history_out,
                                     device_out, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "temporal launch");
  return RT_OK;
}

// ---------------------------------------------------------------- temporal variance
int rt_history_variance_bytes(const rt_frame *f, int64_t *bytes) {
  return frame_bytes(f, bytes, rtk_history_variance_bytes);
}

int rt_temporal_variance_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                                const int32_t *device_tile_strata, int32_t strata_now, const double *device_guides,
                                int32_t guide_strata, const rt_frame *frame_prev, const void *device_history_prev,
                                const double *device_variance_now, const rt_temporal_params *params,
                                void *device_history_out, double *device_out, double *device_variance_out,
                                void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!device_variance_now || !device_variance_out) return set_err(RT_ERR_INVALID, "null argument");
  const size_t hb = rtk_history_variance_bytes(f->image_width, f->image_height);
  rt_temporal_params q{};
  if (int rc = temporal_args(f, device_rgb, device_tile_strata, strata_now, device_guides, guide_strata, frame_prev,
                             device_history_prev, params, device_history_out, device_out, hb, q))
    return rc;
  const size_t px = (size_t)f->image_width * f->image_height;
  const Span vout(device_variance_out, px * sizeof(double));
  if (overlaps(vout, Span(device_history_out, hb)) || overlaps(vout, Span(device_history_prev, hb)))
    return set_err(RT_ERR_INVALID, "device_variance_out overlaps a history");
  if (overlaps(vout, Span(device_variance_now, px * sizeof(double))))
    return set_err(RT_ERR_INVALID, "device_variance_out overlaps device_variance_now");
  if (overlaps(vout, Span(device_out, px * 3 * sizeof(double))))
    return set_err(RT_ERR_INVALID, "device_variance_out overlaps device_out");
  hipError_t e = rtk_launch_temporal_variance(f, device_rgb, rgb_scale, device_tile_strata, strata_now,
                                              device_guides, guide_strata, frame_prev, device_history_prev,
                                              device_variance_now, &q, device_history_out, device_out,
                                              device_variance_out, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "temporal variance launch");
  return RT_OK;
}

// ---------------------------------------------------------------- object motion vectors
static rt_live::PoseCounts pose_counts(const rt_scene *s) {
  return rt_live::PoseCounts{s->n_xforms, s->n_spheres, s->n_quads, 0};
}

int rt_scene_pose_bytes(const rt_scene *s, int64_t *bytes) {
  if (!s || !bytes) return set_err(RT_ERR_INVALID, "null argument");
  *bytes = rt_live::pose_bytes(pose_counts(s));
  return RT_OK;
}

// One pack kernel on `st`: it reads the tables the edits write, so it is a link of the chain.
int rt_scene_pose_device(rt_scene *s, void *device_pose, void *hip_stream) {
  if (!s) return set_err(RT_ERR_INVALID, "null scene");
  if (!device_pose) return set_err(RT_ERR_INVALID, "null device_pose");
  if (((uintptr_t)device_pose & 255) != 0) return set_err(RT_ERR_INVALID, "a pose must be 256-B aligned");
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = order_after_last(s, st);
  if (rc) return rc;
  const rt_live::PoseCounts c = pose_counts(s);
  const DScene &d = s->ds;
  hipError_t e = rtk_pose(&c, d.xforms, d.spheres, d.quads, (double *)device_pose, st);
  rc = mark_last(s, st);
  if (e != hipSuccess) return hip_err(e, "pose kernel launch");
  return rc;
}

int rt_motion_device(rt_scene *s, const rt_frame *f, const void *device_pose_prev, rt_motion *device_motion,
                     void *hip_stream) {
  if (!s || !f || !device_pose_prev || !device_motion) return set_err(RT_ERR_INVALID, "null argument");
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (((uintptr_t)device_pose_prev & 255) != 0) return set_err(RT_ERR_INVALID, "a pose must be 256-B aligned");
  if (((uintptr_t)device_motion & 7) != 0) return set_err(RT_ERR_INVALID, "device_motion must be 8-B aligned");
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = order_after_last(s, st);
  if (rc) return rc;
  const rt_live::PoseCounts c = pose_counts(s);
  hipError_t e = rtk_launch_motion(&s->ds, s->xf_obj, f, &c, (const double *)device_pose_prev, device_motion, st);
  if (e != hipSuccess) return hip_err(e, "motion kernel launch");
  return mark_last(s, st);
}

// what the _motion forms refuse beyond their parents: a null plane, or one an output overlaps
static int motion_args(const rt_frame *f, const rt_motion *device_motion, const void *device_history_out, size_t hb,
                       const double *device_out, const double *device_variance_out) {
  if (!device_motion) return set_err(RT_ERR_INVALID, "null device_motion");
  const size_t px = (size_t)f->image_width * f->image_height;
  const Span m(device_motion, px * sizeof(rt_motion));
  if (overlaps(m, Span(device_history_out, hb))) return set_err(RT_ERR_INVALID, "device_motion overlaps device_history_out");
  if (overlaps(m, Span(device_out, px * 3 * sizeof(double)))) return set_err(RT_ERR_INVALID, "device_motion overlaps device_out");
  if (device_variance_out && overlaps(m, Span(device_variance_out, px * sizeof(double))))
    return set_err(RT_ERR_INVALID, "device_motion overlaps device_variance_out");
  return RT_OK;
}

int rt_temporal_motion_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                              const int32_t *device_tile_strata, int32_t strata_now, const double *device_guides,
                              int32_t guide_strata, const rt_frame *frame_prev, const void *device_history_prev,
                              const rt_motion *device_motion, const rt_temporal_params *params,
                              void *device_history_out, double *device_out, void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  const size_t hb = rtk_history_bytes(f->image_width, f->image_height);
  rt_temporal_params q{};
  if (int rc = temporal_args(f, device_rgb, device_tile_strata, strata_now, device_guides, guide_strata, frame_prev,
                             device_history_prev, params, device_history_out, device_out, hb, q))
    return rc;
  if (int rc = motion_args(f, device_motion, device_history_out, hb, device_out, nullptr)) return rc;
  hipError_t e = rtk_launch_temporal_motion(f, device_rgb, rgb_scale, device_tile_strata, strata_now, device_guides,
                                            guide_strata, frame_prev, device_history_prev, device_motion, &q,
                                            device_history_out, device_out, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "temporal motion launch");
  return RT_OK;
}

int rt_temporal_variance_motion_device(const rt_frame *f, const double *device_rgb, double rgb_scale,
                                       const int32_t *device_tile_strata, int32_t strata_now,
                                       const double *device_guides, int32_t guide_strata, const rt_frame *frame_prev,
                                       const void *device_history_prev, const rt_motion *device_motion,
                                       const double *device_variance_now, const rt_temporal_params *params,
                                       void *device_history_out, double *device_out, double *device_variance_out,
                                       void *hip_stream) {
  int64_t tiles = 0;
  if (int rc = frame_tiles(f, tiles)) return rc;
  if (!device_variance_now || !device_variance_out) return set_err(RT_ERR_INVALID, "null argument");
  const size_t hb = rtk_history_variance_bytes(f->image_width, f->image_height);
  rt_temporal_params q{};
  if (int rc = temporal_args(f, device_rgb, device_tile_strata, strata_now, device_guides, guide_strata, frame_prev,
                             device_history_prev, params, device_history_out, device_out, hb, q))
    return rc;
  const size_t px = (size_t)f->image_width * f->image_height;
  const Span vout(device_variance_out, px * sizeof(double));
  if (overlaps(vout, Span(device_history_out, hb)) || overlaps(vout, Span(device_history_prev, hb)))
    return set_err(RT_ERR_INVALID, "device_variance_out overlaps a history");
  if (overlaps(vout, Span(device_variance_now, px * sizeof(double))))
    return set_err(RT_ERR_INVALID, "device_variance_out overlaps device_variance_now");
  if (overlaps(vout, Span(device_out, px * 3 * sizeof(double))))
    return set_err(RT_ERR_INVALID, "device_variance_out overlaps device_out");
  if (int rc = motion_args(f, device_motion, device_history_out, hb, device_out, device_variance_out)) return rc;
  hipError_t e = rtk_launch_temporal_variance_motion(f, device_rgb, rgb_scale, device_tile_strata, strata_now,
                                                     device_guides, guide_strata, frame_prev, device_history_prev,
                                                     device_motion, device_variance_now, &q, device_history_out,
                                                     device_out, device_variance_out, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "temporal variance motion launch");
  return RT_OK;
}

int rt_render_stats(rt_scene *s, const rt_frame *f, const rt_render_params *p,
                    rt_path_stats *stats) {
  if (!s || !stats || !p) return set_err(RT_ERR_INVALID, "null argument");
  DCamera C;
  DLaunch L;
  // RT_CHUNKS_AUTO: the counters of the subset plan's own units
  const bool auto_units = p->strata_chunks == RT_CHUNKS_AUTO && p->layout == RT_LAYOUT_TILES;
  rt_render_params q = *p;
  if (auto_units) q.strata_chunks = 0;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if ((rc = to_launch(f, &q, L))) return rc;
  DeviceGuard g(s->device);
  L.accumulate = 0;
  size_t n = out_doubles(f, L);
  if ((rc = ensure_out(s, n * sizeof(double)))) return rc;
  hipError_t e = hipMemsetAsync(s->stats, 0, RT_N_STATS * sizeof(unsigned long long), s->stream);
  if (e != hipSuccess) return hip_err(e, "hipMemsetAsync stats");
  UnitPlan sp{};
  if (auto_units) sp = subset_plan(plan_device(s), s->tune, L);
  if ((rc = launch(s, C, L, s->out_buf, s->stats, s->stream, auto_units ? &sp : nullptr))) return rc;
  unsigned long long h[RT_N_STATS];
  e = hipMemcpyAsync(h, s->stats, sizeof h, hipMemcpyDeviceToHost, s->stream);
  if (e != hipSuccess) return hip_err(e, "hipMemcpyAsync stats");
  e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return hip_err(e, "stats kernel");
  stats->samples = h[0];
  stats->segments = h[1];
  stats->node_visits = h[2];
  stats->sphere_tests = h[3];
  stats->quad_tests = h[4];
  stats->other_tests = h[5];
  stats->light_tests = h[6];
  stats->shade_events = h[7];
  stats->wave_trips = h[8];
  stats->wave_node_iters = h[9];
  stats->wave_leaf_iters = h[10];
  stats->wave_shade_iters = h[11];
  stats->cyc_loop = h[12];
  stats->cyc_regen = h[13];
  stats->cyc_trace = h[14];
  stats->cyc_media = h[15];
  stats->cyc_shade = h[16];
  stats->cyc_lights = h[17];
  stats->model_trace_max = h[18];
  stats->model_trace_pair_max = h[19];
  stats->noise_evals = h[20];
  stats->wave_noise_iters = h[21];
  stats->medium_box_tests = h[22];
  stats->medium_box_deferred = h[23];
  return RT_OK;
}

int rt_scene_bvh_cost(const rt_scene *s, double *cost) {
  if (!s || !cost) return set_err(RT_ERR_INVALID, "null argument");
  *cost = 0.0;
  if (s->binary_cost >= 0.0) { // the device holds the 4-wide collapse
    *cost = s->binary_cost;
    return RT_OK;
  }
  const int n = s->ds.n_nodes;
  if (s->ds.root_is_leaf || n <= 0) return RT_OK;
  std::vector<DNode> nodes(n);
  DeviceGuard g(s->device);
  if (s->has_last) (void)hipEventSynchronize(s->last); // a move's refit on a caller stream
  hipError_t e = hipMemcpy(nodes.data(), s->ds.nodes, sizeof(DNode) * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_err(e, "hipMemcpy nodes");
  *cost = rtx::bvh_sah_cost(nodes);
  return RT_OK;
}

// ---------------------------------------------------------------- moving spheres, live transforms and quads
// The state of the scene's first move or edit: one allocation, the
// movable-sphere table and the live index uploaded and the tree's links built
// on `st` (the move's stream; later moves on other streams follow through the
// launch chain).
static int ensure_refit(rt_scene *s, hipStream_t st) {
  if (s->refit) return RT_OK;
  const DScene &d = s->ds;
  const bool tree = !d.root_is_leaf && d.n_nodes > 0;
  const size_t n_obj = s->sphere_of.size();
  size_t bytes = 0;
  auto add = [&](size_t b) {
    const size_t off = bytes;
    bytes += align256(b ? b : 1);
    return off;
  };
  add(sizeof(int32_t) * n_obj); // sphere_of, at 0
  s->refit_named = add(sizeof(unsigned) * n_obj);
  s->refit_boxes = add(tree ? 6 * sizeof(double) * (size_t)s->n_items : 0);
  // room for any tree over these items (a rebuild's may have more nodes than creation's)
  s->refit_temp_bytes = tree ? rtk_refit_temp_bytes(s->n_items, std::max(d.n_nodes, s->n_items - 1)) : 0;
  s->refit_temp = add(s->refit_temp_bytes);
  s->refit_xf_kind = add(sizeof(int32_t) * s->xf_kind.size());
  s->refit_xf_first = add(sizeof(int32_t) * s->xf_first.size());
  s->refit_xf_recs = add(sizeof(int32_t) * s->xf_recs.size());
  s->refit_quad_of = add(sizeof(int32_t) * s->quad_of.size());
  char *buf = nullptr;
  hipError_t e = scene_alloc(s, (void **)&buf, bytes);
  if (e != hipSuccess) return set_err(RT_ERR_OOM, std::string("hipMallocFromPoolAsync refit: ") + hipGetErrorString(e));
  e = hipMemcpyAsync(buf, s->sphere_of.data(), sizeof(int32_t) * n_obj, hipMemcpyHostToDevice, st);
  auto put = [&](size_t off, const std::vector<int32_t> &v) {
    if (e == hipSuccess && !v.empty())
      e = hipMemcpyAsync(buf + off, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice, st);
  };
  put(s->refit_xf_kind, s->xf_kind);
  put(s->refit_xf_first, s->xf_first);
  put(s->refit_xf_recs, s->xf_recs);
  put(s->refit_quad_of, s->quad_of);
  if (e == hipSuccess && tree)
    e = rtk_refit_links(d.nodes, s->bvh_arity, d.n_nodes, buf + s->refit_temp, s->refit_temp_bytes, st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st); // nothing may still use buf
    scene_free(s, buf);
    return hip_err(e, "refit links");
  }
  s->refit = buf;
  return RT_OK;
}

// One update on `st`, a link of the scene's launch chain: the values into the
// tables (sphere centres, transform records or quad corners), then what follows
// from the tables -- every medium's world box, every world item's box and a
// full refit of the tree.  All three kinds of update share the tail.
enum EditKind { EDIT_SPHERES, EDIT_TRANSFORMS, EDIT_QUADS };
static const char *edit_name(EditKind k) {
  return k == EDIT_SPHERES ? "move spheres" : k == EDIT_TRANSFORMS ? "set transforms" : "move quads";
}
static rt_live::LiveIndex device_index(const rt_scene *s) {
  rt_live::LiveIndex L{};
  L.n_objects = (int32_t)s->xf_kind.size();
  L.xf_kind = (const int32_t *)(s->refit + s->refit_xf_kind);
  L.xf_first = (const int32_t *)(s->refit + s->refit_xf_first);
  L.xf_recs = (const int32_t *)(s->refit + s->refit_xf_recs);
  L.quad_of = (const int32_t *)(s->refit + s->refit_quad_of);
  return L;
}
static rt_live::LiveIndex host_index(const rt_scene *s) {
  rt_live::LiveIndex L{};
  L.n_objects = (int32_t)s->xf_kind.size();
  L.xf_kind = s->xf_kind.data();
  L.xf_first = s->xf_first.data();
  L.xf_recs = s->xf_recs.data();
  L.quad_of = s->quad_of.data();
  return L;
}
static int edit_on_stream(rt_scene *s, EditKind kind, int32_t n, const int32_t *d_ids, const double *d_values,
                          hipStream_t st) {
  int rc = order_after_last(s, st);
  if (rc) return rc;
  if ((rc = ensure_refit(s, st))) return rc;
  const DScene &d = s->ds;
  hipError_t e;
  if (kind == EDIT_SPHERES) {
    RefitMove m{};
    m.ids = d_ids;
    m.centres = d_values;
    m.n = n;
    m.n_objects = (int32_t)s->sphere_of.size();
    m.sphere_of = (const int32_t *)s->refit;
    m.named = (unsigned *)(s->refit + s->refit_named);
    m.spheres = const_cast<DSphere *>(d.spheres);
    m.roots = const_cast<DRoot *>(d.roots);
    m.root_items = d.items;
    m.n_roots = d.n_roots;
    e = rtk_move_spheres(&m, st);
  } else {
    LiveEdit le{};
    le.ids = d_ids;
    le.values = d_values;
    le.n = n;
    le.index = device_index(s);
    le.named = (unsigned *)(s->refit + s->refit_named);
    le.xforms = const_cast<DXform *>(d.xforms);
    le.quads = const_cast<DQuad *>(d.quads);
    e = kind == EDIT_TRANSFORMS ? rtk_set_transforms(&le, st) : rtk_move_quads(&le, st);
  }
  if (e == hipSuccess && d.n_mitems > 0) // a flat world has media too
    e = rtk_medium_boxes(d.mitems, d.n_mitems, d.media, d.bitems, d.spheres, d.quads, d.xforms,
                         const_cast<float *>(d.mbox), st);
  if (e == hipSuccess && !d.root_is_leaf && d.n_nodes > 0) {
    double *boxes = (double *)(s->refit + s->refit_boxes);
    e = rtk_item_boxes(d.items, s->n_items, d.spheres, d.quads, d.xforms, boxes, st);
    if (e == hipSuccess)
      e = rtk_refit_boxes(const_cast<DNode *>(d.nodes), s->bvh_arity, d.n_nodes, s->n_items, boxes,
                          s->refit + s->refit_temp, s->refit_temp_bytes, st);
  }
  // whatever was queued reads and writes the scene's tables: the chain ends after it either way
  rc = mark_last(s, st);
  if (e != hipSuccess) return hip_err(e, edit_name(kind));
  return rc;
}

// what the host variant refuses (the device variant skips the same entries)
static int check_move(const rt_scene *s, int32_t n, const int32_t *ids, const double *centres) {
  std::vector<char> seen(s->sphere_of.size(), 0);
  for (int32_t j = 0; j < n; ++j) {
    const int32_t id = ids[j];
    const std::string at = "entry " + std::to_string(j) + ": object " + std::to_string(id);
    if (id < 0 || (size_t)id >= s->sphere_of.size()) return set_err(RT_ERR_INVALID, at + " is out of range");
    if (s->sphere_of[id] == -2)
      return set_err(RT_ERR_UNSUPPORTED, at + " bounds a constant medium: its boundary constants would have to follow");
    if (s->sphere_of[id] < 0)
      return set_err(RT_ERR_INVALID, at + " is not a sphere among the world's primitive items");
    if (seen[id]) return set_err(RT_ERR_INVALID, at + " is named twice");
    seen[id] = 1;
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(centres[3 * (size_t)j + a])) return set_err(RT_ERR_INVALID, at + ": the centre is not finite");
  }
  return RT_OK;
}

static int check_edit(const rt_scene *s, EditKind kind, int32_t n, const int32_t *ids, const double *values) {
  if (kind == EDIT_SPHERES) return check_move(s, n, ids, values);
  std::string err;
  const int rc = kind == EDIT_TRANSFORMS ? rt_live::check_transforms(host_index(s), n, ids, values, err)
                                         : rt_live::check_quads(host_index(s), n, ids, values, s->quad_n.data(), err);
  return rc == RT_OK ? RT_OK : set_err(rc, err);
}

// The host variants: everything validated, the arrays staged, one update on the
// scene's own stream, complete on return.
static int edit_from_host(rt_scene *s, EditKind kind, int32_t n, const int32_t *object_ids, const double *values) {
  if (!s || n < 0) return set_err(RT_ERR_INVALID, "null scene or negative count");
  if (n == 0) return RT_OK;
  if (!object_ids || !values) return set_err(RT_ERR_INVALID, "null argument");
  int rc = check_edit(s, kind, n, object_ids, values);
  if (rc) return rc;
  DeviceGuard g(s->device);
  const size_t id_bytes = align256(sizeof(int32_t) * (size_t)n), c_bytes = 3 * sizeof(double) * (size_t)n;
  // only this function uses move_buf, on the scene's stream, and synchronises before it returns
  if ((rc = grow(s, s->move_buf, s->move_bytes, id_bytes + c_bytes, Idle::Already, "hipMallocFromPoolAsync move")))
    return rc;
  hipError_t e = hipMemcpyAsync(s->move_buf, object_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(s->move_buf + id_bytes, values, c_bytes, hipMemcpyHostToDevice, s->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s->stream);
    return hip_err(e, "move upload");
  }
  rc = edit_on_stream(s, kind, n, (const int32_t *)s->move_buf, (const double *)(s->move_buf + id_bytes), s->stream);
  e = hipStreamSynchronize(s->stream);
  if (rc) return rc;
  return e == hipSuccess ? RT_OK : hip_err(e, edit_name(kind));
}

// The device variants: asynchronous on the caller's stream.
static int edit_from_device(rt_scene *s, EditKind kind, int32_t n, const int32_t *d_ids, const double *d_values,
                            void *hip_stream) {
  if (!s || n < 0) return set_err(RT_ERR_INVALID, "null scene or negative count");
  if (n == 0) return RT_OK;
  if (!d_ids || !d_values) return set_err(RT_ERR_INVALID, "null argument");
  DeviceGuard g(s->device);
  return edit_on_stream(s, kind, n, d_ids, d_values, (hipStream_t)hip_stream);
}

int rt_scene_move_spheres(rt_scene *s, int32_t n, const int32_t *object_ids, const double *centres) {
  return edit_from_host(s, EDIT_SPHERES, n, object_ids, centres);
}
int rt_scene_move_spheres_device(rt_scene *s, int32_t n, const int32_t *device_object_ids,
                                 const double *device_centres, void *hip_stream) {
  return edit_from_device(s, EDIT_SPHERES, n, device_object_ids, device_centres, hip_stream);
}

int rt_scene_set_transforms(rt_scene *s, int32_t n, const int32_t *object_ids, const double *values) {
  return edit_from_host(s, EDIT_TRANSFORMS, n, object_ids, values);
}
int rt_scene_set_transforms_device(rt_scene *s, int32_t n, const int32_t *device_object_ids,
                                   const double *device_values, void *hip_stream) {
  return edit_from_device(s, EDIT_TRANSFORMS, n, device_object_ids, device_values, hip_stream);
}

int rt_scene_move_quads(rt_scene *s, int32_t n, const int32_t *object_ids, const double *corners) {
  return edit_from_host(s, EDIT_QUADS, n, object_ids, corners);
}
int rt_scene_move_quads_device(rt_scene *s, int32_t n, const int32_t *device_object_ids,
                               const double *device_corners, void *hip_stream) {
  return edit_from_device(s, EDIT_QUADS, n, device_object_ids, device_corners, hip_stream);
}

// ---------------------------------------------------------------- rebuilding the world tree
// The state of the scene's first rebuild: one allocation (rt_scene::Rebuild),
// the compile-order items uploaded into it; the host's copy is let go.
static int ensure_rebuild(rt_scene *s) {
  if (s->rebuild) return RT_OK;
  const size_t n = (size_t)s->n_items;
  const bool wide = s->bvh_arity == 4;
  rt_scene::Rebuild R;
  size_t bytes = 0;
  auto add = [&](size_t b) {
    const size_t off = bytes;
    bytes += align256(b ? b : 1);
    return off;
  };
  R.items = add(sizeof(DItem) * n);
  R.boxes = add(6 * sizeof(double) * n);
  R.nodes = add(sizeof(DNode) * (n - 1));
  R.nodes4 = add(wide ? sizeof(DNode4) * (n - 1) : 0);
  R.sorted = add(sizeof(DItem) * n);
  R.temp_bytes = std::max(rtk_sah_temp_bytes((int)n), wide ? rtk_collapse4_temp_bytes((int)n - 1) : (size_t)0);
  R.temp = add(R.temp_bytes);
  char *buf = nullptr;
  hipError_t e = scene_alloc(s, (void **)&buf, bytes);
  if (e != hipSuccess) return set_err(RT_ERR_OOM, std::string("hipMallocFromPoolAsync rebuild: ") + hipGetErrorString(e));
  e = upload(s, buf + R.items, s->compile_items.data(), sizeof(DItem) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    scene_free(s, buf);
    return hip_err(e, "rebuild upload");
  }
  std::vector<DItem>().swap(s->compile_items);
  s->rb = R;
  s->rebuild = buf;
  return RT_OK;
}

int rt_scene_rebuild_bvh(rt_scene *s, int32_t *rebuilt) {
  if (rebuilt) *rebuilt = 0;
  if (!s) return set_err(RT_ERR_INVALID, "null scene");
  DScene &d = s->ds;
  if (d.root_is_leaf || d.n_nodes <= 0 || s->n_items < 2) return RT_OK; // a flat world: nothing to rebuild
  DeviceGuard g(s->device);
  wait_scene(s); // synchronous: the scene's launch chain has ended, on whichever streams it ran
  if (int rc = ensure_rebuild(s)) return rc;
  const int n = s->n_items;
  const bool wide = s->bvh_arity == 4;
  const rt_scene::Rebuild &R = s->rb;
  const DItem *items0 = (const DItem *)(s->rebuild + R.items);
  double *boxes = (double *)(s->rebuild + R.boxes);
  DNode *nodes = (DNode *)(s->rebuild + R.nodes);
  DNode4 *nodes4 = (DNode4 *)(s->rebuild + R.nodes4);
  DItem *sorted = (DItem *)(s->rebuild + R.sorted);
  void *temp = s->rebuild + R.temp;
  hipStream_t st = s->stream;
  auto failed = [&](hipError_t e, const char *what) {
    (void)hipStreamSynchronize(st); // nothing may still use the staging
    return hip_err(e, what);
  };
  // 1-3: the tree a fresh RT_BVH_DEVICE_SAH scene at these positions gets, into staging
  DeviceTree tree;
  hipError_t e = rtk_item_boxes(items0, n, d.spheres, d.quads, d.xforms, boxes, st);
  if (e == hipSuccess)
    e = rtk_build_sah(boxes, items0, n, nodes, sorted, temp, R.temp_bytes, sah_stack_budget(s->tune), &tree.n_nodes,
                      &tree.depth, &tree.root_leaf, st);
  if (e != hipSuccess) return failed(e, "rebuild: device BVH build");
  // 4: accept, or keep the refitted tree.  The instance (RT_FEAT_FLAT, the DRoot table) and the
  // arity are creation's: a root leaf, a tree deeper than the stack or than the 4-wide verdict
  // allows, or one the residency plan refuses is not taken
  const int max_depth = s->tune.lbvh_max_depth > 0 ? (int)s->tune.lbvh_max_depth : RT_STACK_DEPTH - 1;
  if (tree.root_leaf > 0 || tree.n_nodes < 1 || tree.depth < 0 || tree.depth > max_depth) return RT_OK;
  int n4 = 0, d4 = 0;
  double cost = s->binary_cost;
  if (wide) {
    e = rtk_collapse4(nodes, tree.n_nodes, nodes4, temp, R.temp_bytes, &n4, &d4, st);
    KernelAttrs a4;
    if (e == hipSuccess) e = rtk_instance_attrs(d.features, 0, &a4);
    if (e != hipSuccess) return failed(e, "rebuild: 4-wide collapse");
    if (collapse4_verdict(a4, d.features & ~RT_FEAT_BVH4, d4, s->tune.lds_cap) != COLLAPSE4_FITS) return RT_OK;
    // rt_scene_bvh_cost's figure, with a fresh scene's bits: the host's sum over the binary tree
    std::vector<DNode> host(tree.n_nodes);
    e = upload(s, host.data(), nodes, sizeof(DNode) * host.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return failed(e, "rebuild: BVH download");
    cost = rtx::bvh_sah_cost(host);
  }
  const int n_new = wide ? n4 : tree.n_nodes;
  Residency res;
  if (plan_residency(s, n_new, tree.depth, d4, res) != RT_OK) return RT_OK;
  // a host-built scene's node range holds its creation tree: one for any tree over these items
  const size_t each = wide ? sizeof(DNode4) : sizeof(DNode);
  char *range = (char *)const_cast<DNode *>(d.nodes), *fresh_range = nullptr;
  if (each * (size_t)n_new > s->node_room) {
    e = scene_alloc(s, (void **)&fresh_range, each * (size_t)(n - 1));
    if (e != hipSuccess) return set_err(RT_ERR_OOM, std::string("hipMallocFromPoolAsync nodes: ") + hipGetErrorString(e));
    range = fresh_range;
  }
  // 5: commit.  Up to here nothing live was written
  e = hipMemcpyAsync(range, wide ? (const void *)nodes4 : (const void *)nodes, each * (size_t)n_new,
                     hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(const_cast<DItem *>(d.items), sorted, sizeof(DItem) * (size_t)n, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && s->refit) // a later first move builds them itself (ensure_refit)
    e = rtk_refit_links(range, s->bvh_arity, n_new, s->refit + s->refit_temp, s->refit_temp_bytes, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    scene_free(s, fresh_range);
    return hip_err(e, "rebuild: commit");
  }
  if (fresh_range) {
    s->own_nodes = fresh_range; // (a second one never happens: this one holds the bound)
    s->node_room = each * (size_t)(n - 1);
    d.nodes = (const DNode *)fresh_range;
  }
  d.n_nodes = n_new;
  s->bvh_depth = tree.depth;
  s->bvh_depth4 = d4;
  if (wide) s->binary_cost = cost;
  RtkLdsPlan plan{};
  commit_residency(s, res, plan);
  fill_tree_info(s, plan, RT_BVH_DEVICE_SAH);
  if (rebuilt) *rebuilt = 1;
  return RT_OK;
}

int rt_last_kernel_ms(rt_scene *s, double *ms) {
  if (!s || !ms) return set_err(RT_ERR_INVALID, "null argument");
  if (!s->timed) return set_err(RT_ERR_INVALID, "no kernel launched yet");
  DeviceGuard g(s->device);
  hipError_t e = hipEventSynchronize(s->ev1);
  if (e != hipSuccess) return hip_err(e, "hipEventSynchronize");
  float t = 0;
  e = hipEventElapsedTime(&t, s->ev0, s->ev1);
  if (e != hipSuccess) return hip_err(e, "hipEventElapsedTime");
  *ms = t;
  return RT_OK;
}

int rt_to_bytes_device(const double *rgb, int64_t n, double scale, uint8_t *bytes,
                       void *hip_stream) {
  if (!rgb || !bytes || n < 0) return set_err(RT_ERR_INVALID, "invalid argument");
  hipError_t e = rtk_launch_to_bytes(rgb, n, scale, bytes, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "to_bytes launch");
  return RT_OK;
}

// ---------------------------------------------------------------- tile exchange
int rt_tiles_sum_device(const double *parts, int64_t n_tiles, int32_t chunks, double *device_tiles,
                        void *hip_stream) {
  if (!parts || !device_tiles || n_tiles < 0 || chunks < 1) return set_err(RT_ERR_INVALID, "invalid argument");
  if (parts == device_tiles && chunks > 1) return set_err(RT_ERR_INVALID, "parts and tiles must not alias");
  hipError_t e = rtk_launch_tiles_sum(parts, n_tiles, chunks, device_tiles, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "tiles_sum launch");
  return RT_OK;
}

int rt_tiles_to_frame_device(const double *device_tiles, int32_t n_shards, int64_t shard_stride,
                             const rt_frame *f, const rt_render_params *p, double *device_rgb,
                             void *hip_stream) {
  if (!device_tiles || !device_rgb || !f || !p || n_shards < 1)
    return set_err(RT_ERR_INVALID, "invalid argument");
  DLaunch L;
  int rc = to_launch(f, p, L);
  if (rc) return rc;
  const int64_t n_tiles = (int64_t)L.tiles_x * L.tiles_y;
  if (shard_stride < (n_tiles + n_shards - 1) / n_shards)
    return set_err(RT_ERR_INVALID, "shard_stride below the tiles of one shard");
  hipError_t e = rtk_launch_tiles_to_frame(device_tiles, n_shards, shard_stride, f->image_width, L.row_begin,
                                           L.row_end, f->pixel_samples_scale, p->output == RT_OUT_SCALED,
                                           p->accumulate, device_rgb, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_err(e, "tiles_to_frame launch");
  return RT_OK;
}

// ---------------------------------------------------------------- multi-device
// One rt_scene per shard, one host thread per shard (StaticCamera::render_gpu's
// single-device loop, StaticCamera.cpp:136-313, spread over N devices).  Shard
// k renders tiles k, k+N, k+2N, ... in the compact tile layout and finishes
// them on its own device (shard_finish_kernel: chunk partials added in chunk
// order -- split_sum_kernel's order); the compact tiles travel device to
// device (xGMI peer copies) into a staging buffer on shard 0's device, where
// tiles_to_frame_kernel reorders them into the frame, copied to the host once.
// With the frame launch's chunk split the frame is bit-identical to rt_render
// on one device.
struct rt_multi {
  std::vector<rt_scene *> scenes; // one per shard; scenes[0]'s device is the root
  std::vector<double> ms;
  double gather_ms = 0.0;
  double *stage = nullptr; // root device: [shard][stride tiles][64][3]
  size_t stage_bytes = 0;
  double *frame = nullptr; // root device: the assembled rows
  size_t frame_bytes = 0;
};

int rt_multi_destroy(rt_multi *m) {
  if (!m) return RT_OK;
  if (!m->scenes.empty() && m->scenes[0]) {
    DeviceGuard g(m->scenes[0]->device);
    for (rt_scene *s : m->scenes)
      if (s) {
        DeviceGuard gs(s->device);
        (void)hipStreamSynchronize(s->stream);
      }
    bury(m->scenes[0], m->stage); // idle: every shard stream was synchronised above
    bury(m->scenes[0], m->frame);
  }
  for (rt_scene *s : m->scenes) rt_scene_destroy(s);
  delete m;
  return RT_OK;
}

int rt_multi_create(const rt_scene_desc *desc, const int32_t *devices, int32_t n_devices,
                    int32_t n_shards, rt_multi **out) {
  return rt_multi_create_tuned(desc, devices, n_devices, n_shards, nullptr, out);
}

int rt_multi_create_tuned(const rt_scene_desc *desc, const int32_t *devices, int32_t n_devices,
                          int32_t n_shards, const rt_tuning *tuning, rt_multi **out) {
  if (!out || !desc || !devices) return set_err(RT_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_devices < 1 || n_shards < n_devices)
    return set_err(RT_ERR_INVALID, "need n_devices >= 1 and n_shards >= n_devices");
  if (n_shards > RT_MULTI_MAX_SHARDS) // each shard holds a device scene copy and a host thread
    return set_err(RT_ERR_INVALID, "n_shards exceeds RT_MULTI_MAX_SHARDS");
  rt_multi *m = new (std::nothrow) rt_multi();
  if (!m) return set_err(RT_ERR_OOM, "host allocation");
  std::vector<int> rc(n_shards, RT_OK);
  std::vector<std::string> err(n_shards);
  try {
    m->scenes.assign(n_shards, nullptr);
    m->ms.assign(n_shards, 0.0);
    std::vector<std::thread> th;
    try {
      for (int k = 0; k < n_shards; ++k)
        th.emplace_back([&, k]() {
          rc[k] = rt_scene_create_tuned(desc, devices[k % n_devices], tuning, &m->scenes[k]);
          if (rc[k] != RT_OK) err[k] = g_err; // thread-local message of this worker
        });
    } catch (const std::exception &ex) { // thread creation failed: join the started ones
      for (auto &t : th) t.join();
      rt_multi_destroy(m);
      return set_err(RT_ERR_DEVICE, std::string("shard thread: ") + ex.what());
    }
    for (auto &t : th) t.join();
  } catch (const std::exception &ex) { // host allocation inside the containers
    rt_multi_destroy(m);
    return set_err(RT_ERR_OOM, std::string("rt_multi_create: ") + ex.what());
  }
  for (int k = 0; k < n_shards; ++k)
    if (rc[k] != RT_OK) {
      rt_multi_destroy(m);
      return set_err(rc[k], "shard " + std::to_string(k) + ": " + err[k]);
    }
  // direct xGMI access from every shard device to the root's memory (where
  // the peer copies land); without it hipMemcpyPeerAsync stages through the host
  const int root = devices[0];
  for (int d = 1; d < n_devices && d < n_shards; ++d) {
    if (devices[d] == root) continue;
    int can = 0;
    const hipError_t ce = hipDeviceCanAccessPeer(&can, devices[d], root);
    if (ce != hipSuccess) (void)hipGetLastError();
    if (ce == hipSuccess && can) {
      DeviceGuard g(devices[d]);
      const hipError_t e = hipDeviceEnablePeerAccess(root, 0);
      // any failure (already enabled or not) leaves no direct peer access to
      // rely on: the peer copies then stage through the host.  Clear the
      // thread's last error so the first multi frame's launch checks do not
      // report it.
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorPeerAccessAlreadyEnabled)
          fprintf(stderr, "rt_multi_create: no peer access from device %d to %d (%s); "
                          "peer copies stage through the host\n",
                  devices[d], root, hipGetErrorString(e));
      }
    }
  }
  *out = m;
  return RT_OK;
}

// One shard of rt_multi_render: the tiles t = first + k * stride in the tile
// layout with the one-device frame's split plan -- tiles below plan.n_head
// (global index) as head units, the rest as tail chunks -- raw sums, finished
// on the shard's device into its compact tiles [k][64][3] (whole head tiles
// by their own units, chunked tiles by shard_finish_kernel), then copied into
// the root's staging slot `dst`.  *t_done: host clock (ms) when the render and
// finish kernels had completed.
static int render_shard(rt_scene *s, const rt_frame *f, const rt_render_params *p, int first, int stride,
                        const UnitPlan &plan, double *dst, int root_dev, double *t_done) {
  DCamera C;
  DLaunch L;
  rt_render_params q = *p;
  q.tile_first = first;
  q.tile_stride = stride;
  q.layout = RT_LAYOUT_TILES;
  q.strata_chunks = 0;
  q.output = RT_OUT_SUM;
  q.accumulate = 0;
  int rc = to_device_camera(f, C);
  if (rc) return rc;
  if ((rc = to_launch(f, &q, L))) return rc;
  const UnitPlan sp = shard_plan(plan, first, stride, L.n_local_tiles);
  DeviceGuard g(s->device);
  const size_t nt = (size_t)L.n_local_tiles * 64 * 3;
  if ((rc = ensure_out(s, std::max<size_t>(nt, 1) * sizeof(double)))) return rc;
  DLaunch done;
  if ((rc = launch(s, C, L, s->out_buf, nullptr, s->stream, &sp, &done))) return rc;
  hipError_t e = rtk_launch_shard_finish(&done, s->out_buf, s->stream);
  if (e == hipSuccess && (rc = mark_last(s, s->stream))) return rc;
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return hip_err(e, "shard render");
  *t_done = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  if (nt) {
    e = s->device == root_dev
            ? hipMemcpyAsync(dst, s->out_buf, nt * sizeof(double), hipMemcpyDeviceToDevice, s->stream)
            : hipMemcpyPeerAsync(dst, root_dev, s->out_buf, s->device, nt * sizeof(double), s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) return hip_err(e, "shard tiles to the root device");
  }
  return RT_OK;
}

int rt_multi_render(rt_multi *m, const rt_frame *f, const rt_render_params *p, double *host_rgb) {
  if (!m || !host_rgb || !p) return set_err(RT_ERR_INVALID, "null argument");
  if (p->tile_first != 0 || p->tile_stride > 1 || p->layout != RT_LAYOUT_FRAME)
    return set_err(RT_ERR_INVALID, "rt_multi_render takes a whole-frame launch "
                                   "(tile_first 0, tile_stride 0/1, RT_LAYOUT_FRAME)");
  DLaunch L;
  rt_render_params full = *p;
  full.strata_chunks = 0;
  full.accumulate = 0;
  int rc = to_launch(f, &full, L);
  if (rc) return rc;
  const int n = (int)m->scenes.size();
  rt_scene *root = m->scenes[0];
  // the one-device frame launch's units (so the frame is bit-identical to
  // rt_render on one device), or every tile in strata_chunks chunks if asked
  const UnitPlan plan = p->strata_chunks > 0 ? chunks_plan(p->strata_chunks, L.sample_count)
                                             : frame_plan(plan_device(root), root->tune, L);
  const int64_t n_tiles = (int64_t)L.tiles_x * L.tiles_y;
  const int64_t stride = (n_tiles + n - 1) / n; // staging slot per shard, in tiles
  const size_t frame_d = (size_t)(L.row_end - L.row_begin) * f->image_width * 3;
  {
    DeviceGuard g(root->device);
    // the last rt_multi_render synchronised every shard's stream and the
    // root's before it returned: nothing still uses the two buffers
    if ((rc = grow(root, m->stage, m->stage_bytes, std::max<size_t>(1, (size_t)n * stride * 64 * 3) * sizeof(double),
                   Idle::Already, "hipMalloc multi staging")))
      return rc;
    if ((rc = grow(root, m->frame, m->frame_bytes, std::max<size_t>(1, frame_d) * sizeof(double), Idle::Already,
                   "hipMalloc multi frame")))
      return rc;
  }
  std::vector<int> src(n, RT_OK);
  std::vector<double> t_done(n, 0.0);
  std::vector<std::string> err(n);
  std::vector<std::thread> th;
  try {
    for (int k = 0; k < n; ++k) {
      m->ms[k] = 0.0;
      if (k >= n_tiles) continue; // more shards than tiles
      th.emplace_back([&, k]() {
        src[k] = render_shard(m->scenes[k], f, p, k, n, plan, m->stage + (size_t)k * stride * 64 * 3,
                              root->device, &t_done[k]);
        if (src[k] == RT_OK) src[k] = rt_last_kernel_ms(m->scenes[k], &m->ms[k]);
        if (src[k] != RT_OK) err[k] = g_err;
      });
    }
  } catch (const std::exception &ex) { // thread creation failed: join the started ones
    for (auto &t : th) t.join();
    return set_err(RT_ERR_DEVICE, std::string("shard thread: ") + ex.what());
  }
  for (auto &t : th) t.join();
  for (int k = 0; k < n; ++k)
    if (src[k] != RT_OK) return set_err(src[k], "shard " + std::to_string(k) + ": " + err[k]);
  DeviceGuard g(root->device);
  hipError_t e = rtk_launch_tiles_to_frame(m->stage, n, stride, f->image_width, L.row_begin, L.row_end,
                                           f->pixel_samples_scale, p->output == RT_OUT_SCALED, 0, m->frame,
                                           root->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(root->stream);
  if (e != hipSuccess) return hip_err(e, "tiles_to_frame");
  const double t_frame =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  m->gather_ms = t_frame - *std::max_element(t_done.begin(), t_done.end());
  e = hipMemcpyAsync(host_rgb, m->frame, frame_d * sizeof(double), hipMemcpyDeviceToHost, root->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(root->stream);
  if (e != hipSuccess) return hip_err(e, "frame D2H");
  return RT_OK;
}

int rt_multi_move_spheres(rt_multi *m, int32_t n, const int32_t *object_ids, const double *centres) {
  if (!m) return set_err(RT_ERR_INVALID, "null argument");
  // the shards hold one description: what the first refuses none has applied
  for (rt_scene *s : m->scenes)
    if (int rc = rt_scene_move_spheres(s, n, object_ids, centres)) return rc;
  return RT_OK;
}

int rt_multi_set_transforms(rt_multi *m, int32_t n, const int32_t *object_ids, const double *values) {
  if (!m) return set_err(RT_ERR_INVALID, "null argument");
  for (rt_scene *s : m->scenes) // one description: what the first refuses none has applied
    if (int rc = rt_scene_set_transforms(s, n, object_ids, values)) return rc;
  return RT_OK;
}

int rt_multi_move_quads(rt_multi *m, int32_t n, const int32_t *object_ids, const double *corners) {
  if (!m) return set_err(RT_ERR_INVALID, "null argument");
  for (rt_scene *s : m->scenes)
    if (int rc = rt_scene_move_quads(s, n, object_ids, corners)) return rc;
  return RT_OK;
}

int rt_multi_rebuild_bvh(rt_multi *m, int32_t *rebuilt) {
  if (rebuilt) *rebuilt = 0;
  if (!m) return set_err(RT_ERR_INVALID, "null argument");
  // the shards hold one description and one tuning: they decide alike
  int32_t all = 1;
  for (rt_scene *s : m->scenes) {
    int32_t one = 0;
    if (int rc = rt_scene_rebuild_bvh(s, &one)) return rc;
    all &= one;
  }
  if (rebuilt) *rebuilt = m->scenes.empty() ? 0 : all;
  return RT_OK;
}

int rt_multi_trace(rt_multi *m, int64_t n, const rt_ray *rays, rt_ray_hit *hits) {
  // the shards hold one description; a null multi is refused as rt_trace refuses a null scene
  return rt_trace(m && !m->scenes.empty() ? m->scenes[0] : nullptr, n, rays, hits);
}

int rt_multi_occluded(rt_multi *m, int64_t n, const rt_ray *rays, uint8_t *occluded) {
  return rt_occluded(m && !m->scenes.empty() ? m->scenes[0] : nullptr, n, rays, occluded); // as rt_multi_trace
}

int rt_multi_radiance(rt_multi *m, int64_t n, const rt_ray *rays, const rt_radiance_params *p, double *rgb) {
  return rt_radiance(m && !m->scenes.empty() ? m->scenes[0] : nullptr, n, rays, p, rgb); // as rt_multi_trace
}

int rt_multi_shard_ms(rt_multi *m, double *ms) {
  if (!m || !ms) return set_err(RT_ERR_INVALID, "null argument");
  for (size_t k = 0; k < m->ms.size(); ++k) ms[k] = m->ms[k];
  return RT_OK;
}

int rt_multi_gather_ms(rt_multi *m, double *ms) {
  if (!m || !ms) return set_err(RT_ERR_INVALID, "null argument");
  *ms = m->gather_ms;
  return RT_OK;
}

} // extern "C"
