// rt_kernel.hip — gfx950 path-tracing megakernel (the hot path).
//
// Replaces static_render_kernel + ray_color_cuda + init_rand_states
// (CameraKernels.cu:15-25, 106-202, 240-278).  Same estimator as the reference CPU
// integrator (Camera.cpp:232-309), restructured for CDNA4:
//
//  * one 64-lane wavefront owns one 8x8-pixel tile; its work queue is the
//    tile's 64 pixels x the launched strata; lanes that finish a path pull the
//    next (pixel, stratum) item with __ballot + mbcnt ("path regeneration"), so
//    the wave stays full until the tile's queue drains instead of idling lanes
//    whose pixels finished early (sky pixels vs multi-bounce pixels);
//  * the recursive integrator becomes an iterative bounce loop carrying a
//    throughput; every lane traces exactly one segment per loop trip (in the
//    plain flat world a lane that hit waits, parked, until enough lanes of its
//    wave have a hit to shade: RT_PARK_MIN);
//  * stateless Philox4x32-10 random numbers keyed by (seed; pixel, stratum,
//    bounce, slot) — no per-pixel curandState traffic (48 B/pixel/sample in the
//    reference) and sample ranges shard across GPUs exactly;
//  * BVH traversal (rt_path.h) with both child boxes per node, near-first
//    while-while order and a per-lane stack in LDS (stack[depth][lane]:
//    consecutive lanes on consecutive banks);
//  * per-pixel fp64 sums in LDS (ds_add_f64), written once per tile with
//    coalesced stores;
//  * scene-feature specialisation: the launcher picks the instance compiled for
//    the features the scene uses (media, transform chains, light sampling,
//    Perlin noise), so e.g. a sphere-only scene runs without the fog and
//    light-sampling code and its register cost.
// All arithmetic is fp64 like the reference (Vec3.hpp:184); built with
// -ffp-contract=off so expression rounding follows the reference's order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
#include <mutex>
#include <set>
#include <utility>

#include "rt_camq.h"
#include "rt_cull.h"
#include "rt_kernels.h"
#include "rt_lds_plan.h"
#include "rt_path.h"
#include "rt_plan.h"

namespace {

using namespace rtp;
// Idle lanes that trigger a refill while other lanes still trace (measured:
// 16 for the plain instance, C3 +4 %; the rich instances lose with any delay).
// The plain flat world pops its camera rays from a queue (rt_camq.h), a refill
// pass at about a fifth of its former price: re-measured with it, 1 / 4 / 8 /
// 16 idle lanes x RT_PARK_K 48 / 56 all lie within 3.92-3.97 ms of C2 kernel
// time, none apart from (16, 48) (profiles/camq_sweep_ab.log).
#ifndef RT_REGEN_FLAT
#define RT_REGEN_FLAT 16 // re-measured with RT_PARK_K (profiles/parked_k_ab.log, camq_sweep_ab.log)
#endif
#define RT_REGEN_MIN(F) ((F) == F_FLAT ? RT_REGEN_FLAT : (((F) & ~F_BVH4) == 0 ? 16 : 1))
// Parked shading (the plain flat world, every instance of it: M_ANY, M_DIFFUSE,
// STATS, COST): a lane whose trace hit keeps (closest, best) and is shaded only
// once this many lanes of its wave hold a hit, or no refill can add to them --
// shade, the dearest block of a trip, then runs once for the few bounce rays
// that hit and the camera rays of the next refill together.  0: trace and shade
// in one step (segment).  Measured on C2: DESIGN.md §7, profiles/parked_*.
#ifndef RT_PARK_K
#define RT_PARK_K 48
#endif
#define RT_PARK_MIN(F) ((F) == F_FLAT ? RT_PARK_K : 0)
// Occupancy target per instance (waves per SIMD): the compiler may spill a few
// registers to reach it.  Measured: 4 for the plain instance (C3
// +12 % over 3), 3 for the rich ones (C4 +8.6 % over the 2 that 224 VGPRs give).
#define RT_WAVES_PER_EU(F) ((F) == F_FLAT ? 4 : (((F) & ~F_BVH4) == 0 ? 4 : 3))
// The launch fields read afresh from the kernarg segment at each work unit
// (FRESH, the persistent instances): the asm hides the segment pointer's
// value, so the loads stay inside the unit loop instead of being hoisted out
// of it and held in SGPRs across every path trip.  KArgs mirrors
// render_tiles' explicit arguments (laid out in order, naturally aligned);
// the parameter's own address is never taken (that copies it to scratch).
struct KArgs {
  DScene S;
  DCamera C;
  DLaunch P;
  double *out;
  unsigned long long *stats;
};
// The AMDGPU kernarg segment places explicit arguments in order at their
// natural alignment -- the layout of this struct.  The expected offsets are
// spelled out so a field added to DScene / DCamera / DLaunch breaks the build
// here instead of silently shifting what the persistent instance reads (its
// frames are also checked bit for bit against the one-unit-per-wave instance
// on the GPU: tests/test_persistent.py, and through every BASELINE band).
static_assert(sizeof(DScene) == 176 && alignof(DScene) == 8, "DScene kernarg layout");
static_assert(sizeof(DCamera) == 208 && alignof(DCamera) == 8, "DCamera kernarg layout");
static_assert(sizeof(DLaunch) == 112 && alignof(DLaunch) == 8, "DLaunch kernarg layout");
static_assert(offsetof(KArgs, S) == 0 && offsetof(KArgs, C) == 176 && offsetof(KArgs, P) == 384 &&
                  offsetof(KArgs, out) == 496 && offsetof(KArgs, stats) == 504 &&
                  sizeof(KArgs) == 512,
              "KArgs must mirror render_tiles' kernarg layout");
static_assert(offsetof(DLaunch, n_chunks) == 56 && offsetof(DLaunch, unit_ctr) == 64 &&
                  offsetof(DLaunch, grid_cap) == 72 && offsetof(DLaunch, n_head) == 76 &&
                  offsetof(DLaunch, parts) == 80 && offsetof(DLaunch, parts_final) == 88 &&
                  offsetof(DLaunch, head_chunks) == 92 && offsetof(DLaunch, tile_order) == 96 &&
                  offsetof(DLaunch, tile_cost) == 104,
              "DLaunch field offsets read from the kernarg segment");
template <bool FRESH>
__device__ __forceinline__ DLaunch launch_fields(const DLaunch &P) {
  if constexpr (FRESH) {
    auto ka = (const __attribute__((address_space(4))) KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const __attribute__((address_space(4))) DLaunch &K = ka->P;
    DLaunch L;
    L.row_begin = K.row_begin;
    L.row_end = K.row_end;
    L.sample_begin = K.sample_begin;
    L.sample_count = K.sample_count;
    L.seed_lo = K.seed_lo;
    L.seed_hi = K.seed_hi;
    L.output = K.output;
    L.accumulate = K.accumulate;
    L.tiles_x = K.tiles_x;
    L.tiles_y = K.tiles_y;
    L.tile_first = K.tile_first;
    L.tile_stride = K.tile_stride;
    L.n_local_tiles = K.n_local_tiles;
    L.compact = K.compact;
    L.n_chunks = K.n_chunks;
    L.chunk_strata = K.chunk_strata;
    L.unit_ctr = K.unit_ctr;
    L.grid_cap = K.grid_cap;
    L.n_head = K.n_head;
    L.parts = K.parts;
    L.parts_final = K.parts_final;
    L.head_chunks = K.head_chunks;
    L.tile_order = K.tile_order;
    L.tile_cost = K.tile_cost;
    return L;
  } else {
    return P;
  }
}
// The epilogue's camera fields read afresh from the kernarg segment (FRESH:
// once per work unit, outside the path loop, so the one-unit instances need
// not hold them in SGPRs across every path trip).  Scalar loads through the
// asm-hidden segment pointer: they stay at the use, the scalar cache serves them.
// non-flat instances only: the flat one measured -0.5 % kernel time with it
// (C2; C4 neutral); profiles/r03l_ab.log
#define RT_EPI_FRESH_F(F) (((F) & F_FLAT) == 0)
template <bool FRESH>
__device__ __forceinline__ DCamera camera_fields(const DCamera &C) {
  if constexpr (FRESH) {
    auto ka = (const __attribute__((address_space(4))) KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const __attribute__((address_space(4))) DCamera &K = ka->C;
    DCamera D;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      D.center[k] = K.center[k];
      D.p00[k] = K.p00[k];
      D.du[k] = K.du[k];
      D.dv[k] = K.dv[k];
      D.disk_u[k] = K.disk_u[k];
      D.disk_v[k] = K.disk_v[k];
      D.bg[k] = K.bg[k];
    }
    D.defocus_angle = K.defocus_angle;
    D.scale = K.scale;
    D.rs = K.rs;
    D.W = K.W;
    D.H = K.H;
    D.sqrt_spp = K.sqrt_spp;
    D.max_depth = K.max_depth;
    return D;
  } else {
    return C;
  }
}
// The plan's local tile of work unit `unit` (head units: unit / head_chunks;
// tail units: n_head + (unit - head units) / n_chunks), and the launch's
// local tile it maps to (cost-ordered dispatch: tile_order; null: itself).
__device__ __forceinline__ int plan_tile(const DLaunch &L, int unit) {
  const int head_units = L.n_head * L.head_chunks;
  return unit < head_units ? unit / L.head_chunks : L.n_head + (unit - head_units) / L.n_chunks;
}
__device__ __forceinline__ int order_tile(const DLaunch &L, int k) {
  return L.tile_order != nullptr ? __builtin_amdgcn_readfirstlane(L.tile_order[k]) : k;
}
// Cost-ordered dispatch (rt_api.cpp "tile order"): every instance maps its
// units through the launch's tile order (a scalar load per unit); the STATS
// instance measures tile costs, in the probe launch that orders a launch
// shape once (rt_api.cpp tile_order_probe).  The cost bookkeeping compiled
// into a render instance cost it registers and schedule even when skipped at
// run time: C4 -12.5 % (r05u_ab.log), C2 / C3 / C5 -0.9 % (r06y_ab_C*.log);
// so it lives in one extra instance (COST) of the flat world only, for the
// tile-subset launches of a multi-GPU rank, whose order re-measured after
// every launch beats the probe's (r06ad / r06af: 8-way C2 share).
// rtk_cost_f mirrors it for the host.
#define RT_COST_F(F) ((F) == F_FLAT)
extern "C" int rtk_cost_f(int features) { return RT_COST_F((unsigned)features & F_ALL) ? 1 : 0; }
template <bool FRESH>
__device__ __forceinline__ double *out_arg(double *out) {
  if constexpr (FRESH) {
    auto ka = (const __attribute__((address_space(4))) KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return ka->out;
  } else {
    return out;
  }
}

// Tile culling (rt_cull.h; the plain flat world's render instances and COST
// twin): roots a tile's camera rays cannot reach are not tested at generation,
// and a tile that reaches none is settled without rays.  0 builds the flow
// without it, for A/B runs (make EXTRA=-DRT_TILE_CULL=0).
#ifndef RT_TILE_CULL
#define RT_TILE_CULL 1
#endif
#ifndef RT_UNIT_TIMES
#define RT_UNIT_TIMES 0
#endif
#if RT_UNIT_TIMES
// Measurement-only build (make EXTRA=-DRT_UNIT_TIMES=1; tools/unit_timeline.py):
// every work unit's start and end on the device's constant 100 MHz clock
// (s_memrealtime), by unit index, for the launch timeline (how long the
// waves' last units keep the launch open).
constexpr int kUnitTimesMax = 1 << 21;
__device__ unsigned long long g_unit_times[2 * kUnitTimesMax];
extern "C" hipError_t rtk_unit_times(unsigned long long *host, int n_units) {
  const size_t n = 2 * (size_t)(n_units < kUnitTimesMax ? n_units : kUnitTimesMax);
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_unit_times), n * sizeof(unsigned long long), 0,
                             hipMemcpyDeviceToHost);
}
extern "C" hipError_t rtk_unit_times_clear(void) {
  void *p = nullptr;
  hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(g_unit_times));
  if (e != hipSuccess) return e;
  e = hipMemset(p, 0, sizeof(g_unit_times));
  return e != hipSuccess ? e : hipDeviceSynchronize();
}
#endif

// PC (persistent): the instance for launches of more units than the grid's
// resident waves -- frame launches (head units, then the tail chunks) and
// tile-subset launches (multi-GPU shards) alike -- whose waves persist and
// pull units; it reads the per-unit launch fields afresh from the kernarg
// segment, so they are not live across the path loop.
// PCW: 0 = one work unit per wavefront; else a persistent instance with
// blocks of PCW waves (kPcWaves = one block per CU; kWaves when the traversal
// stacks of 16 waves do not fit the CU's LDS, e.g. deep 4-wide trees)
// MS: the material set shade is compiled for (rt_path.h MatSet)
template <bool STATS, unsigned F, int PCW = 0, bool COST = false, MatSet MS = M_ANY>
__global__ __launch_bounds__(64 * (PCW ? PCW : block_waves(F))) __attribute__((amdgpu_waves_per_eu(RT_WAVES_PER_EU(F)))) void render_tiles(DScene S_, DCamera C, DLaunch P, double *out,
                                                    unsigned long long *stats) {
  constexpr bool PC = PCW > 0;
  constexpr int BW = PC ? PCW : block_waves(F); // waves per block
  // the persistent instance stages its own (larger) node prefix
  DScene S = S_;
  if constexpr (PC) S.n_lds_nodes = S_.n_lds_nodes_pc;
  // dynamic LDS: traversal stacks [BW][S.stack_depth][64] ints, then the
  // staged BVH prefix nodes [0, S.n_lds_nodes) (sizes: rt_lds_plan.h lds_bytes)
  extern __shared__ int4 dyn_lds[];
  __shared__ double acc_lds[BW][64][3];
  // compacted leaf tests (BVH instances only; 1 KB per wave)
  __shared__ LeafPool leaf_pool[RT_LEAF_SHARE_F(F) ? BW : 1];

  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  int *stack_base = reinterpret_cast<int *>(dyn_lds);
  DNode *lnodes_g = reinterpret_cast<DNode *>(stack_base + BW * S.stack_depth * 64);
  const RT_LDS DNode *lnodes = (const RT_LDS DNode *)lnodes_g; // DNode4 in BVH4 instances
  constexpr int kNodeBytes = RT_LDS_NODE_BYTES(F);
  // persistent instance: world items and spheres after the nodes (LdsPrims)
  LdsPrims lp{nullptr, nullptr};
  int4 *prim_g = reinterpret_cast<int4 *>(lnodes_g) + (size_t)max(0, S.n_lds_nodes) * (kNodeBytes / 16);
  if constexpr (PC) {
    if (S.lds_items_pc > 0) {
      lp.items = (const RT_LDS DItem *)reinterpret_cast<DItem *>(prim_g);
      lp.spheres = (const RT_LDS DSphere *)reinterpret_cast<DSphere *>(prim_g + (size_t)S.lds_items_pc * 2);
    }
  }
  if (S.n_lds_nodes > 0 || (PC && S.lds_items_pc > 0)) { // stage once per block
    if constexpr ((F & F_BVH4) != 0) {
      const int4 *src = reinterpret_cast<const int4 *>(S.nodes);
      int4 *dst = reinterpret_cast<int4 *>(lnodes_g);
      const int n16 = max(0, S.n_lds_nodes) * (kNodeBytes / 16);
      for (int k = threadIdx.x; k < n16; k += blockDim.x) dst[k] = src[k];
    } else {
      // binary nodes as DNodeL: 8-B unit j of staged node i is, per axis a =
      // j / 3, the lo pair (8a in the DNode), the hi pair (24 + 8a), the lo pair
      // again; unit 9 the child entries (48) -- inner children as DNodeL byte
      // offsets when the whole tree is staged (the LDS-only walk's `cur`)
      const uint2 *src = reinterpret_cast<const uint2 *>(S.nodes);
      uint2 *dst = reinterpret_cast<uint2 *>(lnodes_g);
      const int n8 = max(0, S.n_lds_nodes) * 10;
      const bool whole = S.n_lds_nodes >= S.n_nodes; // trace()'s LDS-only walk
      for (int k = threadIdx.x; k < n8; k += blockDim.x) {
        const int i = k / 10, j = k - 10 * (k / 10);
        const int a = j / 3, m = j - 3 * (j / 3);
        const int u = j == 9 ? 6 : (m == 1 ? 3 + a : a);
        uint2 v = src[8 * i + u];
        if (j == 9 && whole) {
          if ((int)v.x >= 0) v.x *= (unsigned)sizeof(DNodeL);
          if ((int)v.y >= 0) v.y *= (unsigned)sizeof(DNodeL);
        }
        dst[k] = v;
      }
    }
    if constexpr (PC) {
      if (S.lds_items_pc > 0) {
        const int ni = S.lds_items_pc * 2, ns = S.lds_spheres_pc * 4; // int4 per DItem / DSphere
        const int4 *si = reinterpret_cast<const int4 *>(S.items);
        const int4 *ss = reinterpret_cast<const int4 *>(S.spheres);
        for (int k = threadIdx.x; k < ni; k += blockDim.x) prim_g[k] = si[k];
        for (int k = threadIdx.x; k < ns; k += blockDim.x) prim_g[ni + k] = ss[k];
      }
    }
    __syncthreads();
  }
  if constexpr ((F & F_NOISE) != 0) { // the Perlin table (tex_value), once per block
    if (S.lds_perlin) {
      const int4 *src = reinterpret_cast<const int4 *>(S.perlin);
      RT_LDS int4 *dst = (RT_LDS int4 *)perlin_lds();
      for (int k = threadIdx.x; k < (int)(sizeof(DPerlin) / 16); k += blockDim.x) dst[k] = src[k];
      __syncthreads();
    }
  }
  // work unit = (local tile, stratum chunk).  Persistent launches (P.unit_ctr
  // set, grid = the resident waves): a wave's first unit is its static slot,
  // the next ones come from the agent-scope counter (initialised by the host to
  // the grid's wave count), so waves take new units as they finish instead of
  // waiting for their block.
  // The unit count, the unit decode below and the epilogue's `part` are this
  // kernel's own copy of rt_plan.h's plan_units / plan_unit (routing them
  // through the shared helpers changed the instances' register allocation):
  // they must agree with it.  tests/test_multi.py, test_subset_auto.py,
  // test_tile_order.py and test_persistent.py tie the two together -- a
  // disagreement misplaces partial sums and breaks their bit-identity asserts.
  const int n_units = P.n_head * P.head_chunks + (P.n_local_tiles - P.n_head) * P.n_chunks;
  int unit = blockIdx.x * BW + wv;
  int *stk = stack_base + wv * S.stack_depth * 64 + lane;
  double *acc = &acc_lds[wv][0][0];
  Counters cnt{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t cyc_regen = 0;
  const uint64_t t_start = STATS ? clk() : 0;
  uint32_t n_samples = 0, n_segments = 0, n_trips = 0;
  // traversal-SIMD model (STATS): per trip the largest per-lane visit count,
  // and for trips paired back to back the largest per-lane sum of the pair
  uint64_t m_single = 0, m_pair = 0;
  uint32_t v_prev = 0, m_prev = 0;
  bool have_prev = false;
  auto wave_max = [](uint32_t x) {
    for (int off = 32; off > 0; off >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, off));
    return x;
  };
  while (unit < n_units) { // wave-uniform
#if RT_UNIT_TIMES
  const unsigned long long t_unit0 = __builtin_amdgcn_s_memrealtime();
#endif
  const DLaunch PU = launch_fields<PC>(P);
  // (wave-uniform) head unit: tile unit / head_chunks; tail unit: a chunk of
  // the tail tile n_head + (unit - head units) / n_chunks
  const int head_units = PU.n_head * PU.head_chunks;
  const bool whole = PU.head_chunks == 1 && unit < PU.n_head;
  int local_tile, s_first, s_count;
  {
    const bool head = unit < head_units;
    const int nc = head ? PU.head_chunks : PU.n_chunks;
    const int cs = head ? (PU.sample_count + nc - 1) / nc : PU.chunk_strata;
    const int u = head ? unit : unit - head_units, q = u / nc, chunk = u - q * nc;
    local_tile = head ? q : PU.n_head + q;
    s_first = PU.sample_begin + chunk * cs;
    s_count = min(cs, PU.sample_count - chunk * cs);
  }
  // the plan's k-th tile -> the launch's local tile (cost-ordered dispatch);
  // in the probe (STATS) and the COST instance the unit's cost is its end time
  // minus its start time, both added to the tile's counter (mod 2^32), so no
  // start time is held across the path loop
  local_tile = order_tile(PU, local_tile);
  if constexpr (STATS || COST) {
    if (lane == 0 && PU.tile_cost != nullptr)
      atomicSub(&PU.tile_cost[local_tile], (unsigned)__builtin_amdgcn_s_memrealtime());
  }
  const int tile = PU.tile_first + local_tile * PU.tile_stride;
  const int tx = tile % PU.tiles_x, ty = tile / PU.tiles_x;
  const int x0 = tx * 8, y0 = PU.row_begin + ty * 8;
  acc[lane * 3 + 0] = 0.0;
  acc[lane * 3 + 1] = 0.0;
  acc[lane * 3 + 2] = 0.0;

  int n_items = 64 * max(0, s_count); // wave-uniform; 0 for a unit settled without rays (kCull)
  int next_item = 0; // wave-uniform head of the tile's work queue
  // camera rays generated a batch at a time by the whole wave and popped from
  // LDS (rt_camq.h): the plain flat world, every instance of it
  constexpr bool kCamq = F == F_FLAT;
  [[maybe_unused]] int gen_items = 0; // items generated so far (wave-uniform, whole batches)
  PathState ps;
  ps.active = false;
  Key key{P.seed_lo, P.seed_hi, 0, 0};
  // gen_trace: camera-ray batches are traced where they are generated (the
  // refill below) -- no defocus disk, a world with a root table, whose walk
  // is the root tests alone (rt_path.h trace_closest_roots), and a unit of
  // more than one batch: a one-batch unit (the progressive frames) is popped
  // by all 64 lanes at once and traced at full lane use as it is, and measured
  // 1.2-2.5 % slower with the detour (profiles/batch_progressive_ab.log).  A flat world
  // without a table (a quad, a moving or a transformed sphere among its root
  // items) keeps the flow of a camera with a disk: the whole walk inlined a
  // second time costs the Lambertian-only instance its register advantage
  // (127 VGPRs, the general instance's count, and 2 of them spilled).
  // org_tab: every camera ray of the unit leaves the camera centre, so the
  // (oc, c) per root (rt_path.h root_origin) are formed here once per unit
  // and the generation-time trace reads them from LDS, one address in
  // every lane; a table of more than kRootOriginMax roots takes the general
  // root test there.  Both wave-uniform.
  // root_mask (kCull: the render instances and the COST twin; the STATS
  // instance keeps the full flow and its counters): bit ii says that a camera
  // ray of this tile may reach root ii (rt_cull.h: a conservative reach test of
  // the tile's bounding cone against the root, lane ii doing root ii).  It is
  // formed where the table is (org_tab) and serves twice:
  // the generation-time trace walks the set bits only (a skipped test is one
  // that returned false, so (closest, best) keep their bits), and a unit whose
  // mask is empty is settled without rays: every one of its samples is
  // 1.0 * bg, added below by the pop's own LDS add, s_count times per pixel of
  // the image, and the unit goes to the epilogue with an empty work queue.
  // Bounce rays keep the full walk: their origins differ per lane.
  constexpr bool kCull = RT_TILE_CULL != 0 && kCamq && !STATS && kRootOriginMax > 0;
  static_assert(kRootOriginMax <= 32, "root_mask holds a bit per table entry");
  [[maybe_unused]] bool gen_trace = false, org_tab = false;
  [[maybe_unused]] uint32_t root_mask = ~0u; // wave-uniform
  [[maybe_unused]] const RT_LDS RootOrigin *root_org = nullptr;
  if constexpr (kCamq) {
    __shared__ RootOrigin root_org_lds[kRootOriginMax > 0 ? kRootOriginMax : 1];
    root_org = (const RT_LDS RootOrigin *)&root_org_lds[0];
    gen_trace = RT_ROOT_TABLE_F(F) && n_items > rtq::kBatch && C.defocus_angle <= 0 && S.n_roots > 0;
    org_tab = gen_trace && S.n_roots <= kRootOriginMax;
    if constexpr (!kCull) {
      if (org_tab) { // a unit that does not read the table pays nothing for it
        const DCamera Co = camera_fields<true>(C);
        for (int ii = 0; ii < S.n_roots; ++ii) { // the walk's own scalar loads: no vector load opens a unit
          const RootOrigin q = root_origin(ldu<true>(&S.roots[ii].test, 0), ld3(Co.center));
          if (lane == 0) root_org_lds[ii] = q;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    } else if (org_tab) {
      // the table and the mask.  Units of more than one batch only: the cone
      // and the reach test are about 400 VALU instructions (six fp64 divisions,
      // five square roots), which 64 batches do not notice and one batch does
      // -- with the mask formed for one-batch units too, the one-stratum C2
      // frames measured 0.157-0.158 -> 0.175-0.176 ms (profiles/cull_progressive_ab.log)
      const DCamera Co = camera_fields<true>(C);
      RootOrigin mq{v3(0.0, 0.0, 0.0), 0.0}; // lane ii: root ii
      double mrr = 0.0;
      for (int ii = 0; ii < S.n_roots; ++ii) { // the walk's own scalar loads: no vector load opens a unit
        const DRootTest e = ldu<true>(&S.roots[ii].test, 0);
        const RootOrigin q = root_origin(e, ld3(Co.center));
        if (lane == 0) root_org_lds[ii] = q;
        if (lane == ii) {
          mq = q;
          mrr = e.rr;
        }
      }
      const TileCone cone = tile_cone(Co, x0, y0);
      root_mask = (uint32_t)__ballot(lane < S.n_roots && !root_unreachable(cone, mq, mrr));
      if (root_mask == 0 && Co.max_depth > 0) { // ---- an all-sky unit
        const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
        if (i < Co.W && j < P.row_end) { // slots outside the image stay 0
          const V3 sky = v3(1.0, 1.0, 1.0) * ld3(Co.bg); // the pop's T * bg, T = 1
          for (int k = 0; k < s_count; ++k) {
            atomicAdd(&acc[lane * 3 + 0], sky.x);
            atomicAdd(&acc[lane * 3 + 1], sky.y);
            atomicAdd(&acc[lane * 3 + 2], sky.z);
          }
        }
        n_items = 0;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  // a parked lane's hit (RT_PARK_MIN): pk_best >= 0 is the flag
  constexpr int kPark = RT_PARK_MIN(F);
  [[maybe_unused]] double pk_closest = 0.0;
  [[maybe_unused]] int pk_best = -1;

  for (;;) {
    // ---- regeneration: idle lanes pull the next (pixel, stratum) items
    const uint64_t t_regen = STATS ? clk() : 0;
    for (;;) {
      unsigned long long idle = __ballot(!ps.active);
      if (idle == 0 || next_item >= n_items) break;
      // refill only once enough lanes are idle: camera-ray generation costs the
      // whole wave, however few lanes take new paths
      if (__popcll(idle) < RT_REGEN_MIN(F) && ~idle != 0ull) break;
      if constexpr (kCamq) {
        // ---- camera-ray queue (rt_camq.h): the batches this pop needs and the
        // ring does not hold yet are generated by the whole wave, lane l making
        // the ray of pixel slot l in the batch's stratum (wave-uniform: the
        // stratum's cell and key.sample on the scalar side); then the idle
        // lanes pop their items.  A ray's arithmetic is camera_ray's, whichever
        // lane runs it.  Where gen_trace holds (above) the batch is traced right
        // there, at full lane use and once per batch: a popped hit arrives
        // parked, a popped miss adds the background and leaves its lane idle,
        // and the refill loop's own repeat (RT_REGEN_MIN idle lanes, items
        // left) fills such lanes again.  The path loop's trace site then sees
        // bounce rays only.  Every ray, root and weight keeps its bits; what
        // moves is when a sky sample joins its pixel's sum.  Otherwise nothing
        // is traced here and a popped lane is traced by the path loop.
        static_assert(BW == 1, "the camera-ray queue is one wave's");
        __shared__ double camq[rtq::kComps][rtq::kEntries];
        const DCamera &Cr = C;
        const bool lens = !(Cr.defocus_angle <= 0); // camera_ray_jt's branch: the origin is drawn
        // this lane's rank among the idle lanes (mbcnt: no lane mask held in registers)
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        const int item = next_item + rank;
        // wave-uniform by construction; said so, so that the loop below is a
        // scalar branch and gen_items and the batch's stratum stay in SGPRs
        const int need = __builtin_amdgcn_readfirstlane(rtq::camq_need(next_item, __popcll(idle), n_items));
        while (rtq::camq_generate(gen_items, need)) { // wave-uniform: all 64 lanes
          // the camera read afresh from the kernarg segment: its fields are not
          // held in SGPRs across the path loop (held, they spill into the trace)
          const DCamera Cg = camera_fields<true>(C);
          const int gk = __builtin_amdgcn_readfirstlane(s_first + rtq::camq_batch(gen_items));
          const int gi = x0 + (lane & 7), gj = y0 + (lane >> 3);
          const Key gkey{P.seed_lo, P.seed_hi, (uint32_t)(gj * Cg.W + gi), (uint32_t)gk};
          const Ray gr = camera_ray<RT_KB_F(F), RT_KCONST_MODE(F)>(Cg, gkey, gi, gj, gk);
          const int e = rtq::camq_write_entry(gen_items, lane);
          camq[0][e] = gr.d.x;
          camq[1][e] = gr.d.y;
          camq[2][e] = gr.d.z;
          camq[3][e] = gr.tm;
          if (lens) {
            camq[4][e] = gr.o.x;
            camq[5][e] = gr.o.y;
            camq[6][e] = gr.o.z;
          } else if (gen_trace) {
            // ---- traced at generation: the batch is complete here, so the
            // closest-hit search of its camera rays runs with every lane of an
            // inside tile, once per batch, and the entry carries its outcome
            // in the origin's place (rtq::kClosest, rtq::kBest; best -1: a
            // miss).  The search is the root-table walk of the path loop's
            // own (trace_closest) on the ray the popping lane would have traced:
            // (closest, best) keep their bits.  A slot outside the image and a depth-0 launch are
            // not traced, as they never were; their entries are not read.
            double g_closest = 0.0;
            int g_best = -1;
            if (gi < Cg.W && gj < P.row_end && Cg.max_depth > 0) {
              if (STATS) n_segments++;
              // timed into cyc_trace like every trace; it also lies inside cyc_regen's
              // span, so the two phase shares overlap by this much
              const uint64_t t0 = STATS ? clk() : 0;
              if constexpr (kCull) {
                if (org_tab) // ... and only the roots this tile can reach are walked
                  trace_closest_roots<STATS, true, true>(S, root_org, gr, g_closest, g_best, cnt, root_mask);
                else
                  trace_closest_roots<STATS, false>(S, root_org, gr, g_closest, g_best, cnt);
              } else if (org_tab) // one origin: (oc, c) per root stand ready (root_org)
                trace_closest_roots<STATS, true>(S, root_org, gr, g_closest, g_best, cnt);
              else
                trace_closest_roots<STATS, false>(S, root_org, gr, g_closest, g_best, cnt);
              if (STATS && wave_once()) cnt.ctrace += clk() - t0;
            }
            camq[rtq::kClosest][e] = g_closest;
            camq[rtq::kBest][e] = __longlong_as_double((long long)g_best);
          }
          gen_items += rtq::kBatch;
        }
        // one wave's LDS operations complete in order: the compiler must only
        // keep the pop's reads after the batch's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        next_item += __popcll(idle);
        if (!ps.active && item < n_items) {
          int slot = item & 63;
          int i = x0 + (slot & 7), j = y0 + (slot >> 3);
          if (i < Cr.W && j < P.row_end) { // an item outside is consumed and leaves its lane idle
            const int e = rtq::camq_read_entry(item);
            ps.slot = slot;
            ps.sample = s_first + (item >> 6);
            key.pixel = (uint32_t)(j * Cr.W + i);
            key.sample = (uint32_t)ps.sample;
            ps.ray.d = v3(camq[0][e], camq[1][e], camq[2][e]);
            ps.ray.tm = camq[3][e];
            ps.T = v3(1.0, 1.0, 1.0);
            ps.bounce = 0;
            if (STATS) n_samples++;
            if (!gen_trace) { // untraced: the path loop's trace site takes it
              ps.ray.o = lens ? v3(camq[4][e], camq[5][e], camq[6][e]) : ld3(Cr.center);
              ps.active = Cr.max_depth > 0;
            } else if (Cr.max_depth > 0) {
              // traced at generation: a hit arrives parked; a miss is the
              // background (Camera.cpp:242-243), added here with the path
              // loop's own add of T * bg, T = 1, and its lane stays idle for
              // the next pass of this refill loop
              ps.ray.o = ld3(Cr.center);
              const int eb = (int)__double_as_longlong(camq[rtq::kBest][e]);
              if (eb >= 0) {
                pk_closest = camq[rtq::kClosest][e];
                pk_best = eb;
                ps.active = true;
              } else {
                const V3 sky = ps.T * ld3(C.bg);
                atomicAdd(&acc[slot * 3 + 0], sky.x);
                atomicAdd(&acc[slot * 3 + 1], sky.y);
                atomicAdd(&acc[slot * 3 + 2], sky.z);
              }
            }
          }
        }
      } else {
        int rank = __popcll(idle & ((1ull << lane) - 1ull));
        int item = next_item + rank;
        next_item += __popcll(idle);
        if (!ps.active && item < n_items) {
          const DCamera &Cr = C;
          int slot = item & 63;
          int i = x0 + (slot & 7), j = y0 + (slot >> 3);
          if (i < Cr.W && j < P.row_end) {
            ps.slot = slot;
            ps.sample = s_first + (item >> 6);
            key.pixel = (uint32_t)(j * Cr.W + i);
            key.sample = (uint32_t)ps.sample;
            ps.ray = camera_ray<RT_KB_F(F), RT_KCONST_MODE(F)>(Cr, key, i, j, ps.sample);
            ps.T = v3(1.0, 1.0, 1.0);
            ps.bounce = 0;
            ps.active = Cr.max_depth > 0;
            if (STATS) n_samples++;
          }
        }
      }
    }
    if (STATS) cyc_regen += clk() - t_regen; // converged here (every lane)
    if (__ballot(ps.active) == 0) break; // a parked lane is active
    if (STATS) n_trips++; // converged here: every lane counts, lane 0 reports
    uint32_t v_trace = 0;
    if constexpr (kPark > 0) {
      // ---- parked shading (RT_PARK_MIN): trace, and shade only once enough
      // lanes hold a hit or no refill can add to them
      bool done = false; // this lane's path ended in this trip: ps.T is its sample
      if (ps.active && pk_best < 0) {
        if (STATS) n_segments++;
        const uint64_t t0 = STATS ? clk() : 0;
        trace_closest<STATS, F, PC>(S, ps.ray, pk_closest, pk_best, stk, lnodes, cnt,
                                    (RT_LDS LeafPool *)&leaf_pool[0], lp);
        if (STATS && wave_once()) cnt.ctrace += clk() - t0;
        if (pk_best < 0) { // miss -> background (Camera.cpp:242-243)
          ps.T = ps.T * ld3(C.bg);
          done = true;
        }
      }
      const bool parked = ps.active && pk_best >= 0;
      // Wave-uniform.  Shading waits only while the next trip's regeneration is
      // certain to take items: with next_item < n_items and at least
      // RT_REGEN_MIN idle lanes (a lane that just missed is idle once it has
      // added its sample below) the refill rule above passes both of its
      // breaks, and next_item grows by the idle count, at least one.  That
      // holds of every pass of the refill loop, whatever its items turn out to
      // be: a pass hands hits to lanes or settles misses, and advances
      // next_item either way, so the refill loop itself ends (next_item
      // reaches n_items, or fewer than RT_REGEN_MIN lanes are left idle).
      // n_items is finite, so after finitely many waiting trips next_item
      // reaches it, `wait` is false and every parked lane is shaded; a trip
      // that does not wait shades every parked lane, and one without parked
      // lanes traces a bounce ray or finds no active lane and leaves: the loop
      // cannot spin.  host/rtx_batch_check.cpp replays it on the CPU.
      const bool wait = __popcll(__ballot(parked)) < kPark && next_item < n_items &&
                        __popcll(__ballot(!ps.active || done)) >= RT_REGEN_MIN(F);
      if (!wait && parked) { // ---- the one shade site
        const uint64_t t1 = STATS ? clk() : 0;
        done = !shade_closest<STATS, F, PC, MS>(S, C, ps, key, pk_closest, pk_best, cnt, lp);
        if (STATS && wave_once()) cnt.cshade += clk() - t1;
        pk_best = -1;
      }
      if (done) {
        atomicAdd(&acc[ps.slot * 3 + 0], ps.T.x);
        atomicAdd(&acc[ps.slot * 3 + 1], ps.T.y);
        atomicAdd(&acc[ps.slot * 3 + 2], ps.T.z);
        ps.active = false;
      }
    } else if (ps.active) {
      if (STATS) n_segments++;
      const uint32_t nv0 = cnt.nodes;
      bool cont = segment<STATS, F, PC, MS>(
          S, C, ps, key, stk, lnodes, cnt, (RT_LDS LeafPool *)&leaf_pool[RT_LEAF_SHARE_F(F) ? wv : 0], lp);
      if (STATS) v_trace = cnt.nodes - nv0;
      if (!cont) {
        atomicAdd(&acc[ps.slot * 3 + 0], ps.T.x);
        atomicAdd(&acc[ps.slot * 3 + 1], ps.T.y);
        atomicAdd(&acc[ps.slot * 3 + 2], ps.T.z);
        ps.active = false;
      }
    }
    if (STATS) { // converged: every lane
      const uint32_t m1 = wave_max(v_trace);
      m_single += m1;
      if (!have_prev) {
        v_prev = v_trace;
        m_prev = m1;
      } else {
        m_pair += wave_max(v_prev + v_trace);
      }
      have_prev = !have_prev;
    }
  }
  if (STATS && have_prev) {
    m_pair += m_prev;
    have_prev = false;
  }
  __builtin_amdgcn_wave_barrier();

  // ---- tile epilogue: one coalesced store per pixel
  {
    // the epilogue's launch fields, camera width / scale and output pointer
    // read afresh (RT_EPI_FRESH_F): once per unit, outside the path loop, so the
    // one-unit instances need not hold them in SGPRs across every path trip
    constexpr bool kEpiFresh = RT_EPI_FRESH_F(F);
    const DCamera Ce = camera_fields<kEpiFresh>(C);
    const DLaunch PE = launch_fields<PC || kEpiFresh>(P);
    int i = x0 + (lane & 7), j = y0 + (lane >> 3);
    // whole units: the frame (pixels outside the image are not written) or
    // the compact tile layout; split units: their chunk's partial sums
    const bool to_parts = !whole;
    const bool compact = to_parts || PE.compact;
    if (compact || (i < Ce.W && j < PE.row_end)) { // tile slots outside the image hold 0
      double sx = acc[lane * 3 + 0], sy = acc[lane * 3 + 1], sz = acc[lane * 3 + 2];
      const bool final_out = !to_parts || PE.parts_final;
      if (final_out && PE.output == RT_OUT_SCALED) {
        sx = Ce.scale * sx;
        sy = Ce.scale * sy;
        sz = Ce.scale * sz;
      }
      double *const ob = out_arg<PC || kEpiFresh>(out);
      const int part = unit - (PE.head_chunks == 1 ? PE.n_head : 0);
      double *o = to_parts ? PE.parts + 3 * ((size_t)part * 64 + lane)
                  : PE.compact ? ob + 3 * ((size_t)order_tile(PE, unit) * 64 + lane)
                               : ob + 3 * ((size_t)(j - PE.row_begin) * Ce.W + i);
      if (final_out && PE.accumulate) {
        o[0] += sx;
        o[1] += sy;
        o[2] += sz;
      } else {
        o[0] = sx;
        o[1] = sy;
        o[2] = sz;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  // the unit's duration into its tile's cost (the shape's dispatch order)
  if constexpr (STATS || COST) {
    if (lane == 0) {
      const DLaunch PT = launch_fields<true>(P);
      if (PT.tile_cost != nullptr)
        atomicAdd(&PT.tile_cost[order_tile(PT, plan_tile(PT, unit))], (unsigned)__builtin_amdgcn_s_memrealtime());
    }
  }
#if RT_UNIT_TIMES
  if (lane == 0 && !STATS && unit < kUnitTimesMax) {
    g_unit_times[2 * unit] = t_unit0;
    g_unit_times[2 * unit + 1] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  if constexpr (!PC) break;
  int next = n_units;
  if (P.unit_ctr != nullptr && lane == 0)
    next = __hip_atomic_fetch_add(P.unit_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unit = P.unit_ctr != nullptr ? __builtin_amdgcn_readfirstlane(__shfl(next, 0)) : n_units;
  } // unit loop
  if (STATS) {
    const uint64_t cyc_loop = clk() - t_start;
    unsigned long long v[RT_N_STATS] = {n_samples, n_segments, cnt.nodes, cnt.spheres,
                                        cnt.quads, cnt.other,  cnt.light, cnt.shade,
                                        lane == 0 ? n_trips : 0u, cnt.wnode, cnt.wleaf, cnt.wshade,
                                        lane == 0 ? cyc_loop : 0u, lane == 0 ? cyc_regen : 0u,
                                        cnt.ctrace, cnt.cmedia, cnt.cshade, cnt.clights,
                                        lane == 0 ? m_single : 0u, lane == 0 ? m_pair : 0u,
                                        cnt.noise, cnt.wnoise, cnt.mbox, cnt.mbox_fb};
    for (int k = 0; k < RT_N_STATS; ++k) {
      unsigned long long x = v[k];
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
      if (lane == 0) atomicAdd(&stats[k], x);
    }
  }
}

using RenderFn = void (*)(DScene, DCamera, DLaunch, double *, unsigned long long *);

// the F_FLAT | F_BVH4 slots reuse the flat instance (rt_path.h canonical_features)
template <bool STATS, unsigned... Fs>
constexpr std::array<RenderFn, sizeof...(Fs)> instance_table(std::integer_sequence<unsigned, Fs...>) {
  return {render_tiles<STATS, canonical_features(Fs)>...};
}

// the persistent instances (RT_PERSIST_F feature sets), blocks of pcw waves
RenderFn persistent_instance(unsigned f, int pcw) {
  if (pcw == kPcWaves)
    return (f & F_BVH4) ? render_tiles<false, F_BVH4, kPcWaves> : render_tiles<false, 0u, kPcWaves>;
  return (f & F_BVH4) ? render_tiles<false, F_BVH4, kWaves> : render_tiles<false, 0u, kWaves>;
}

// the cost-measuring instance (RT_COST_F: the flat world, never persistent);
// the plain BVH worlds' shares measured as well as by the probe (C3 4- / 8-way
// shares +-0.2 %, profiles/r06ai_sim_C3.log), so they have none
RenderFn cost_instance(unsigned f) { return f == F_FLAT ? render_tiles<false, F_FLAT, 0, true> : nullptr; }

// one instance per feature set (F_MEDIA | F_XFORM | F_LIGHTS | F_NOISE | F_FLAT)
const RenderFn *render_table(bool stats) {
  static constexpr auto plain = instance_table<false>(std::make_integer_sequence<unsigned, F_ALL + 1>{});
  static constexpr auto counted = instance_table<true>(std::make_integer_sequence<unsigned, F_ALL + 1>{});
  return stats ? counted.data() : plain.data();
}

// The one-unit render instance of a scene's DScene::features: the table's, or
// for the plain flat world of a diffuse-only materials table (RT_FEAT_DIFFUSE)
// its Lambertian-only twin -- one more kernel, keyed on the material set
// (rt_path.h MatSet).  The STATS and COST instances, the rich flat worlds and
// the BVH worlds have no twin and stay general.  C2: profiles/diffuse_ab.log.
RenderFn render_instance(int features, bool stats) {
  if (!stats && (features & RT_FEAT_DIFFUSE) && (unsigned)(features & F_ALL) == F_FLAT)
    return render_tiles<false, F_FLAT, 0, false, M_DIFFUSE>;
  return render_table(stats)[features & F_ALL];
}

} // namespace

// ---------------------------------------------------------------- launchers
// What the runtime reports about the instance a scene of these features runs:
// the one-unit instance (pc_waves 0), or the persistent instance in blocks of
// pc_waves waves (RT_PERSIST_F feature sets) -- the inputs of the residency
// plan (rt_lds_plan.h).
extern "C" hipError_t rtk_instance_attrs(int features, int pc_waves, KernelAttrs *attrs) {
  const unsigned f = (unsigned)(features & F_ALL);
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(
      &a, reinterpret_cast<const void *>(pc_waves ? persistent_instance(f, pc_waves) : render_instance(features, false)));
  if (e != hipSuccess) return e;
  attrs->num_regs = a.numRegs;
  attrs->static_lds = (int32_t)a.sharedSizeBytes;
  return hipSuccess;
}

// Lets a persistent instance's blocks use more than 64 KB of dynamic LDS: set
// once per device and function, to the most any scene's plan can ask for (the
// CU's LDS less the static part), so scenes of different staged sizes used
// from different host threads never lower it between another launch's check
// and its dispatch.
static hipError_t allow_cu_lds(RenderFn fn) {
  static std::mutex mu;
  static std::set<std::pair<int, const void *>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const void *f = reinterpret_cast<const void *>(fn);
  std::lock_guard<std::mutex> g(mu);
  if (done.count({dev, f})) return hipSuccess;
  hipFuncAttributes a;
  e = hipFuncGetAttributes(&a, f);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsPerCu - a.sharedSizeBytes));
  if (e == hipSuccess) done.insert({dev, f});
  return e;
}

extern "C" hipError_t rtk_launch_render(const DScene *S, const DCamera *C, const DLaunch *P,
                                        double *out, unsigned long long *stats,
                                        hipStream_t stream) {
  const int64_t units = plan_units(*P);
  const int bw = block_waves((unsigned)S->features);
  int blocks = (int)((units + bw - 1) / bw);
  if (blocks == 0) return hipSuccess;
  RenderFn fn = render_instance(S->features, stats != nullptr);
  // a launch that measures its tiles' costs (rt_api.cpp: the first tile-subset
  // launch of a shape in the flat world)
  const bool cost = stats == nullptr && P->tile_cost != nullptr;
  if (cost) {
    fn = cost_instance((unsigned)(S->features & F_ALL));
    if (fn == nullptr) return hipErrorInvalidValue;
  }
  size_t lds = lds_bytes(S->features, S->stack_depth, S->n_lds_nodes);
  int launch_waves = bw;
  DLaunch Q = *P;
  const unsigned f = (unsigned)(S->features & F_ALL);
  if (RT_PERSIST_F(f) && stats == nullptr && Q.unit_ctr != nullptr && Q.grid_cap > 0 &&
      S->pc_waves > 0 && units > (int64_t)Q.grid_cap * S->pc_waves) {
    // persistent: the resident blocks' waves take units [0, grid_cap * pc_waves)
    // statically, the rest from the counter
    fn = persistent_instance(f, S->pc_waves);
    blocks = Q.grid_cap;
    launch_waves = S->pc_waves;
    lds = lds_bytes_pc(S->features, S->pc_waves, S->stack_depth, S->n_lds_nodes_pc, S->lds_items_pc, S->lds_spheres_pc);
    hipError_t e = allow_cu_lds(fn);
    if (e != hipSuccess) return e;
    e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(Q.unit_ctr), blocks * S->pc_waves, 1, stream);
    if (e != hipSuccess) return e;
  } else {
    Q.unit_ctr = nullptr; // every unit has its own wave
  }
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * launch_waves), lds, stream, *S, *C, Q, out, stats);
  return hipGetLastError();
}

