// rtx_plan_check — host-only check of the work-unit plans (csrc/rt_plan.h,
// csrc/rt_plan.cpp) and of the LDS residency plan (csrc/rt_lds_plan.h,
// csrc/rt_lds_plan.cpp); no HIP.
//   rtx_plan_check          sweeps launches, devices and tunings and checks the
//                           unit arithmetic's invariants on every plan the
//                           planners return; then sweeps kernel attributes,
//                           scene sizes and tunings and checks the residency
//                           plans' invariants; exit 1 at the first violation
//   rtx_plan_check --table  prints the plans of the pinned cases, one per line
//                           (tests/test_plan.py compares them with its table)
//   rtx_plan_check --lds-table  the same for the residency plans
//                           (tests/test_lds_plan.py)
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../csrc/rt_lds_plan.h"
#include "../csrc/rt_plan.h"

namespace {

// the plan-relevant part of rtx::launch_geometry: strata [3, 3 + strata) of
// tiles first + k * stride of a W x H frame
DLaunch make_launch(int W, int H, int strata, int first = 0, int stride = 1, int compact = 0) {
  DLaunch L;
  std::memset(&L, 0, sizeof L);
  L.row_end = H;
  L.sample_begin = 3;
  L.sample_count = strata;
  L.tiles_x = (W + 7) / 8;
  L.tiles_y = (H + 7) / 8;
  const int64_t n_tiles = (int64_t)L.tiles_x * L.tiles_y;
  L.tile_first = first;
  L.tile_stride = stride;
  L.n_local_tiles = (int32_t)(n_tiles > first ? (n_tiles - first + stride - 1) / stride : 0);
  L.compact = compact;
  apply_plan(L, whole_plan(L.n_local_tiles), nullptr, 0);
  return L;
}

#define REQUIRE(cond)                                                                              \
  do {                                                                                             \
    if (!(cond)) {                                                                                 \
      why = std::string(#cond) + " at unit " + std::to_string(u);                                  \
      return false;                                                                                \
    }                                                                                              \
  } while (0)

// plan_unit over [0, units) covers every (plan tile, stratum) exactly once, in
// consecutive non-empty units per tile; chunk units' partial records are a
// bijection onto [0, parts), at the tile's first record + the chunk index;
// whole units have none.
bool check_units(const DLaunch &L, std::string &why) {
  const int64_t units = plan_units(L), parts = plan_parts(L);
  const int n = L.n_local_tiles, first_chunked = plan_first_chunked(L);
  std::vector<int> next_s(n, L.sample_begin), chunk(n, 0);
  std::vector<char> seen(parts, 0);
  int64_t u = 0, n_seen = 0;
  REQUIRE(units <= 0x7FFFFFFF && parts >= 0);
  int prev = -1;
  for (; u < units; ++u) {
    const PlanUnit p = plan_unit(L, (int)u);
    REQUIRE(p.tile >= 0 && p.tile < n);
    REQUIRE(p.s_count >= 1);
    REQUIRE(p.s_first == next_s[p.tile]);
    REQUIRE(p.tile == prev || chunk[p.tile] == 0); // a tile's units are consecutive
    REQUIRE(p.whole == (p.tile < first_chunked));
    if (p.whole) {
      REQUIRE(p.part == -1 && p.s_count == L.sample_count);
    } else {
      REQUIRE(p.part >= 0 && p.part < parts && !seen[p.part]);
      REQUIRE(p.part == plan_tile_part0(L, p.tile) + chunk[p.tile]);
      seen[p.part] = 1;
      ++n_seen;
    }
    next_s[p.tile] += p.s_count;
    ++chunk[p.tile];
    prev = p.tile;
  }
  REQUIRE(n_seen == parts);
  for (int k = 0; k < n; ++k) {
    u = k; // reported as the tile
    REQUIRE(next_s[k] == L.sample_begin + L.sample_count);
    REQUIRE(chunk[k] == plan_tile_chunks(L, k));
  }
  return true;
}

// the shard plans of all n shards of a frame plan partition its head and tail:
// local tile j of shard k (global tile k + j * n) is a head tile exactly when
// its global index is below the frame plan's n_head
bool check_shards(UnitPlan fp, int64_t n_tiles, int n, std::string &why) {
  int64_t u = 0, heads = 0;
  for (int k = 0; k < n; ++k) {
    u = k; // reported as the shard
    const int n_local = (int)(n_tiles > k ? (n_tiles - k + n - 1) / n : 0);
    const UnitPlan sp = shard_plan(fp, k, n, n_local);
    REQUIRE(sp.head_chunks == fp.head_chunks && sp.n_chunks == fp.n_chunks);
    REQUIRE(sp.n_head >= 0 && sp.n_head <= n_local);
    REQUIRE(sp.n_head == 0 || k + (int64_t)(sp.n_head - 1) * n < fp.n_head);
    REQUIRE(sp.n_head == n_local || k + (int64_t)sp.n_head * n >= fp.n_head);
    heads += sp.n_head;
  }
  REQUIRE(heads == fp.n_head);
  return true;
}

struct Dev {
  const char *name;
  PlanDevice d;
};
// 1, 64, 3072 and 4096 wave slots, without and with a persistent instance
// (whose residency pc_grid x pc_waves is then the slot count the planners use)
const Dev kDevs[] = {
    {"1", {1, 0, 0}},          {"1p", {4, 1, 1}},
    {"64", {64, 0, 0}},        {"64p", {48, 4, 16}},
    {"3072", {3072, 0, 0}},    {"3072p", {4096, 192, 16}},
    {"4096", {4096, 0, 0}},    {"4096p", {4096, 256, 16}},
};

struct Tune {
  const char *name;
  rt_tuning t;
};
rt_tuning tuning(int chunk_target, int head_strata, int tail_split, int no_uniform_tail, double tail_tiles,
                 int sub_head_strata = 0, int sub_tail_split = 0, int sub_tail_permille = 0) {
  rt_tuning t;
  std::memset(&t, 0, sizeof t);
  t.chunk_target = chunk_target;
  t.head_strata = head_strata;
  t.tail_split = tail_split;
  t.no_uniform_tail = no_uniform_tail;
  t.tail_tiles = tail_tiles;
  t.sub_head_strata = sub_head_strata;
  t.sub_tail_split = sub_tail_split;
  t.sub_tail_permille = sub_tail_permille;
  return t;
}
// every plan field at zero (default), negative, and the values the GPU tests pass
const Tune kTunes[] = {
    {"default", tuning(0, 0, 0, 0, 0.0)},
    {"chunk_target=-1", tuning(-1, 0, 0, 0, 0.0)},                        // test_c5, test_dist, test_abi
    {"chunk_target=7", tuning(7, 0, 0, 0, 0.0)},
    {"head_strata=-1", tuning(0, -1, 0, 0, 0.0)},
    {"tail_split=-1", tuning(0, 0, -1, 0, 0.0)},
    {"tail_tiles=-1", tuning(0, 0, 0, 0, -1.0)},                          // test_multi
    {"tail_tiles=0.25", tuning(-1, 0, 0, 0, 0.25)},                       // test_abi
    {"no_uniform_tail", tuning(0, 0, 0, 1, 0.0)},
    {"head64 tail1 split4", tuning(0, 64, 4, 0, 1.0)},                    // test_tile_order
    {"head_strata=32 tail_split=3", tuning(0, 32, 3, 0, 0.0)},
    {"sub 8/2/2", tuning(0, 0, 0, 0, 0.0, 8, 2, 2)},                      // test_subset_auto
    {"sub_tail_permille=-1", tuning(0, 0, 0, 0, 0.0, 0, 0, -1)},          // test_subset_auto
    {"sub 64/0/3", tuning(0, 0, 0, 0, 0.0, 64, 0, 3)},                    // test_subset_auto
    {"sub_head_strata=-1 sub_tail_split=-1", tuning(0, 0, 0, 0, 0.0, -1, -1, 0)},
};

const int kSizes[][2] = {{1, 1}, {8, 8}, {9, 17}, {96, 54}, {160, 90}, {320, 180}, {1920, 1080}, {3840, 2160}};
const int kStrata[] = {1, 2, 63, 64, 65, 256, 1024, 4096};
const int kStrides[] = {1, 3, 8};

int sweep() {
  // the unit arithmetic depends on the launch's tiles and strata and the plan
  // only: each distinct combination is walked once
  std::set<std::tuple<int, int, int, int, int>> walked;
  long n_plans = 0;
  std::string why;
  auto fail = [&](const char *what, const DLaunch &L, const Dev &dv, const Tune &tu, UnitPlan p) {
    std::fprintf(stderr, "rtx_plan_check: %s: %s\n  %d x %d tiles, first %d stride %d, %d strata, device %s, "
                         "tuning %s: plan %d, %d, %d\n",
                 what, why.c_str(), L.tiles_x, L.tiles_y, L.tile_first, L.tile_stride, L.sample_count, dv.name,
                 tu.name, p.n_head, p.head_chunks, p.n_chunks);
    return 1;
  };
  auto units_ok = [&](DLaunch L, UnitPlan p) {
    ++n_plans;
    if (!walked.insert(std::make_tuple(L.n_local_tiles, L.sample_count, p.n_head, p.head_chunks, p.n_chunks)).second)
      return true;
    apply_plan(L, p, nullptr, 0);
    return check_units(L, why);
  };
  for (const auto &wh : kSizes)
    for (int strata : kStrata)
      for (const Dev &dv : kDevs)
        for (const Tune &tu : kTunes) {
          const DLaunch F = make_launch(wh[0], wh[1], strata);
          const UnitPlan fp = frame_plan(dv.d, tu.t, F);
          if (!units_ok(F, fp)) return fail("frame plan", F, dv, tu, fp);
          if (!units_ok(F, chunks_plan(7, strata))) return fail("chunks plan", F, dv, tu, chunks_plan(7, strata));
          for (int stride : kStrides) {
            if (!check_shards(fp, (int64_t)F.tiles_x * F.tiles_y, stride, why))
              return fail("shard plans", F, dv, tu, fp);
            for (int first : {0, stride - 1}) {
              const DLaunch S = make_launch(wh[0], wh[1], strata, first, stride, 1);
              const UnitPlan sp = subset_plan(dv.d, tu.t, S);
              if (!units_ok(S, sp)) return fail("subset plan", S, dv, tu, sp);
              const UnitPlan sh = shard_plan(fp, first, stride, S.n_local_tiles);
              if (!units_ok(S, sh)) return fail("shard plan", S, dv, tu, sh);
            }
          }
        }
  std::printf("rtx_plan_check: %ld plans, %zu distinct unit layouts walked: ok\n", n_plans, walked.size());
  return 0;
}

void row(const char *name, UnitPlan p) { std::printf("%s: %d, %d, %d\n", name, p.n_head, p.head_chunks, p.n_chunks); }

int table() {
  const PlanDevice p4096{4096, 256, 16}, d3072{3072, 0, 0}, d64{64, 0, 0};
  const rt_tuning def = kTunes[0].t;
  auto frame = [&](const char *name, int W, int H, int strata, PlanDevice d, const rt_tuning &t) {
    row(name, frame_plan(d, t, make_launch(W, H, strata)));
  };
  auto subset = [&](const char *name, int W, int H, int strata, int first, int stride, PlanDevice d,
                    const rt_tuning &t) { row(name, subset_plan(d, t, make_launch(W, H, strata, first, stride, 1))); };
  // frame_plan: every return path
  frame("frame 1080p s64 4096p", 1920, 1080, 64, p4096, def);
  frame("frame 1080p s64 3072", 1920, 1080, 64, d3072, def);
  frame("frame 1080p s256 4096p", 1920, 1080, 256, p4096, def);
  frame("frame 1080p s1024 3072", 1920, 1080, 1024, d3072, def);
  frame("frame 1080p s1024 4096p", 1920, 1080, 1024, p4096, def);
  frame("frame 4K s4096 4096p", 3840, 2160, 4096, p4096, def);
  frame("frame 4K s4096 3072", 3840, 2160, 4096, d3072, def);
  frame("frame 96x54 s64 4096p", 96, 54, 64, p4096, def);
  frame("frame 96x54 s64 3072", 96, 54, 64, d3072, def);
  frame("frame 1080p s1 4096p", 1920, 1080, 1, p4096, def);
  frame("frame 96x54 s1 3072", 96, 54, 1, d3072, def);
  frame("frame 1080p s2 4096p", 1920, 1080, 2, p4096, def);
  frame("frame 1080p s4 4096p", 1920, 1080, 4, p4096, def);
  frame("frame 1080p s64 no device", 1920, 1080, 64, PlanDevice{0, 0, 0}, def);
  frame("frame 160x90 s64 64 (uniform + tail)", 160, 90, 64, d64, def);
  frame("frame 160x90 s64 64 no_uniform_tail", 160, 90, 64, d64, kTunes[7].t);
  frame("frame 320x180 s64 64", 320, 180, 64, d64, def);
  frame("frame 160x90 s16 64p grid", 160, 90, 16, kDevs[3].d, def);
  row("frame compact 1080p s64 4096p", frame_plan(p4096, def, make_launch(1920, 1080, 64, 0, 1, 1)));
  row("frame strided 1080p s64 4096p", frame_plan(p4096, def, make_launch(1920, 1080, 64, 1, 2, 0)));
  frame("frame 1080p s64 4096p chunk_target=-1", 1920, 1080, 64, p4096, kTunes[1].t);
  frame("frame 1080p s64 4096p chunk_target=7", 1920, 1080, 64, p4096, kTunes[2].t);
  frame("frame 96x54 s64 4096p chunk_target=7", 96, 54, 64, p4096, kTunes[2].t);
  frame("frame 1080p s64 4096p tail_tiles=-1", 1920, 1080, 64, p4096, kTunes[5].t);
  frame("frame 1080p s256 4096p tail_tiles=-1", 1920, 1080, 256, p4096, kTunes[5].t);
  frame("frame 320x180 s64 4096p head64 tail1 split4", 320, 180, 64, p4096, kTunes[8].t);
  frame("frame 320x180 s64 64 head64 tail1 split4", 320, 180, 64, d64, kTunes[8].t);
  frame("frame 1080p s256 4096p head32 split3", 1920, 1080, 256, p4096, kTunes[9].t);
  frame("frame 1080p s1024 4096p head32 split3", 1920, 1080, 1024, p4096, kTunes[9].t);
  // subset_plan: every return path
  subset("subset (1,8) 1080p s64 4096p", 1920, 1080, 64, 1, 8, p4096, def);
  subset("subset (1,8) 1080p s256 4096p", 1920, 1080, 256, 1, 8, p4096, def);
  subset("subset (1,8) 1080p s1024 4096p", 1920, 1080, 1024, 1, 8, p4096, def);
  subset("subset (1,8) 1080p s64 3072", 1920, 1080, 64, 1, 8, d3072, def);
  subset("subset (1,8) 4K s4096 3072", 3840, 2160, 4096, 1, 8, d3072, def);
  subset("subset (1,8) 96x54 s64 4096p", 96, 54, 64, 1, 8, p4096, def);
  subset("subset (1,8) 96x54 s64 3072", 96, 54, 64, 1, 8, d3072, def);
  subset("subset (1,3) 96x54 s64 4096p", 96, 54, 64, 1, 3, p4096, def);
  subset("subset (1,3) 96x54 s64 4096p sub 8/2/2", 96, 54, 64, 1, 3, p4096, kTunes[10].t);
  subset("subset (1,3) 96x54 s64 4096p sub_tail_permille=-1", 96, 54, 64, 1, 3, p4096, kTunes[11].t);
  subset("subset (1,3) 96x54 s64 4096p sub 64/0/3", 96, 54, 64, 1, 3, p4096, kTunes[12].t);
  subset("subset (0,1) 96x54 s64 4096p sub 64/0/3", 96, 54, 64, 0, 1, p4096, kTunes[12].t);
  subset("subset (0,1) 1080p s4 4096p (frame plan)", 1920, 1080, 4, 0, 1, p4096, def);
  subset("subset (0,1) 1080p s64 4096p (frame plan)", 1920, 1080, 64, 0, 1, p4096, def);
  subset("subset (1,3) 320x180 s64 64 (frame plan)", 320, 180, 64, 1, 3, d64, def);
  subset("subset (1,8) 1080p s1 4096p", 1920, 1080, 1, 1, 8, p4096, def);
  subset("subset (5,8) 16x9 s4 4096p (no tiles)", 16, 9, 4, 5, 8, p4096, def);
  subset("subset (1,8) 1080p s64 no device", 1920, 1080, 64, 1, 8, PlanDevice{0, 0, 0}, def);
  // the inline planners
  row("chunks_plan(4, 64)", chunks_plan(4, 64));
  row("chunks_plan(100, 64)", chunks_plan(100, 64));
  row("chunks_plan(3, 0)", chunks_plan(3, 0));
  row("shard_plan({31376,1,8}, 3, 8, 4050)", shard_plan(UnitPlan{31376, 1, 8}, 3, 8, 4050));
  row("shard_plan({5,2,16}, 7, 8, 4)", shard_plan(UnitPlan{5, 2, 16}, 7, 8, 4));
  row("whole_plan(4050)", whole_plan(4050));
  return 0;
}

// ---- the LDS residency plan (csrc/rt_lds_plan.h)

rt_tuning lds_tuning(int lds_cap, int lds_nodes, int lds_nodes_pc, int no_lds_prims, int pc_waves,
                     int no_lds_perlin) {
  rt_tuning t;
  std::memset(&t, 0, sizeof t);
  t.lds_cap = lds_cap;
  t.lds_nodes = lds_nodes;
  t.lds_nodes_pc = lds_nodes_pc;
  t.no_lds_prims = no_lds_prims;
  t.pc_waves = pc_waves;
  t.no_lds_perlin = no_lds_perlin;
  return t;
}
// every field the plan reads at zero (default), positive and negative where
// that means something; the values the GPU tests pass
const Tune kLdsTunes[] = {
    {"default", lds_tuning(0, 0, 0, 0, 0, 0)},
    {"lds_cap=4096", lds_tuning(4096, 0, 0, 0, 0, 0)},      // test_bvh4
    {"lds_cap=30000", lds_tuning(30000, 0, 0, 0, 0, 0)},
    {"lds_cap=100000", lds_tuning(100000, 0, 0, 0, 0, 0)},  // above 64 KB: no effect
    {"lds_nodes=100", lds_tuning(0, 100, 0, 0, 0, 0)},
    {"lds_nodes=-1", lds_tuning(0, -1, 0, 0, 0, 0)},        // test_hit_identity
    {"lds_nodes_pc=100", lds_tuning(0, 0, 100, 0, 0, 0)},
    {"lds_nodes_pc=-1", lds_tuning(0, 0, -1, 0, 0, 0)},     // test_persistent
    {"no_lds_prims", lds_tuning(0, 0, 0, 1, 0, 0)},         // test_persistent
    {"pc_waves=4", lds_tuning(0, 0, 0, 0, 4, 0)},           // test_persistent
    {"no_lds_perlin", lds_tuning(0, 0, 0, 0, 0, 1)},        // test_lds_perlin
    {"lds_cap=4096 lds_nodes=100 pc_waves=4", lds_tuning(4096, 100, 0, 0, 4, 0)},
};

#define LDS_REQUIRE(cond)                                                                          \
  do {                                                                                             \
    if (!(cond)) {                                                                                 \
      why = #cond;                                                                                 \
      return false;                                                                                \
    }                                                                                              \
  } while (0)

// What must hold of every residency plan: nothing staged beyond the LDS the
// occupancy target leaves, and the dynamic LDS the launcher requests
// (lds_bytes / lds_bytes_pc of the DScene fields) is what the planner budgeted.
bool check_lds_plan(const LdsPlanInput &in, const SceneLdsPlan &p, std::string &why) {
  const RtkLdsPlan &r = p.render;
  const int64_t node_b = RT_LDS_NODE_BYTES(in.features);
  LDS_REQUIRE(r.waves_per_simd >= 1 && r.waves_per_simd <= 8);
  LDS_REQUIRE(r.block_budget > 0 && (size_t)r.block_budget <= kLdsPerBlock);
  LDS_REQUIRE(r.stack_fits == (r.fixed_bytes <= r.block_budget));
  LDS_REQUIRE((size_t)r.fixed_bytes == in.render.static_lds + lds_bytes(in.features, in.stack_depth, 0));
  if (p.outcome == LDS_UNSUPPORTED) {
    LDS_REQUIRE(!r.stack_fits && (size_t)r.fixed_bytes > kLdsPerBlock);
    return true;
  }
  LDS_REQUIRE((p.outcome == LDS_OK) == (r.stack_fits != 0));
  LDS_REQUIRE((size_t)r.fixed_bytes <= kLdsPerBlock);
  LDS_REQUIRE(p.n_lds_nodes >= 0 && p.n_lds_nodes <= in.n_nodes);
  const size_t launch = in.render.static_lds + lds_bytes(in.features, in.stack_depth, p.n_lds_nodes);
  LDS_REQUIRE(launch == (size_t)(r.fixed_bytes + p.n_lds_nodes * node_b));
  if (r.stack_fits) LDS_REQUIRE(launch <= (size_t)r.block_budget);
  else LDS_REQUIRE(p.n_lds_nodes == 0);
  LDS_REQUIRE(p.wave_slots > 0 && p.wave_slots % in.cus == 0);
  // as many blocks as the slots count fit the CU's LDS
  const int bw = block_waves((unsigned)in.features);
  LDS_REQUIRE(p.wave_slots / in.cus % bw == 0 && (size_t)(p.wave_slots / in.cus / bw) * launch <= kLdsPerCu);
  LDS_REQUIRE((p.n_lds_nodes_pc == -1) == (p.pc_waves == 0));
  if (p.pc_waves == 0) {
    LDS_REQUIRE(p.pc_grid == 0 && p.lds_items_pc == 0 && p.lds_spheres_pc == 0);
  } else {
    LDS_REQUIRE(p.pc_waves == kPcWaves || p.pc_waves == kWaves);
    LDS_REQUIRE(RT_PERSIST_F((unsigned)in.features & 63u));
    LDS_REQUIRE(p.pc_grid > 0 && p.pc_grid % in.cus == 0);
    LDS_REQUIRE(p.n_lds_nodes_pc >= 0 && p.n_lds_nodes_pc <= in.n_nodes);
    const KernelAttrs a = p.pc_waves == kPcWaves ? in.pc16 : in.pc4;
    const size_t launch_pc = a.static_lds + lds_bytes_pc(in.features, p.pc_waves, in.stack_depth, p.n_lds_nodes_pc,
                                                          p.lds_items_pc, p.lds_spheres_pc);
    LDS_REQUIRE(launch_pc <= kLdsPerCu / (p.pc_grid / in.cus));
    LDS_REQUIRE(p.pc_grid / in.cus * p.pc_waves <= 4 * waves_per_simd(a.num_regs) || p.pc_grid == in.cus);
    if (p.lds_items_pc || p.lds_spheres_pc)
      LDS_REQUIRE(p.n_lds_nodes_pc == in.n_nodes && p.lds_items_pc == in.n_items && p.lds_spheres_pc == in.n_spheres);
  }
  LDS_REQUIRE(p.lds_perlin == 0 || (p.lds_perlin == 1 && (in.features & RT_FEAT_NOISE) && in.n_perlin == 1));
  return true;
}

int lds_sweep() {
  const int kRegs[] = {8, 96, 120, 128, 129, 168, 256, 512};
  const int kStatic[] = {0, 6144, 24576, 65536};
  const int kDepths[] = {1, 13, 21, RT_STACK_DEPTH, 46, RT_STACK_DEPTH4};
  const int kNodes[] = {0, 485, 2000, 100000};
  const int kPrims[][2] = {{0, 0}, {486, 486}, {486, 0}, {4000, 4000}};
  long n_plans = 0;
  std::string why;
  for (int regs : kRegs)
    for (int slds : kStatic)
      for (int depth : kDepths)
        for (int nodes : kNodes)
          for (const auto &prims : kPrims)
            for (int features = 0; features < 64; ++features)
              for (int cus : {1, 256})
                for (const Tune &tu : kLdsTunes) {
                  LdsPlanInput in{};
                  in.render = KernelAttrs{regs, slds};
                  // the persistent instances: the 16-wave form with four times the one-unit
                  // block's static LDS, as the real ones
                  in.pc16 = KernelAttrs{regs, 4 * slds};
                  in.pc4 = KernelAttrs{regs, slds};
                  in.cus = cus;
                  in.features = features;
                  in.stack_depth = depth;
                  in.n_nodes = nodes;
                  in.n_items = prims[0];
                  in.n_spheres = prims[1];
                  in.n_perlin = nodes % 3; // 0, 2, 2, 1
                  const SceneLdsPlan p = plan_scene_lds(in, tu.t);
                  ++n_plans;
                  if (!check_lds_plan(in, p, why)) {
                    std::fprintf(stderr,
                                 "rtx_plan_check: residency plan: %s\n  %d regs, %d B static, features %d, stack %d, "
                                 "%d nodes, %d items, %d spheres, %d CUs, tuning %s\n",
                                 why.c_str(), regs, slds, features, depth, nodes, prims[0], prims[1], cus, tu.name);
                    return 1;
                  }
                }
  std::printf("rtx_plan_check: %ld residency plans: ok\n", n_plans);
  return 0;
}

// The instances' register counts and static LDS in the gfx950 build (`make
// asm`: build/asm/resource.txt "VGPRs" and "LDS Size [bytes/block]";
// tools/regs.py prints the former): what hipFuncGetAttributes reports as
// numRegs and sharedSizeBytes.
const KernelAttrs kF0{120, 6144}, kF4{150, 6144}, kF5{168, 6144}, kF8{158, 15360}, kF13{168, 15360},
    kF16{128, 1536}, kF32{128, 6144}, kPc16{128, 24576}, kPc4{128, 6144};

void lds_row(const char *name, KernelAttrs render, int features, int stack_depth, int n_nodes, int n_items,
             int n_spheres, int n_perlin, const rt_tuning &t, KernelAttrs pc16 = kPc16, KernelAttrs pc4 = kPc4) {
  LdsPlanInput in{};
  in.render = render;
  in.pc16 = pc16;
  in.pc4 = pc4;
  in.cus = 256;
  in.features = features;
  in.stack_depth = stack_depth;
  in.n_nodes = n_nodes;
  in.n_items = n_items;
  in.n_spheres = n_spheres;
  in.n_perlin = n_perlin;
  const SceneLdsPlan p = plan_scene_lds(in, t);
  const RtkLdsPlan &r = p.render;
  std::printf("%s: %s; block %d waves/SIMD, %d of %d B, room for %d nodes, %d waves/CU", name,
              p.outcome == LDS_OK ? "ok" : p.outcome == LDS_STACKS_OVER_SHARE ? "stacks over share" : "unsupported",
              r.waves_per_simd, r.fixed_bytes, r.block_budget, r.n_nodes, r.resident_waves_per_cu);
  if (p.outcome != LDS_UNSUPPORTED)
    std::printf("; %d nodes, %d slots; persistent %d waves x %d: %d nodes, %d items, %d spheres; perlin %d",
                p.n_lds_nodes, p.wave_slots, p.pc_waves, p.pc_grid, p.n_lds_nodes_pc, p.lds_items_pc,
                p.lds_spheres_pc, p.lds_perlin);
  std::printf("\n");
}

int lds_table() {
  const rt_tuning def = kLdsTunes[0].t;
  // C3's shape: everything staged, DESIGN.md §2's byte split (stacks 53,248 +
  // sums 24,576 + nodes 38,800 + items 15,552 + spheres 31,104 of 163,840 B)
  lds_row("C3 485 nodes 486 items 486 spheres", kF0, 0, 13, 485, 486, 486, 0, def);
  lds_row("tree over the free bytes: prefix, no prims", kF0, 0, 20, 5000, 5001, 5001, 0, def);
  lds_row("tree fits, prims do not", kF0, 0, 13, 485, 3000, 3000, 0, def);
  lds_row("tree and items fit, no spheres", kF0, 0, 13, 485, 486, 0, 0, def);
  lds_row("empty world", kF0, 0, 1, 0, 0, 0, 0, def);
  lds_row("4-wide 1000 nodes", kF32, 32, 22, 1000, 4096, 4096, 0, def);
  lds_row("4-wide depth 34: 16-wave stacks fill the CU", kF32, 32, 34, 1000, 4096, 4096, 0, def);
  lds_row("4-wide depth 34, 32 KB static at 16 waves: 4-wave blocks", kF32, 32, 34, 1000, 4096, 4096, 0, def,
          KernelAttrs{128, 32768});
  lds_row("4-wide depth 37: no shape fits, stacks over share", kF32, 32, 37, 1000, 4096, 4096, 0, def);
  lds_row("persistent instance at 168 registers: still one 16-wave block per CU", kF0, 0, 13, 485, 486, 486, 0, def,
          KernelAttrs{168, 24576}, KernelAttrs{168, 6144});
  lds_row("rich set (media + lights) at 3 waves/SIMD", kF5, 5, 10, 100, 60, 10, 0, def);
  lds_row("flat world: one-wave blocks", kF16, 16, 1, 0, 8, 8, 0, def);
  lds_row("lds_cap below the fixed bytes", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[1].t);
  lds_row("lds_cap=30000", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[2].t);
  lds_row("4-wide depth 46: stacks over share, 3 blocks per CU", kF32, 32, 46, 1000, 4096, 4096, 0, def);
  lds_row("fixed bytes above 64 KB", kF32, 32, 64, 1000, 4096, 4096, 0, def);
  lds_row("lds_nodes=100", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[4].t);
  lds_row("lds_nodes=-1", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[5].t);
  lds_row("lds_cap=4096 lds_nodes=100 pc_waves=4", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[11].t);
  lds_row("lds_nodes_pc=100", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[6].t);
  lds_row("lds_nodes_pc=-1", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[7].t);
  lds_row("no_lds_prims", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[8].t);
  lds_row("pc_waves=4", kF0, 0, 13, 485, 486, 486, 0, kLdsTunes[9].t);
  lds_row("pc_waves=4 small tree", kF0, 0, 8, 85, 86, 86, 0, kLdsTunes[9].t);
  lds_row("noise, one Perlin table", kF8, 8, 10, 100, 101, 101, 1, def);
  lds_row("noise, no_lds_perlin", kF8, 8, 10, 100, 101, 101, 1, kLdsTunes[10].t);
  lds_row("noise, two Perlin tables", kF8, 8, 10, 100, 101, 101, 2, def);
  lds_row("one Perlin table, no noise texture", kF0, 0, 10, 100, 101, 101, 1, def);
  lds_row("C4's set (media, lights, noise)", kF13, 13, 12, 300, 301, 250, 1, def);
  // rt_tuning.extra_features is OR'ed into the instance key before the plan
  lds_row("extra_features=4: the lights instance", kF4, 0 | 4, 13, 485, 486, 486, 0, def);
  const char *const verdicts[] = {"fits", "too deep", "over share"};
  std::printf("collapse 4 levels: %s\n", verdicts[collapse4_verdict(kF32, 0, 4, 0)]);
  std::printf("collapse 11 levels (stack 34): %s\n", verdicts[collapse4_verdict(kF32, 0, 11, 0)]);
  std::printf("collapse 12 levels (stack 37): %s\n", verdicts[collapse4_verdict(kF32, 0, 12, 0)]);
  std::printf("collapse 21 levels (stack 64): %s\n", verdicts[collapse4_verdict(kF32, 0, 21, 0)]);
  std::printf("collapse 22 levels (stack 67): %s\n", verdicts[collapse4_verdict(kF32, 0, 22, 0)]);
  std::printf("collapse 4 levels, lds_cap=4096: %s\n", verdicts[collapse4_verdict(kF32, 0, 4, 4096)]);
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--table")) return table();
  if (argc == 2 && !std::strcmp(argv[1], "--lds-table")) return lds_table();
  if (argc != 1) {
    std::fprintf(stderr, "usage: rtx_plan_check [--table | --lds-table]\n");
    return 2;
  }
  const int rc = sweep();
  return rc ? rc : lds_sweep();
}
