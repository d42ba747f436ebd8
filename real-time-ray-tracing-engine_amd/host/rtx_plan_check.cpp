// rtx_plan_check — host-only check of the work-unit plans (csrc/rt_plan.h,
// csrc/rt_plan.cpp; no HIP).
//   rtx_plan_check          sweeps launches, devices and tunings and checks the
//                           unit arithmetic's invariants on every plan the
//                           planners return; exit 1 at the first violation
//   rtx_plan_check --table  prints the plans of the pinned cases, one per line
//                           (tests/test_plan.py compares them with its table)
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

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

} // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--table")) return table();
  if (argc != 1) {
    std::fprintf(stderr, "usage: rtx_plan_check [--table]\n");
    return 2;
  }
  return sweep();
}
