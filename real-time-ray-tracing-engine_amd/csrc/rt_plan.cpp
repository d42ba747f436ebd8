// rt_plan.cpp — the work-unit planners (rt_plan.h): pure integer functions of
// the launch, the device's wave slots and the scene's tuning.  No HIP here:
// host/rtx_plan_check.cpp runs them on the CPU, tests/test_plan.py pins the
// plans of the benchmark shapes.
#include "rt_plan.h"

#include <algorithm>
#include <cmath>

namespace {

// chunk count with no empty chunks
int no_empty(int64_t c, int sample_count) {
  c = std::max<int64_t>(1, std::min<int64_t>(c, sample_count));
  const int64_t cs = (sample_count + c - 1) / c;
  return (int)((sample_count + cs - 1) / cs);
}

} // namespace

// Work units of a frame-layout launch over every tile: the waves
// should end together, so the launch must end on short units, while every
// unit pays a refill drain at its end (its last paths finish while lanes
// idle) and long units pay it less often.
//  * Frames of more than 4 tiles per resident wave (1080p: 7.9 on 4,096 wave
//    slots) whose head plan keeps the partials within 4 frames: head tiles
//    whole (up to 64 strata: written straight into the frame, C2) or in
//    chunks of 128 strata (C3: 2 per tile), and the last `slots` x
//    rt_tuning.tail_tiles (default 0.25) tiles in 8x finer chunks, the units the
//    waves take last (dispatch / counter order), so the launch ends on a
//    short unit (C2 +3.9 %, C3 +1.2 % over the uniform split;
//    profiles/r03f_ab.log).  Whole 256-strata tiles as C3's head: -9 %
//    (r03e_ab.log, r04b_head_strata_ab.log); chunks of 128 strata measure the
//    same as 64 with half the partial writes (r04b).
//  * Otherwise every tile split, ~RTX_CHUNK_TARGET (default 32) units per
//    wave slot (the round-1 rule), the last tiles again in finer chunks.
// rt_tuning.chunk_target < 0: whole tiles only (tests).
UnitPlan frame_plan(const PlanDevice &dev, const rt_tuning &tu, const DLaunch &L) {
  UnitPlan sp = whole_plan(L.n_local_tiles);
  if (L.compact || L.tile_stride != 1 || L.tile_first != 0 || L.sample_count < 2) return sp;
  const int target = tu.chunk_target == 0 ? 32 : tu.chunk_target;
  if (target <= 0 || dev.wave_slots <= 0) return sp;
  const int64_t tiles = (int64_t)L.n_local_tiles, slots = dev.slots();
  // tail tiles per wave slot: a quarter for the head/tail plan since the head
  // tiles are taken most expensive first (tile order; C2 +0.9 %, C3 +0.2 %,
  // profiles/r05x_ab.log), a half after the uniform split (C4 -1.6 % at a
  // quarter)
  const double tail_ht = tu.tail_tiles == 0.0 ? 0.25 : std::max(0.0, tu.tail_tiles);
  const double tail = tu.tail_tiles == 0.0 ? 0.5 : std::max(0.0, tu.tail_tiles);
  // head units: whole tiles up to 64 strata (C2); beyond, chunks of 128
  // strata (C3: 2 per tile -- as fast as 4 chunks of 64, half the partial
  // writes; whole 256-strata tiles -9 %, profiles/r04b_head_strata_ab.log)
  const int head_max = tu.head_strata > 0 ? (int)tu.head_strata : L.sample_count <= 64 ? 64 : 128;
  const int64_t head_chunks = (L.sample_count + head_max - 1) / head_max;
  const int split = tu.tail_split > 0 ? (int)tu.tail_split : 8; // tail chunks per head chunk
  // partial records of a head/tail plan: bounded by 4 frames (a tail of
  // chunked tiles + head chunks); otherwise the uniform split
  const bool bounded = head_chunks == 1 || head_chunks * tiles <= 4 * tiles;
  if (tiles > 4 * slots && tail > 0 && bounded) {
    const int64_t n_tail = std::min<int64_t>(tiles, std::max<int64_t>(1, (int64_t)(tail_ht * slots)));
    sp.head_chunks = no_empty((L.sample_count + head_max - 1) / head_max, L.sample_count);
    sp.n_chunks = no_empty(split * (int64_t)sp.head_chunks, L.sample_count);
    sp.n_head = (int)(tiles - n_tail);
    if (sp.n_chunks <= 1) sp = whole_plan(L.n_local_tiles);
    return sp;
  }
  const int64_t c = ((int64_t)target * slots + tiles - 1) / std::max<int64_t>(1, tiles);
  sp.n_chunks = no_empty(c, L.sample_count);
  if (sp.n_chunks > 1) sp.n_head = 0;
  // ... with the last `slots` x rt_tuning.tail_tiles (default 0.5 here) tiles in `split` times finer
  // chunks when the frame has a tile per wave slot (C4, C5: the uniform
  // units last 15 / 84 ms: C4 +1.7 %, C5 +0.9 %, profiles/r03ae_ab.log;
  // rt_tuning.no_uniform_tail: off, A/B runs)
  if (!tu.no_uniform_tail && sp.n_chunks > 1 && tiles > slots && tail > 0) {
    const int64_t n_tail = std::min<int64_t>(tiles, std::max<int64_t>(1, (int64_t)(tail * slots)));
    const int tc = no_empty(split * (int64_t)sp.n_chunks, L.sample_count);
    if (tc > sp.n_chunks && n_tail < tiles) {
      sp.head_chunks = sp.n_chunks;
      sp.n_chunks = tc;
      sp.n_head = (int)(tiles - n_tail);
    }
  }
  return sp;
}

// Work units of a tile-subset launch that returns its tiles' sums
// (strata_chunks = RT_CHUNKS_AUTO: one rank's share of a tile-sharded frame).
// A share of more than 4 tiles per wave slot takes the frame plan.  A smaller
// one (an 8-way rank of a 1080p frame: 4,050 tiles on 4,096 slots) cannot
// hand whole tiles to the waves -- the slowest tile would be the launch -- so
// every tile is split into head units of `sub_head_strata` strata, and the
// last sub_tail_permille / 1000 x slots tiles into `sub_tail_split` times
// finer chunks, which the waves take last (dispatch / counter order) so the
// launch ends on short units.  Long units drain less often (a unit ends with
// its last paths finishing while lanes idle), short ones balance the end.
// Defaults from 8-way sweeps on one GPU (profiles/r05n_*, r05o_*): head units
// of 16 x sqrt(strata / 64) strata (C2 16, C3 32, C4 64), a tail of an eighth
// of the slots' tiles in halves of those: against every tile in the rank's
// uniform chunks, C2's share -3 to -8 %, C3's -1.5 %, C4's -0.8 % (a quarter
// then; an eighth since tile order, C2 -3.4 %: profiles/r05x_sim_C2.log).
constexpr int kSubTailSplit = 2, kSubTailPermille = 125;
UnitPlan subset_plan(const PlanDevice &dev, const rt_tuning &tu, const DLaunch &L) {
  UnitPlan sp = whole_plan(L.n_local_tiles);
  if (L.sample_count < 2 || L.n_local_tiles < 1 || dev.wave_slots <= 0) return sp;
  const int64_t tiles = (int64_t)L.n_local_tiles, slots = dev.slots();
  if (tiles > 4 * slots) {
    DLaunch F = L;
    F.compact = 0;
    F.tile_first = 0;
    F.tile_stride = 1;
    return frame_plan(dev, tu, F);
  }
  const int head = tu.sub_head_strata > 0
                       ? tu.sub_head_strata
                       : std::max(1, (int)std::lround(16.0 * std::sqrt(L.sample_count / 64.0)));
  const int split = tu.sub_tail_split > 0 ? tu.sub_tail_split : kSubTailSplit;
  const int permille = tu.sub_tail_permille != 0 ? tu.sub_tail_permille : kSubTailPermille;
  sp.head_chunks = no_empty((L.sample_count + head - 1) / head, L.sample_count);
  sp.n_chunks = sp.head_chunks;
  sp.n_head = (int)tiles;
  if (permille > 0) {
    const int64_t n_tail = std::min<int64_t>(tiles, std::max<int64_t>(1, slots * permille / 1000));
    const int tc = no_empty((int64_t)split * sp.head_chunks, L.sample_count);
    if (tc > sp.head_chunks) {
      sp.n_chunks = tc;
      sp.n_head = (int)(tiles - n_tail);
    }
  }
  if (sp.n_head == 0) sp.head_chunks = 1; // every tile a tail tile
  return sp;
}

UnitPlan shard_plan(UnitPlan frame, int first, int stride, int n_local) {
  frame.n_head = frame.n_head > first ? std::min(n_local, (frame.n_head - first + stride - 1) / stride) : 0;
  return frame;
}

UnitPlan chunks_plan(int strata_chunks, int sample_count) {
  return UnitPlan{0, 1, std::max(1, std::min(strata_chunks, std::max(1, sample_count)))};
}
