// rt_plan.h — the work-unit plan of a launch, defined once.
//
// A work unit is a (plan tile, stratum chunk) pair, one wavefront's work.  A
// plan (UnitPlan) says which tiles are head tiles, how many chunks a head tile
// and a tail tile get; with the launch's tile and stratum counts that fixes
// every unit's strata and where its partial sums go (DLaunch, rt_layout.h) --
// and so the fp64 summation grouping of every pixel, on which the bit-identity
// of one GPU against N, ordered against unordered dispatch and persistent
// against one-unit waves rests.  This header holds the unit arithmetic (host
// and device) and apply_plan, the only writer of a DLaunch's plan fields;
// rt_plan.cpp holds the planners (plain C++, no HIP: host/rtx_plan_check.cpp
// runs them on the CPU).  render_tiles (rt_kernel.hip) keeps its own copy of
// plan_unit's decode, for its register allocation's sake.
#ifndef RT_PLAN_H
#define RT_PLAN_H
#include <stdint.h>

#include "../../include/rt_api.h"
#include "rt_layout.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_PLAN_HD __host__ __device__
#else
#define RT_PLAN_HD
#endif

struct UnitPlan {
  int32_t n_head, head_chunks, n_chunks; // head tiles, their chunks; the tail tiles' chunks
};
inline UnitPlan whole_plan(int n_local) { return UnitPlan{n_local, 1, 1}; } // one unit per tile
inline UnitPlan plan_of(const DLaunch &L) { return UnitPlan{L.n_head, L.head_chunks, L.n_chunks}; }

// The only code that writes a launch's plan fields.  parts: where chunk units
// write their partial sums; parts_final: they are the caller's output.
inline void apply_plan(DLaunch &L, UnitPlan p, double *parts, int parts_final) {
  L.n_head = p.n_head;
  L.head_chunks = p.head_chunks;
  L.n_chunks = p.n_chunks;
  L.chunk_strata = (L.sample_count + p.n_chunks - 1) / p.n_chunks;
  L.parts = parts;
  L.parts_final = parts_final;
}

RT_PLAN_HD inline int64_t plan_units(const DLaunch &L) {
  return (int64_t)L.n_head * L.head_chunks + (int64_t)(L.n_local_tiles - L.n_head) * L.n_chunks;
}
// first plan tile whose units are chunks (the tiles before it are whole units)
RT_PLAN_HD inline int plan_first_chunked(const DLaunch &L) { return L.head_chunks > 1 ? 0 : L.n_head; }
// chunk partial records [64][3] of the launch
RT_PLAN_HD inline int64_t plan_parts(const DLaunch &L) {
  return (L.head_chunks > 1 ? (int64_t)L.n_head * L.head_chunks : 0) +
         (int64_t)(L.n_local_tiles - L.n_head) * (L.n_head < L.n_local_tiles ? L.n_chunks : 0);
}
RT_PLAN_HD inline int plan_tile_chunks(const DLaunch &L, int k) { return k < L.n_head ? L.head_chunks : L.n_chunks; }
// first partial record of chunked plan tile k; its chunk c is record + c
RT_PLAN_HD inline int64_t plan_tile_part0(const DLaunch &L, int k) {
  return k < L.n_head ? (int64_t)k * L.head_chunks
                      : (L.head_chunks > 1 ? (int64_t)L.n_head * L.head_chunks : 0) +
                            (int64_t)(k - L.n_head) * L.n_chunks;
}

struct PlanUnit {
  int tile;             // plan tile (before the dispatch order)
  int s_first, s_count; // strata [s_first, s_first + s_count)
  bool whole;           // writes final pixels, no partial record
  int64_t part;         // partial record index (-1: whole)
};
// Head unit: chunk unit % head_chunks of tile unit / head_chunks; tail unit: a
// chunk of the tail tile n_head + (unit - head units) / n_chunks.
RT_PLAN_HD inline PlanUnit plan_unit(const DLaunch &L, int unit) {
  const int head_units = L.n_head * L.head_chunks;
  const bool head = unit < head_units;
  const int nc = head ? L.head_chunks : L.n_chunks;
  const int cs = head ? (L.sample_count + nc - 1) / nc : L.chunk_strata;
  const int u = head ? unit : unit - head_units, q = u / nc, chunk = u - q * nc;
  PlanUnit r;
  r.tile = head ? q : L.n_head + q;
  r.s_first = L.sample_begin + chunk * cs;
  r.s_count = cs < L.sample_count - chunk * cs ? cs : L.sample_count - chunk * cs;
  r.whole = L.head_chunks == 1 && unit < L.n_head;
  r.part = r.whole ? -1 : unit - (L.head_chunks == 1 ? L.n_head : 0);
  return r;
}

// ---- the planners (rt_plan.cpp)
struct PlanDevice {
  int wave_slots; // resident waves of the render instance on the device
  int pc_grid;    // resident blocks of the persistent instance (0: none)
  int pc_waves;   // its waves per block (0: none)
  // wave slots of the instance that runs the launch (the persistent one's own
  // residency for the feature sets that have one)
  int64_t slots() const { return pc_grid > 0 && pc_waves > 0 ? (int64_t)pc_grid * pc_waves : wave_slots; }
};
UnitPlan frame_plan(const PlanDevice &dev, const rt_tuning &tu, const DLaunch &L);
UnitPlan subset_plan(const PlanDevice &dev, const rt_tuning &tu, const DLaunch &L);
// The share of a frame plan's head that falls to the shard of tiles first +
// k * stride, k in [0, n_local): the tiles below frame.n_head (global index).
UnitPlan shard_plan(UnitPlan frame, int first, int stride, int n_local);
// Every tile in strata_chunks chunks (at most one per stratum).
UnitPlan chunks_plan(int strata_chunks, int sample_count);

#endif
