// rt_camq.h — the per-wave camera-ray queue of the plain flat world, its ring
// arithmetic defined once.
//
// A work unit's items are numbered k = 0 .. n_items - 1; item k is (pixel slot
// k & 63, stratum s_first + (k >> 6)), so a batch of 64 consecutive items,
// batch g = items [64 g, 64 g + 64), is one stratum of all 64 pixels of the
// tile.  render_tiles (rt_kernel.hip) generates a batch with the whole wave,
// lane l making item 64 g + l, and keeps it in LDS; the idle lanes of a refill
// then pop their items, idle lane of rank r taking item next_item + r as it
// always did.  The ring holds two batches: batch g lives in entries
// [64 (g & 1), 64 (g & 1) + 64), entry = item & 127, laid out structure-of-
// arrays so that a batch writes entry = lane and a pop reads consecutive
// entries from consecutive idle lanes.
//
// A refill of n_idle lanes pops items [next_item, min(next_item + n_idle,
// n_items)): at most 64 of them, so they lie in at most two batches, the one
// next_item is in and the next.  Batches are generated in order, and batch g
// only when a pop needs an item of it (camq_generate): then 64 g < next_item +
// 64, so every item of batch g - 2, whose entries batch g overwrites, has been
// popped by an earlier refill (camq_may_overwrite).  One pop per refill; no
// entry is read before its batch is written or after it is overwritten.
// host/rtx_camq_check.cpp replays this on the CPU (tests/test_camera_queue.py).
#ifndef RT_CAMQ_H
#define RT_CAMQ_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_CAMQ_HD __host__ __device__
#else
#define RT_CAMQ_HD
#endif

namespace rtq {

constexpr int kBatch = 64;                // items of a batch: one stratum of the tile's 64 pixels
constexpr int kBatches = 2;               // batches the ring holds
constexpr int kEntries = kBatch * kBatches;
// doubles of an entry: ray direction, ray time, ray origin (written and read
// only with a defocus disk; without one the origin is the camera centre)
constexpr int kComps = 7;
// Without a defocus disk the batch is traced where it is generated, and the
// first two origin components hold the outcome instead: the closest root, and
// the world item it belongs to (an int in the double's low bits; -1: a miss).
constexpr int kClosest = 4;
constexpr int kBest = 5;

// One past the last item the pop of a refill reads: idle lane of rank r takes
// item next_item + r while that is an item of the unit.
RT_CAMQ_HD inline int camq_need(int next_item, int n_idle, int n_items) {
  const int e = next_item + n_idle;
  return e < n_items ? e : n_items;
}
// Whether the next batch (items [gen_items, gen_items + 64)) has to be
// generated before the pop: gen_items counts the items generated so far, a
// multiple of 64; need <= n_items, so no batch past the unit's last is made.
RT_CAMQ_HD inline bool camq_generate(int gen_items, int need) { return gen_items < need; }
// The stratum of the unit (0-based: add s_first) the next batch holds.
RT_CAMQ_HD inline int camq_batch(int gen_items) { return gen_items / kBatch; }
// The entry lane `lane` writes when the wave generates the next batch.
RT_CAMQ_HD inline int camq_write_entry(int gen_items, int lane) { return (gen_items & (kEntries - 1)) + lane; }
// The entry item `item` is read from.
RT_CAMQ_HD inline int camq_read_entry(int item) { return item & (kEntries - 1); }
// Whether generating the next batch overwrites only entries whose items
// (those of the batch two before it) earlier refills have popped: next_item is
// the queue's head before this refill's pop.  Implied by camq_generate with
// need <= next_item + 64; the host check asserts it at every generation.
RT_CAMQ_HD inline bool camq_may_overwrite(int gen_items, int next_item) {
  return gen_items < kEntries || next_item >= gen_items - kBatch;
}

} // namespace rtq
#endif
