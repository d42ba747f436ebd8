// rtx_batch_check — host replay of the flat world's refill and parking flow
// (csrc/rt_kernel.hip render_tiles, F == F_FLAT) with camera-ray batches
// traced where they are generated (csrc/rt_camq.h kClosest / kBest).
//
//   rtx_batch_check N_ITEMS THRESHOLD K SEED MODE
//
// MODE: mixed   every camera ray hits with a probability redrawn per batch
//       allmiss no camera ray hits            allhit  every camera ray hits
//       lens    nothing is traced at generation: a popped lane is active and
//               untraced, and the path loop's trace site decides (a defocus disk)
//
// Replays one work unit of N_ITEMS items with the kernel's rules -- refill
// once THRESHOLD lanes are idle or every lane is, repeated while that holds
// and items remain; shade once K lanes hold a hit or no refill can add to
// them -- over seeded random outcomes: per item whether its slot lies in the
// image and whether its camera ray hits, per traced bounce ray whether it
// hits, per shade whether the path goes on.  The ring holds item numbers and
// outcomes where the kernel's holds rays and roots.  Checked, exit status 1
// with a message otherwise:
//   * every item inside the image is either settled once as a miss or handed
//     once to the idle lane of its rank, parked; an item outside is consumed
//     and leaves its lane idle;
//   * no entry is read before its batch is written or after it is overwritten
//     (the entry holds the item that is read), and a batch overwrites only
//     popped items (camq_may_overwrite);
//   * every pass of the refill loop advances next_item, and a trip after one
//     that waited (`wait`) takes at least one item in its refill; every trip
//     takes an item, traces a lane or shades one;
//   * the loop ends, with every item consumed and every batch generated once.
// Prints one line of counts (tests/test_batch_trace.py reads it).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/rt_camq.h"

static uint64_t rng_state;
static uint32_t rnd() { // splitmix64, upper half
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

#define FAIL(...)                 \
  do {                            \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
    return 1;                     \
  } while (0)

struct Entry {
  int item = -1;       // the item the entry holds (-1: never written)
  bool inside = false; // its slot lies in the image
  bool hit = false;    // its camera ray's outcome (traced at generation)
};

int main(int argc, char **argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: rtx_batch_check N_ITEMS THRESHOLD K SEED mixed|allmiss|allhit|lens\n");
    return 2;
  }
  const int n_items = atoi(argv[1]), threshold = atoi(argv[2]), park_k = atoi(argv[3]);
  rng_state = strtoull(argv[4], nullptr, 10);
  const char *mode = argv[5];
  const bool lens = !strcmp(mode, "lens"), allmiss = !strcmp(mode, "allmiss"), allhit = !strcmp(mode, "allhit");
  if (!lens && !allmiss && !allhit && strcmp(mode, "mixed")) return 2;
  if (n_items < 0 || n_items % rtq::kBatch != 0 || threshold < 1 || threshold > 64 || park_k < 1 || park_k > 64)
    return 2;
  const int max_depth = 8;

  Entry ring[rtq::kEntries];
  std::vector<int> settled(n_items, 0), handed(n_items, 0), outside(n_items, 0);
  bool active[64] = {}, parked[64] = {};
  int bounce[64] = {};
  int next_item = 0, gen_items = 0;
  long trips = 0, passes = 0, max_passes = 0, n_hits = 0, n_misses = 0, n_outside = 0, n_waits = 0, n_shades = 0;
  bool waited = false; // the previous trip's `wait`
  const long trip_cap = 64L * (n_items + 64) * (max_depth + 2);
  for (;; ++trips) {
    if (trips > trip_cap) FAIL("the loop does not end: %ld trips, head %d of %d", trips, next_item, n_items);
    // ---- the refill loop of render_tiles
    int took = 0;
    long trip_passes = 0;
    for (;;) {
      uint64_t idle = 0;
      for (int l = 0; l < 64; ++l)
        if (!active[l]) idle |= 1ull << l;
      if (idle == 0 || next_item >= n_items) break;
      const int n_idle = __builtin_popcountll(idle);
      if (n_idle < threshold && ~idle != 0ull) break;
      const int need = rtq::camq_need(next_item, n_idle, n_items);
      while (rtq::camq_generate(gen_items, need)) {
        if (!rtq::camq_may_overwrite(gen_items, next_item))
          FAIL("batch at %d would overwrite unpopped items (head %d)", gen_items, next_item);
        const uint32_t p_hit = rnd() % 257; // of 256, this batch's camera rays
        for (int l = 0; l < 64; ++l) {
          Entry &e = ring[rtq::camq_write_entry(gen_items, l)];
          if (e.item >= next_item) FAIL("entry of unpopped item %d overwritten", e.item);
          e.item = gen_items + l;
          e.inside = rnd() % 16 != 0;
          // traced here, by the generating lane, only inside the image and without a lens
          e.hit = !lens && e.inside && (allhit || (!allmiss && rnd() % 256 < p_hit));
        }
        gen_items += rtq::kBatch;
      }
      const int head = next_item;
      next_item += n_idle;
      for (int l = 0; l < 64; ++l) {
        const int rank = __builtin_popcountll(idle & ((1ull << l) - 1ull));
        const int item = head + rank;
        if (active[l] || item >= n_items) continue;
        if (parked[l]) FAIL("idle lane %d holds a parked hit", l);
        const Entry &e = ring[rtq::camq_read_entry(item)];
        if (e.item != item) FAIL("lane %d reads item %d from an entry that holds %d", l, item, e.item);
        ++took;
        if (!e.inside) { // consumed, the lane stays idle
          ++outside[item];
          ++n_outside;
        } else if (lens) { // active and untraced: the path loop traces it
          ++handed[item];
          active[l] = true;
          bounce[l] = 0;
        } else if (e.hit) { // active and parked
          ++handed[item];
          ++n_hits;
          active[l] = parked[l] = true;
          bounce[l] = 0;
        } else { // the background, added at once; the lane stays idle
          ++settled[item];
          ++n_misses;
        }
      }
      if (next_item <= head) FAIL("a refill pass at head %d took nothing", head);
      ++passes;
      ++trip_passes;
    }
    if (trip_passes > max_passes) max_passes = trip_passes;
    if (waited && took == 0) FAIL("trip %ld follows a waiting trip and its refill takes no item (head %d of %d)", trips, next_item, n_items);
    bool any = false;
    for (int l = 0; l < 64; ++l) any = any || active[l];
    if (!any) break;
    // ---- the path loop's trace site: active lanes that hold no hit
    bool done[64] = {};
    int traced = 0, shaded = 0;
    for (int l = 0; l < 64; ++l)
      if (active[l] && !parked[l]) {
        ++traced;
        const bool camera = bounce[l] == 0;
        if (camera && !lens) FAIL("lane %d traces a camera ray in the path loop", l);
        const bool hit = camera ? (allhit || (!allmiss && rnd() % 2 != 0)) : rnd() % 4 != 0;
        if (hit) parked[l] = true;
        else {
          done[l] = true;
          if (camera) ++n_misses;
        }
        if (camera && hit) ++n_hits;
      }
    int n_parked = 0, n_free = 0;
    for (int l = 0; l < 64; ++l) {
      n_parked += active[l] && parked[l];
      n_free += !active[l] || done[l];
    }
    const bool wait = n_parked < park_k && next_item < n_items && n_free >= threshold;
    if (!wait)
      for (int l = 0; l < 64; ++l)
        if (active[l] && parked[l]) { // ---- the one shade site
          ++shaded;
          parked[l] = false;
          ++bounce[l];
          if (bounce[l] >= max_depth || rnd() % 8 == 0) done[l] = true; // depth cap, emitter or absorption
        }
    n_waits += wait;
    n_shades += shaded > 0;
    if (took == 0 && traced == 0 && shaded == 0)
      FAIL("trip %ld takes no item, traces no lane and shades none (head %d of %d)", trips, next_item, n_items);
    for (int l = 0; l < 64; ++l)
      if (done[l]) active[l] = false;
    waited = wait;
  }
  if (next_item < n_items || gen_items != n_items) FAIL("ended at head %d, %d generated, of %d", next_item, gen_items, n_items);
  for (int k = 0; k < n_items; ++k) {
    const int n = settled[k] + handed[k] + outside[k];
    if (n != 1) FAIL("item %d: settled %d, handed %d, outside %d", k, settled[k], handed[k], outside[k]);
  }
  printf("OK items %d hits %ld misses %ld outside %ld trips %ld passes %ld max_passes %ld waits %ld shades %ld\n", n_items,
         n_hits, n_misses, n_outside, trips, passes, max_passes, n_waits, n_shades);
  return 0;
}
