// rtx_camq_check — host replay of the camera-ray queue's ring arithmetic
// (csrc/rt_camq.h), as render_tiles' refill uses it (csrc/rt_kernel.hip).
//
//   rtx_camq_check N_ITEMS THRESHOLD SEED
//
// replays one work unit of N_ITEMS items with the kernel's refill rules
// (refill once THRESHOLD lanes are idle, or every lane is) over seeded random
// idle masks, and prints what the queue does, one event per line:
//   R next_item idle_mask_hex      a refill begins (the head before its pop)
//   G gen_items first_entry        the wave generates a batch: lane l writes entry first_entry + l
//   P lane item entry              an idle lane pops an item
//   E pops                         the refill ends after this many pop passes
// The ring holds item numbers where the kernel's holds rays; the program
// itself asserts only camq_may_overwrite at every generation.  What must hold
// of the trace is asserted by tests/test_camera_queue.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../csrc/rt_camq.h"

static uint64_t rng_state;
static uint32_t rnd() { // splitmix64, upper half
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

int main(int argc, char **argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: rtx_camq_check N_ITEMS THRESHOLD SEED\n");
    return 2;
  }
  const int n_items = atoi(argv[1]), threshold = atoi(argv[2]);
  rng_state = strtoull(argv[3], nullptr, 10);
  if (n_items < 0 || n_items % rtq::kBatch != 0 || threshold < 1 || threshold > 64) return 2;
  bool active[64] = {};
  int next_item = 0, gen_items = 0;
  // per trip: each active lane ends its path with probability p / 256; p is
  // redrawn now and then so that refills of every size occur
  uint32_t p = 64;
  for (long trip = 0; trip < 100000000; ++trip) {
    // ---- the refill loop of render_tiles
    for (;;) {
      uint64_t idle = 0;
      for (int l = 0; l < 64; ++l)
        if (!active[l]) idle |= 1ull << l;
      if (idle == 0 || next_item >= n_items) break;
      const int n_idle = __builtin_popcountll(idle);
      if (n_idle < threshold && ~idle != 0ull) break;
      printf("R %d %016llx\n", next_item, (unsigned long long)idle);
      const int need = rtq::camq_need(next_item, n_idle, n_items);
      while (rtq::camq_generate(gen_items, need)) {
        if (!rtq::camq_may_overwrite(gen_items, next_item)) {
          fprintf(stderr, "batch at %d would overwrite unpopped items (head %d)\n", gen_items, next_item);
          return 1;
        }
        printf("G %d %d\n", gen_items, rtq::camq_write_entry(gen_items, 0));
        gen_items += rtq::kBatch;
      }
      for (int l = 0; l < 64; ++l) {
        const int rank = __builtin_popcountll(idle & ((1ull << l) - 1ull));
        const int item = next_item + rank;
        if (!active[l] && item < n_items) {
          printf("P %d %d %d\n", l, item, rtq::camq_read_entry(item));
          active[l] = rnd() % 16 != 0; // an item outside the image leaves its lane idle
        }
      }
      next_item += n_idle;
      printf("E 1\n");
    }
    bool any = false;
    for (int l = 0; l < 64; ++l) any = any || active[l];
    if (!any) break;
    if (rnd() % 8 == 0) p = 1 + rnd() % 255;
    for (int l = 0; l < 64; ++l)
      if (active[l] && rnd() % 256 < p) active[l] = false;
  }
  printf("D %d %d\n", next_item, gen_items);
  return 0;
}
