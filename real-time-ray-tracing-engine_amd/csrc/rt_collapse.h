// rt_collapse.h — one 4-wide node of the collapsed world BVH from the binary
// tree: the source the host collapse (rt_scene.cpp collapse_bvh4) and the
// device collapse (rt_collapse.hip) share.
//
// A 4-wide node starts from the two children of one binary node and opens, up
// to twice, its inner child of largest half-area x*y + y*z + z*x (extents
// formed in fp64, (double)hi - lo per axis; the first maximum wins, strict >);
// the two children of the opened one take its place, so the leaf order is
// kept.  The expansion reads the source node and at most two more, whatever
// the rest of the tree looks like: that is what lets the device run one thread
// per 4-wide node of a level.  Built with -ffp-contract=off on both sides, so
// the areas -- and with them every choice -- are the same doubles.
//
// The loops run over all four slots with the slot index a constant after
// unrolling (a predicate instead of c[pick]): on the device the children stay
// in registers.
#ifndef RT_COLLAPSE_H
#define RT_COLLAPSE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_layout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_COLLAPSE_HD __host__ __device__ inline
#define RT_COLLAPSE_UNROLL _Pragma("unroll")
#else
#define RT_COLLAPSE_HD inline
#define RT_COLLAPSE_UNROLL
#endif

namespace rt_collapse {

struct Child { // one child box of a binary node and its entry
  float lo[3], hi[3];
  int32_t e;
};

RT_COLLAPSE_HD Child child_of(const DNode &b, int k) {
  Child c;
  for (int a = 0; a < 3; ++a) {
    c.lo[a] = b.lo[a][k];
    c.hi[a] = b.hi[a][k];
  }
  c.e = b.entry[k];
  return c;
}
RT_COLLAPSE_HD Child no_child() { // an empty slot
  Child c;
  for (int a = 0; a < 3; ++a) {
    c.lo[a] = INFINITY;
    c.hi[a] = -INFINITY;
  }
  c.e = -1;
  return c;
}
RT_COLLAPSE_HD double half_area(const Child &c) {
  const double x = (double)c.hi[0] - c.lo[0], y = (double)c.hi[1] - c.lo[1], z = (double)c.hi[2] - c.lo[2];
  return x * y + y * z + z * x;
}
// an entry that names a binary node (one at or past n_bin is no tree's: it is
// carried like a leaf entry, never followed)
RT_COLLAPSE_HD bool is_inner(int32_t e, int n_bin) { return e >= 0 && e < n_bin; }

// The children of the 4-wide node whose source is binary node `src`, in slot
// order into c[0 .. n): returns n (2 to 4); c[n .. 4) are empty slots.
RT_COLLAPSE_HD int expand(const DNode *bin, int n_bin, int src, Child c[4]) {
  c[0] = child_of(bin[src], 0);
  c[1] = child_of(bin[src], 1);
  c[2] = c[3] = no_child();
  int n = 2;
  RT_COLLAPSE_UNROLL
  for (int round = 0; round < 2; ++round) {
    int pick = -1;
    int32_t open = -1;
    double best = -1.0;
    RT_COLLAPSE_UNROLL
    for (int i = 0; i < 4; ++i) {
      if (i >= n || !is_inner(c[i].e, n_bin)) continue;
      const double a = half_area(c[i]);
      if (a > best) {
        best = a;
        pick = i;
        open = c[i].e;
      }
    }
    if (pick < 0) break;
    const Child l = child_of(bin[open], 0), r = child_of(bin[open], 1);
    RT_COLLAPSE_UNROLL
    for (int i = 3; i >= 1; --i) // keep the leaf order
      if (i <= n && i > pick + 1) c[i] = c[i - 1];
    RT_COLLAPSE_UNROLL
    for (int i = 0; i < 4; ++i) {
      if (i == pick) c[i] = l;
      if (i == pick + 1) c[i] = r;
    }
    ++n;
  }
  return n;
}

// The node of those children: SoA boxes, empty slots +inf / -inf and entry -1,
// pads zero.  Every entry is still the binary tree's: leaf entries stay, and
// the caller replaces each inner one (is_inner) by the 4-wide index it gives
// that child.
RT_COLLAPSE_HD DNode4 node_of(const Child c[4]) {
  DNode4 q;
  for (int i = 0; i < 4; ++i) {
    for (int a = 0; a < 3; ++a) {
      q.lo[a][i] = c[i].lo[a];
      q.hi[a][i] = c[i].hi[a];
    }
    q.entry[i] = c[i].e;
    q.pad[i] = 0;
  }
  return q;
}

} // namespace rt_collapse
#endif
