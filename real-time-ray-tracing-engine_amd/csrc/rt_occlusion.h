// rt_occlusion.h — any-hit visibility of caller rays (rt_occluded_device;
// DESIGN.md §7n).
//
// The verdict of one rt_ray: 1 exactly where rt_query.h query_ray's record of
// the same ray is a hit.  It is reached by a walk of its own, not by
// trace_closest and a comparison: the interval is (0.001, limit] from the
// first node on and never narrows, so the fp32 box bound is one constant per
// ray and a short segment culls every box beyond its end, and a lane leaves
// at the first primitive it accepts.  The walk is built from rt_path.h's
// pieces -- sphere_root, quad_t, to_local, the slab and plane helpers -- with
// the operands trace gives them, so every root is trace's double; rt_path.h
// itself is untouched.  RT_HD code like rt_query.h: the gfx950 kernel
// (rt_occlusion.hip) and the host build (tests/native/rt_occlusion_emu.cpp)
// compile this one source with -ffp-contract=off.
//
// Why the fixed interval gives trace's verdict (the argument in full: §7n).
// trace's minimum is taken over what each item offers it, whatever the order:
//  * a quad offers its plane distance t when tmin <= t (quad_t's closed
//    interval; the narrowing bound only ever removes offers above the running
//    minimum).  query_ray accepts closest <= limit, so the quad blocks iff
//    tmin <= t <= limit: quad_t with tmax = limit.
//  * a sphere offers its near root n when tmin < n, else its far root f when
//    tmin < f (sphere_root's open interval; n <= f).  It blocks iff that offer
//    is <= limit.  sphere_root with tmax = up(limit), the next double above
//    limit, accepts n iff tmin < n <= limit; when it rejects n, either
//    n <= tmin, and f is tested the same way, or n > limit, and f >= n fails
//    too -- the far root counts only when the near one is at or below tmin, as
//    in trace.  (up(+inf) = +inf: trace's own first bound.)
#ifndef RT_OCCLUSION_H
#define RT_OCCLUSION_H
#include "rt_query.h"

namespace rto {

using namespace rtq;

// the next double above x, for x > 0 (finite or +inf; +inf stays)
RT_HD RT_FI double next_up(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  return b == 0x7ff0000000000000ull ? x : __builtin_bit_cast(double, b + 1);
}

// Whether world item ii stops ray r (|d|^2 = a, its reciprocal ya) within
// (tmin, limit]: trace's item_root_t with the two bounds above.  U: ii is the
// same in every lane (the flat walk) -- scalar loads and the constant-axis
// quad form, the same operations on the same values.
template <unsigned F, bool U>
RT_HD RT_FI bool item_blocks(const DScene &S, int ii, const Ray &r, double a, double ya, double limit,
                             double limit_up) {
  const double tmin = 0.001; // Camera.cpp:242, as trace
  const DItem it = ldu<U>(S.items, ii);
  Ray lr = r;
  double al = a;
  bool local = false;
  if constexpr ((F & F_XFORM) != 0) {
    if (it.xf_count) {
      lr = to_local<U>(S, it.xf_first, it.xf_count, r);
      al = len2(lr.d);
      local = true;
    }
  }
  double t;
  if (it.kind == I_SPHERE) {
    const double yl = local ? 1.0 / al : ya;
    return sphere_root<true>(ldu<U>(S.spheres, it.idx), lr, al, tmin, limit_up, t, true, yl);
  }
  // (rtp:: by name: sys/types.h has a quad_t of its own)
  if constexpr (U) return rtp::quad_t<true, true>(ldu<true>(S.quads, it.idx), lr, tmin, limit, t);
  // the record where it lies: quad_t_aa indexes it by axis, and a copy indexed so would live in scratch
  return rtp::quad_t<false, false>(S.quads[it.idx], lr, tmin, limit, t);
}

// 1: something stands in (0.001, t_max] of the ray; 0: nothing does, or the
// ray is not traced at all (ray_valid).  stk: this lane's traversal stack
// (stk[64 k] its k-th entry), S.stack_depth entries as for trace: the pushes
// are trace's (one sibling per binary level, up to three per 4-wide level).
template <unsigned F>
RT_HD RT_FI uint8_t occluded_ray(const DScene &S, const rt_ray &q, int *stk) {
  static_assert(F == query_features(F), "an occlusion instance has no media, lights or noise");
  bool hit = false;
  if (ray_valid(q)) { // a divergent branch: invalid rays never enter a loop
    const Ray r{ld3(q.origin), ld3(q.direction), q.time};
    const double limit = q.t_max > 0.0 ? q.t_max : kInf;
    const double limit_up = next_up(limit);
    const double a = len2(r.d);
    const double ya = 1.0 / a;
    if constexpr ((F & F_FLAT) != 0) {
      // the root leaf's items in turn, wave-uniform; a lane that is blocked
      // tests no more, and the wave leaves once every lane is
      for (int ii = 0; ii < S.n_root_items; ++ii) {
        if (!hit) hit = item_blocks<F, true>(S, ii, r, a, ya, limit, limit_up);
        if (wave_none(!hit)) break;
      }
    } else {
      // trace's while-while walk with postponed leaves, without a running
      // minimum: tmin32 and cl32 are constants of the ray.  Near child first,
      // as in trace: the entry distances are at hand, and the nearer box is
      // the likelier one to hold a blocker inside a short interval.
      const RayF<true> qf = ray_f32<true>(r);
      const float tmin32 = f32_dn(0.001);
      const float cl32 = f32_up_c(limit);
      int *top = stk;
      auto push = [&](int e) {
        *top = e;
        top += 64;
      };
      auto pop = [&]() -> int {
        if (top == stk) return -1;
        top -= 64;
        return *top;
      };
      int cur = 0, lf = 0, ln = 0;
      if (S.root_is_leaf) {
        cur = -1;
        ln = S.n_root_items;
      }
      [[maybe_unused]] PlaneOff po{};
      if constexpr ((F & F_BVH4) != 0) po = plane_offsets<4>(qf);
      for (;;) {
        while (cur >= 0) {
          if (wave_none(ln == 0)) break; // every walking lane holds a leaf: test them
          if constexpr ((F & F_BVH4) != 0) {
            NodePlanes<4> pl;
            load_planes<4>(pl, (const char *)S.nodes, cur * (int)sizeof(DNode4), po);
            float tn[4];
            bool hh[4];
            int en[4];
            slab_planes<4>(qf, pl, tmin32, cl32, tn, hh);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              en[c] = pl.en[c];
              if (en[c] == -1 || !hh[c]) tn[c] = __builtin_huge_valf();
            }
            auto cswap = [&](int x, int y) {
              const bool sw = tn[y] < tn[x];
              const float tx = tn[x], ty = tn[y];
              const int ex = en[x], ey = en[y];
              tn[x] = sw ? ty : tx;
              tn[y] = sw ? tx : ty;
              en[x] = sw ? ey : ex;
              en[y] = sw ? ex : ey;
            };
            cswap(0, 1);
            cswap(2, 3);
            cswap(0, 2);
            cswap(1, 3);
            cswap(1, 2);
#pragma unroll
            for (int c = 3; c >= 1; --c)
              if (tn[c] != __builtin_huge_valf()) push(en[c]);
            cur = tn[0] != __builtin_huge_valf() ? en[0] : pop();
          } else {
            const DNode N = S.nodes[cur];
            float tn0, tn1;
            bool h0, h1;
            slab_hit2(qf, N, tmin32, cl32, tn0, tn1, h0, h1);
            if (h0 && h1) {
              const bool first0 = tn0 <= tn1;
              push(first0 ? N.entry[1] : N.entry[0]);
              cur = first0 ? N.entry[0] : N.entry[1];
            } else if (h0 || h1) {
              cur = h0 ? N.entry[0] : N.entry[1];
            } else {
              cur = pop();
            }
          }
          if (cur < -1 && ln == 0) { // first leaf: park it, keep walking
            lf = (~cur) >> 3;
            ln = (~cur) & 7;
            cur = pop();
          }
        }
        if (ln == 0) break; // nothing parked and nothing left to walk: unoccluded
        while (ln > 0 && !hit) {
          hit = item_blocks<F, false>(S, lf, r, a, ya, limit, limit_up);
          ++lf;
          --ln;
        }
        if (hit) break; // done: no further leaf tests or node visits for this lane
        if (cur < -1) { // a second leaf met while one was parked: it is next
          lf = (~cur) >> 3;
          ln = (~cur) & 7;
          cur = pop();
        }
      }
    }
  }
  return hit ? 1 : 0;
}

} // namespace rto
#endif
