// rt_refit.h — a world item's box from the device tables alone, and the fp32
// rounding of the builders: the source the refit kernels (rt_refit.hip) and
// their host twin (tests/native/rt_refit_emu.cpp) share.
//
// The scene compiler (rt_scene.cpp) computes each item's fp64 world box from
// the caller's description with the reference's rules (AABB.cpp:7-27, 167-175;
// Sphere.cpp:15-23; Plane.cpp:17-20; RotateY.cpp:10-34; AABBUtility.hpp:7-11).
// After spheres have moved (rt_scene_move_spheres) or transforms and quads have
// been edited (rt_scene_set_transforms, rt_scene_move_quads; rt_live.h) the
// description is gone, so
// the same rules are restated here over DSphere / DQuad / DXform, operation by
// operation: for a scene that has not moved, the boxes -- and so every refitted
// node -- are the compiler's bit for bit (tests/test_refit.py holds them to
// that over every committed scene; tests/test_live_edits.py holds medium_box,
// a world medium's fp32 box, to the compiler's mbox likewise).  Built with -ffp-contract=off like
// rt_scene.cpp; nothing here may be contracted.
//
// The radius is sqrt(rr): DSphere keeps r*r and 1/r, and sqrt(r*r) == r for
// every r whose square neither overflows nor underflows (the squaring loses at
// most half an ulp, the root halves the relative error, and the rounded root
// of a value within half an ulp of r*r is r itself; tests/test_refit.py samples
// it).  A sphere described with a negative radius has rr == 0: its refitted box
// is that of radius 0, which covers what the kernel tests (Sphere::hit with
// rr == 0); the identity above holds for radii >= 0.
#ifndef RT_REFIT_H
#define RT_REFIT_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_layout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_REFIT_HD __host__ __device__ inline
#else
#define RT_REFIT_HD inline
#endif

namespace rt_refit {

struct Bx { // rt_scene.cpp's Bx
  double lo[3], hi[3];
};

RT_REFIT_HD void bx_pad(Bx &b) { // pad_to_minimums
  for (int i = 0; i < 3; ++i)
    if (b.hi[i] - b.lo[i] < 0.0001) {
      b.lo[i] -= 0.0001 * 0.5;
      b.hi[i] += 0.0001 * 0.5;
    }
}
RT_REFIT_HD Bx bx_points(const double a[3], const double b[3]) {
  Bx r;
  for (int i = 0; i < 3; ++i) {
    const double u = a[i], v = b[i];
    r.lo[i] = u <= v ? u : v;
    r.hi[i] = u <= v ? v : u;
  }
  bx_pad(r);
  return r;
}
RT_REFIT_HD Bx bx_join(const Bx &a, const Bx &b) {
  Bx r;
  for (int i = 0; i < 3; ++i) {
    r.lo[i] = a.lo[i] <= b.lo[i] ? a.lo[i] : b.lo[i];
    r.hi[i] = a.hi[i] >= b.hi[i] ? a.hi[i] : b.hi[i];
  }
  return r;
}

// bx_points(c - r, c + r)
RT_REFIT_HD Bx ball_box(const double c[3], double r) {
  double a[3], b[3];
  for (int i = 0; i < 3; ++i) {
    a[i] = c[i] - r;
    b[i] = c[i] + r;
  }
  return bx_points(a, b);
}
RT_REFIT_HD Bx sphere_box(const DSphere &s) {
  const double r = sqrt(s.rr);
  Bx b = ball_box(s.c0, r);
  if (s.dir[0] != 0.0 || s.dir[1] != 0.0 || s.dir[2] != 0.0) { // Sphere.cpp:15-23: both ends
    double c1[3];
    for (int i = 0; i < 3; ++i) c1[i] = s.c0[i] + 1 * s.dir[i];
    b = bx_join(b, ball_box(c1, r));
  }
  return b;
}
RT_REFIT_HD Bx quad_box(const DQuad &q) { // Plane.cpp:17-20: both diagonals
  double quv[3], qu[3], qv[3];
  for (int i = 0; i < 3; ++i) {
    qu[i] = q.Q[i] + q.u[i];
    quv[i] = qu[i] + q.v[i];
    qv[i] = q.Q[i] + q.v[i];
  }
  return bx_join(bx_points(q.Q, quv), bx_points(qu, qv));
}
RT_REFIT_HD Bx rot_box(const Bx &cb, double s, double c) { // RotateY.cpp:10-34
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++)
      for (int k = 0; k < 2; k++) {
        const double px = i * cb.hi[0] + (1 - i) * cb.lo[0];
        const double py = j * cb.hi[1] + (1 - j) * cb.lo[1];
        const double pz = k * cb.hi[2] + (1 - k) * cb.lo[2];
        const double t[3] = {c * px + s * pz, py, -s * px + c * pz};
        for (int a = 0; a < 3; a++) {
          mn[a] = fmin(mn[a], t[a]);
          mx[a] = fmax(mx[a], t[a]);
        }
      }
  return bx_points(mn, mx);
}
RT_REFIT_HD Bx trans_box(const Bx &cb, double x, double y, double z) { // AABBUtility.hpp:7-11
  Bx b;
  const double o[3] = {x, y, z};
  for (int i = 0; i < 3; ++i) {
    b.lo[i] = cb.lo[i] + o[i];
    b.hi[i] = cb.hi[i] + o[i];
  }
  bx_pad(b);
  return b;
}

// The world box of a world primitive item (a sphere or a quad; media are not
// in the world tree): its primitive's box under its transform chain, innermost
// (last) first.
RT_REFIT_HD Bx item_box(const DItem &it, const DSphere *spheres, const DQuad *quads, const DXform *xforms) {
  Bx b = it.kind == I_SPHERE ? sphere_box(spheres[it.idx]) : quad_box(quads[it.idx]);
  for (int k = it.xf_count; k-- > 0;) {
    const DXform &x = xforms[it.xf_first + k];
    b = x.kind == X_ROTATE_Y ? rot_box(b, x.a, x.b) : trans_box(b, x.a, x.b, x.c);
  }
  return b;
}

RT_REFIT_HD Bx bx_empty() { // the compiler's empty box
  Bx b;
  for (int i = 0; i < 3; ++i) {
    b.lo[i] = INFINITY;
    b.hi[i] = -INFINITY;
  }
  return b;
}

// fp32 bounds rounded outward with the builders' margins (rt_scene.cpp
// SahBuilder::f32_lo / f32_hi; nextafter written on the bits, as
// rt_bvh_build.hip has it).
RT_REFIT_HD float bits_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
RT_REFIT_HD uint32_t float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
RT_REFIT_HD float next_down(float f) {
  if (f == 0.0f) return bits_float(0x80000001u);
  const uint32_t u = float_bits(f);
  return bits_float(f > 0.0f ? u - 1u : u + 1u);
}
RT_REFIT_HD float next_up(float f) {
  if (f == 0.0f) return bits_float(0x00000001u);
  const uint32_t u = float_bits(f);
  return bits_float(f > 0.0f ? u + 1u : u - 1u);
}
RT_REFIT_HD float f32_lo(double x) {
  const double m = x - (fabs(x) * 0x1p-20 + 1e-7);
  float f = (float)m;
  if ((double)f > m) f = next_down(f);
  return f;
}
RT_REFIT_HD float f32_hi(double x) {
  const double m = x + (fabs(x) * 0x1p-20 + 1e-7);
  float f = (float)m;
  if ((double)f < m) f = next_up(f);
  return f;
}

// The world box of a world medium item (DScene::mbox's six floats, lo xyz then
// hi xyz): the join of its boundary items' boxes, each under its own chain in
// the medium's local frame, then the medium item's chain, innermost first,
// rounded outward -- the compiler's make_item and run() (rt_scene.cpp), operation
// by operation.  Nothing here reads DMedium's face constants (bnk, bD, bB):
// they are functions of the boundary quads in the boundary's frame alone.
RT_REFIT_HD void medium_box(const DItem &m, const DMedium *media, const DItem *bitems, const DSphere *spheres,
                            const DQuad *quads, const DXform *xforms, float out[6]) {
  const DMedium &md = media[m.idx];
  Bx b = bx_empty();
  for (int k = 0; k < md.b_count; ++k) b = bx_join(b, item_box(bitems[md.b_first + k], spheres, quads, xforms));
  for (int k = m.xf_count; k-- > 0;) {
    const DXform &x = xforms[m.xf_first + k];
    b = x.kind == X_ROTATE_Y ? rot_box(b, x.a, x.b) : trans_box(b, x.a, x.b, x.c);
  }
  for (int a = 0; a < 3; ++a) {
    out[a] = f32_lo(b.lo[a]);
    out[3 + a] = f32_hi(b.hi[a]);
  }
}

// A node of either width as the refit sees it: DNode (A = 2) and DNode4
// (A = 4) are both lo[3][A], hi[3][A], entry[A], pad[A].
template <int A>
struct NodeOf {
  float lo[3][A], hi[3][A];
  int32_t entry[A];
  int32_t pad[A];
};
static_assert(sizeof(NodeOf<2>) == sizeof(DNode) && sizeof(NodeOf<4>) == sizeof(DNode4), "node layouts");

// The union of the rounded boxes of the items of one leaf entry
// (~((first << 3) | count)): exact fp32 min / max.
RT_REFIT_HD void leaf_union(int32_t entry, const double *boxes, float lo[3], float hi[3]) {
  const int first = (~entry) >> 3, count = (~entry) & 7;
  for (int a = 0; a < 3; ++a) {
    lo[a] = INFINITY;
    hi[a] = -INFINITY;
  }
  for (int i = first; i < first + count; ++i) {
    const double *b = boxes + 6 * (size_t)i;
    for (int a = 0; a < 3; ++a) {
      const float l = f32_lo(b[a]), h = f32_hi(b[a + 3]);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
}
// ... and of a node's own non-empty slots (entry -1: an empty 4-wide slot)
template <int A>
RT_REFIT_HD void node_union(const NodeOf<A> &n, float lo[3], float hi[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = INFINITY;
    hi[a] = -INFINITY;
  }
  for (int k = 0; k < A; ++k) {
    if (n.entry[k] == -1) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = n.lo[a][k] < lo[a] ? n.lo[a][k] : lo[a];
      hi[a] = n.hi[a][k] > hi[a] ? n.hi[a][k] : hi[a];
    }
  }
}

} // namespace rt_refit
#endif
