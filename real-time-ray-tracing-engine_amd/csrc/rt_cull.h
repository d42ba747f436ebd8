// rt_cull.h — which roots the camera rays of one 8x8 tile can reach.
//
// Every camera ray of a flat-world work unit under a pinhole camera leaves
// C.center through the unit's tile, so whether it can meet a root (a static
// sphere of the root table) is largely a property of the tile.  tile_cone
// bounds the tile's ray directions by a cone, root_unreachable sets a root
// against it: `true` says that the kernel's own test of that root
// (rt_path.h sphere_root_origin on a ray of camera_ray_jt) returns false for
// every ray the tile can form; `false` says "don't know".  `true` is a promise,
// `false` is always safe.  Pure functions, no trigonometry, host and device;
// tests/native/rt_tile_cull_check.cpp holds them to the kernel's functions.
//
// The inequality.  Let m be the direction to the tile's centre, beta the
// largest angle between m and a direction of the tile, g the angle between m
// and the root's oc, and alpha the root's angular radius as the kernel's
// arithmetic sees it.  A ray at angle t from oc has t >= g - beta, so with
//     g > alpha + beta,   i.e.   cos g < cos alpha cos beta - sin alpha sin beta
// (all angles in [0, pi], alpha and beta below pi / 2) every ray of the tile
// passes outside.  The function answers `true` only where
//     cos g + 2^-40  <  ca * cb - sa * sb
// holds in its own arithmetic, with (ca, sa) and (cb, sb) as below.
//
// beta: the footprint.  camera_ray_jt forms d = (p00 + (i + px) du + (j + py)
// dv) - center with i + px in [x0 - 0.5, x0 + 7.5], likewise j + py; the
// rectangle used here is wider by kCullPixelMargin = 1/64 pixel on every side,
// which covers the rounding of px and py (a few ulps of the pixel index).  A
// cone of half-angle below pi / 2 is convex and the rectangle is planar, so the
// cone through the farthest of the rectangle's four corners holds all of it:
// cb = min over the corners k of cos(m, k), sb = max of sin(m, k), the sine from
// the cross product so that a small beta keeps its digits.  The rounding of d
// itself: seven operations per component on values of at most
//     M = max_c (|p00_c| + X |du_c| + Y |dv_c| + |center_c|),
// X, Y the largest |pixel coordinate| of the rectangle, so |d - d_exact| <=
// 13 u M (u = 2^-53), and with every |d| >= |m| / 2 (the function requires the
// rectangle's half-diagonal R <= |m| / 2) the direction turns by at most
// 26 u M / |m| (1 + 2^-30).  The function requires M <= 2^12 |m| ("don't know"
// otherwise: a camera whose distance from the origin dwarfs its focus
// distance), so that is below 1.2e-11, and it widens the cone by
// kCullConeMargin = 2^-36 = 1.46e-11 on both cb (down) and sb (up), which also
// covers their own rounding (below 10 u each).
//
// alpha: the kernel's disc = h * h - a * c.  The function takes the kernel's own
// (oc, c) (RootOrigin), so they are exact data here.  With H = d . oc and A =
// |d|^2 exact, |h - H| <= 3 u |d| |oc|, a = A (1 + 3 u), each product and the
// difference round once, so for c > 0
//     disc >= 0   ==>   cos^2 t >= K - 13 u,    K = c / |oc|^2,
// t the exact angle between the kernel's d and oc.  A computed h < 0 cannot
// hit either: c > 0 gives disc <= h * h, sqrt(disc) <= |h|, both roots <= 0 <
// tmin; so a hit needs cos t >= -3 u and with K - 13 u > 9 u^2 altogether
//     hit   ==>   cos t >= sqrt(K - 13 u).
// The function uses Kc = K - kCullDiscMargin, kCullDiscMargin = 2^-46 = 128 u
// (13 u for the kernel, 4 u for its own quotient, the rest spare), ca =
// sqrt(Kc), sa = sqrt(1 - Kc): an angular radius no smaller than the kernel's.
// The margin is taken in K, where the kernel's error lives, so it holds at any
// |oc|^2 / rr: at |oc| / r = 1e6, K = 1 - 1e-12 and 128 u is 1.4 % of 1 - K.
// No underflow or overflow enters: |m|^2 and |oc|^2 must lie in [2^-190,
// 2^190], so a * c >= 2^-428 is normal, and an h * h that underflows is below
// it (no hit).
//
// "Don't know" (false): the origin inside or on the sphere or within the
// margin of it (c <= 0 or Kc <= 0), K > 1 (rr < 0), beta's cone not below pi /
// 2 or the tile not small against |m| (R > |m| / 2), M > 2^12 |m|, magnitudes
// outside the range above, and any non-finite input: every comparison below is
// written so that a NaN fails it.
#ifndef RT_CULL_H
#define RT_CULL_H

#include "rt_path.h"

namespace rtp {

constexpr double kCullPixelMargin = 1.0 / 64;  // pixels, every side of the tile's footprint
constexpr double kCullConeMargin = 0x1p-36;    // on cos beta and sin beta: the rounding of d
constexpr double kCullDiscMargin = 0x1p-46;    // on K = c / |oc|^2: the rounding of disc
constexpr double kCullFinalMargin = 0x1p-40;   // on cos g: this header's own rounding
constexpr double kCullMagLo = 0x1p-190, kCullMagHi = 0x1p190;

// The tile's bounding cone: axis m, |m|^2, cos and sin of its half-angle (both
// with their margins).  ok: the conditions on the tile hold.
struct TileCone {
  V3 m;
  double mm, cb, sb;
  bool ok;
};

// The tile's pixel rectangle is [x0, x0 + 8) x [y0, y0 + 8), whole, also for an
// edge tile.  Only center, p00, du and dv of the camera are read.
RT_HD RT_FI TileCone tile_cone(const DCamera &C, int x0, int y0) {
  const V3 cen = ld3(C.center), p00 = ld3(C.p00), du = ld3(C.du), dv = ld3(C.dv);
  const double xa = (x0 - 0.5) - kCullPixelMargin, xb = (x0 + 7.5) + kCullPixelMargin;
  const double ya = (y0 - 0.5) - kCullPixelMargin, yb = (y0 + 7.5) + kCullPixelMargin;
  const double xm = x0 + 3.5, ym = y0 + 3.5;
  TileCone t;
  t.m = ((p00 + (xm * du)) + (ym * dv)) - cen;
  t.mm = len2(t.m);
  // largest sin^2 and smallest cos^2 over the four corners; dot > 0 at each
  double s2 = 0.0, c2 = 1.0;
  bool front = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    const double x = (k & 1) ? xb : xa, y = (k & 2) ? yb : ya;
    const V3 d = ((p00 + (x * du)) + (y * dv)) - cen;
    const double dm = dot(t.m, d), w = 1.0 / (t.mm * len2(d));
    front = front && dm > 0.0;
    s2 = fmax(s2, len2(cross(t.m, d)) * w);
    c2 = fmin(c2, (dm * dm) * w);
  }
  t.sb = sqrt(s2) + kCullConeMargin;
  t.cb = sqrt(c2) - kCullConeMargin;
  // half-diagonal of the widened rectangle, against |m| / 2; the magnitude of
  // the values d is formed from, against 2^12 |m|
  const double hx = 4.0 + kCullPixelMargin;
  const double R2 = 2.0 * (hx * hx) * (len2(du) + len2(dv)); // (|a| + |b|)^2 <= 2 (|a|^2 + |b|^2)
  const double X = fmax(fabs(xa), fabs(xb)), Y = fmax(fabs(ya), fabs(yb));
  const double M = fmax(fmax(fabs(p00.x) + X * fabs(du.x) + Y * fabs(dv.x) + fabs(cen.x),
                             fabs(p00.y) + X * fabs(du.y) + Y * fabs(dv.y) + fabs(cen.y)),
                        fabs(p00.z) + X * fabs(du.z) + Y * fabs(dv.z) + fabs(cen.z));
  t.ok = front && t.mm >= kCullMagLo && t.mm <= kCullMagHi && 4.0 * R2 <= t.mm && M * M <= 0x1p24 * t.mm &&
         t.cb > 0.0 && t.sb < 1.0 && s2 >= 0.0;
  return t;
}

// No camera ray of the cone's tile can hit root (q, rr): see the head comment.
RT_HD RT_FI bool root_unreachable(const TileCone &t, const RootOrigin &q, double rr) {
  const double oo = len2(q.oc);
  if (!(t.ok && q.c > 0.0 && rr >= 0.0 && oo >= kCullMagLo && oo <= kCullMagHi)) return false;
  const double K = q.c / oo;
  const double Kc = K - kCullDiscMargin;
  if (!(Kc > 0.0 && K <= 1.0)) return false;
  const double ca = sqrt(Kc), sa = sqrt(1.0 - Kc);
  const double cg = dot(t.m, q.oc) / sqrt(t.mm * oo);
  return cg + kCullFinalMargin < ca * t.cb - sa * t.sb;
}

// The unit's root mask, bit ii set: root ii may be reached.  (The kernel forms
// it a root per lane; this is the same arithmetic for the host.)
RT_HD RT_FI unsigned tile_root_mask(const DCamera &C, int x0, int y0, const RootOrigin *q, const double *rr,
                                    int n_roots) {
  const TileCone t = tile_cone(C, x0, y0);
  unsigned mask = 0;
  for (int ii = 0; ii < n_roots; ++ii)
    if (!root_unreachable(t, q[ii], rr[ii])) mask |= 1u << ii;
  return mask;
}

} // namespace rtp
#endif
