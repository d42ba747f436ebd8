// rt_motion.h — object motion vectors, one pixel (rt_motion_device).
//
// A new kind in the query family (rt_query.h): the ray is the pixel-centre ray
// of a frame, formed here with rt_pixel_ray's operations, and the record says
// where the surface under the pixel stood at an earlier pose of the scene
// (rt_live.h: a pose) instead of where it is.  The search is the render's own
// (trace_closest, media masked out of the instance as in every query); t,
// object and chain_object are rt_trace_device's bytes for the same ray.
//
// The hit is taken into the winning item's local frame through the current
// chain; its offset from the primitive's anchor (c0 of a sphere, Q of a quad)
// and its local normal are then placed twice by one function, once with the
// scene's tables and once with the pose's values of the same records.  Both
// calls run the same operations, so an object nothing moved gets d = dn = +0
// exactly -- not the rounding error of a round trip through the chain.
// RT_HD code: the gfx950 kernel (rt_motion.hip) and the host twin
// (tests/native/rt_motion_emu.cpp) compile this one source with
// -ffp-contract=off.
#ifndef RT_MOTION_H
#define RT_MOTION_H
#include <stddef.h>

#include "rt_live.h"
#include "rt_query.h"

namespace rtm {

using namespace rtq;

RT_HD RT_FI rt_motion miss_motion() {
  rt_motion m;
  m.d[0] = m.d[1] = m.d[2] = 0.0;
  m.dn[0] = m.dn[1] = m.dn[2] = 0.0;
  m.t = kInf;
  m.object = m.chain_object = -1;
  return m;
}

// rt_pixel_ray(frame, i, j): its operations in its order
RT_HD RT_FI rt_ray pixel_ray(const rt_frame &f, int i, int j) {
  const double x = (double)i, y = (double)j;
  const double c[3] = {f.center.x, f.center.y, f.center.z};
  const double p00[3] = {f.pixel00_loc.x, f.pixel00_loc.y, f.pixel00_loc.z};
  const double du[3] = {f.pixel_delta_u.x, f.pixel_delta_u.y, f.pixel_delta_u.z};
  const double dv[3] = {f.pixel_delta_v.x, f.pixel_delta_v.y, f.pixel_delta_v.z};
  rt_ray q;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q.origin[a] = c[a];
    q.direction[a] = p00[a] + x * du[a] + y * dv[a] - c[a];
  }
  q.time = 0.0;
  q.t_max = kInf;
  return q;
}

struct Placed {
  V3 p, n;
};
// anchor + q and the local normal nl through the chain xforms[f, f + n), innermost first
// (to_world's loop).  The kinds are the table's; the values of record r are the three
// doubles at vals + stride * r: the table's own (a, b, c) or a pose's.
RT_HD RT_FI Placed place(const DXform *xforms, const double *vals, int stride, int f, int n, V3 anchor, V3 q,
                         V3 nl) {
  Placed o{anchor + q, nl};
  for (int k = n - 1; k >= 0; --k) {
    const double *v = vals + (int64_t)stride * (f + k);
    if (xforms[f + k].kind == X_TRANSLATE) {
      o.p = o.p + v3(v[0], v[1], v[2]);
    } else {
      o.p = rot_out(v[0], v[1], o.p);
      o.n = rot_out(v[0], v[1], o.n);
    }
  }
  return o;
}
// a DXform's (a, b, c) as a row of doubles
constexpr int kXformStride = sizeof(DXform) / sizeof(double);
static_assert(sizeof(DXform) % sizeof(double) == 0 && offsetof(DXform, a) == sizeof(double) &&
                  offsetof(DXform, c) == 3 * sizeof(double),
              "DXform is a row of doubles");
RT_HD RT_FI const double *xform_values(const DXform *xforms) { return reinterpret_cast<const double *>(xforms) + 1; }

// The record of pixel (i, j).  pose: the earlier pose of this scene's tables (c its layout).
template <unsigned F>
RT_HD RT_FI rt_motion motion_pixel(const DScene &S, const int32_t *xf_obj, const rt_frame &frame,
                                   const rt_live::PoseCounts &c, const double *pose, int i, int j, int *stk) {
  static_assert(F == query_features(F), "a query instance has no media, lights or noise");
  rt_motion out = miss_motion();
  const rt_ray q = pixel_ray(frame, i, j);
  if (!ray_valid(q)) return out;
  const Ray r{ld3(q.origin), ld3(q.direction), q.time};
  double closest;
  int best;
  Counters cnt{};
  trace_closest<false, F>(S, r, closest, best, stk, (const RT_LDS DNode *)nullptr, cnt);
  if (best < 0 || !(closest <= kInf)) return out;
  const DItem it = S.items[best];
  int xf_first = 0, xf_count = 0;
  Ray lr = r;
  if constexpr ((F & F_XFORM) != 0) {
    if (it.xf_count) {
      xf_first = it.xf_first, xf_count = it.xf_count;
      lr = to_local(S, xf_first, xf_count, r);
    }
  }
  // the local record (trace_tail's item_record before to_world) and both anchors
  Hit h;
  V3 a_now, a_prev;
  if (it.kind == I_SPHERE) {
    const DSphere s = S.spheres[it.idx];
    sphere_record<true>(s, lr, closest, it.mat, h);
    a_now = ld3(s.c0);
    a_prev = ld3(rt_live::pose_sphere(c, pose, it.idx));
  } else {
    const DQuad &Q = S.quads[it.idx];
    quad_record(Q, lr, closest, it.mat, h);
    a_now = ld3(Q.Q);
    a_prev = ld3(rt_live::pose_quad(c, pose, it.idx));
  }
  const V3 off = h.p - a_now;
  const Placed now = place(S.xforms, xform_values(S.xforms), kXformStride, xf_first, xf_count, a_now, off, h.n);
  const Placed prev = place(S.xforms, rt_live::pose_xform(c, pose, 0), 3, xf_first, xf_count, a_prev, off, h.n);
  const V3 d = prev.p - now.p, dn = prev.n - now.n;
  out.d[0] = d.x, out.d[1] = d.y, out.d[2] = d.z;
  out.dn[0] = dn.x, out.dn[1] = dn.y, out.dn[2] = dn.z;
  out.t = h.t;
  out.object = it.id;
  if constexpr ((F & F_XFORM) != 0) {
    if (it.xf_count) out.chain_object = xf_obj[it.xf_first];
  }
  return out;
}

} // namespace rtm
#endif
