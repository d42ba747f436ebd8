// rt_query.h — closest hits of caller rays (rt_trace_device).
//
// One query is the render's own closest-hit search (rt_path.h trace_closest)
// and hit record (trace_tail) for Ray{origin, direction, time}, with constant
// media masked out of the instance: no RNG key, no shading, no second
// segment.  What the record adds to the render's Hit is the vocabulary of the
// edit calls: DItem::id of the winning item and the object of the outermost
// transform above it.  RT_HD code like rt_guides.h: the gfx950 kernel
// (rt_query.hip) and the host build (tests/native/rt_query_emu.cpp) compile
// this one source with -ffp-contract=off, so the device records are
// reproducible on the host byte for byte.
#ifndef RT_QUERY_H
#define RT_QUERY_H
#include "rt_path.h"

namespace rtq {

using namespace rtp;

// The query instance of a scene's feature bits: what the search and the record
// read of them.  Media are not reported, lights belong to shading, noise to
// textures; F_BVH4 never comes with F_FLAT (rt_kernel.hip canonical).
constexpr unsigned query_features(unsigned f) {
  return f & ((f & F_FLAT) ? (F_XFORM | F_FLAT) : (F_XFORM | F_BVH4));
}

// `S` as the query walks read it: nodes from memory (trace's unstaged form,
// as rt_guides.h guide_scene), so a query block needs LDS for its traversal
// stacks only.
RT_HD RT_FI DScene query_scene(const DScene &S) {
  DScene Q = S;
  Q.n_lds_nodes = 0;
  Q.lds_perlin = 0;
  return Q;
}

// neither NaN nor +-inf, from the bits: no comparison for a compiler to fold
RT_HD RT_FI bool finite_bits(double x) {
  return (__builtin_bit_cast(uint64_t, x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// A ray that is traced: finite origin, direction and time, a direction that is
// not zero, a t_max that is not NaN.  Every other ray is a miss and never
// enters a traversal loop.
RT_HD RT_FI bool ray_valid(const rt_ray &q) {
  bool ok = finite_bits(q.time) && q.t_max == q.t_max;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && finite_bits(q.origin[a]) && finite_bits(q.direction[a]);
  return ok && (q.direction[0] != 0.0 || q.direction[1] != 0.0 || q.direction[2] != 0.0);
}

RT_HD RT_FI rt_ray_hit miss_record() {
  rt_ray_hit m;
  m.t = kInf;
  m.p[0] = m.p[1] = m.p[2] = 0.0;
  m.n[0] = m.n[1] = m.n[2] = 0.0;
  m.object = m.chain_object = m.material = -1;
  m.front = 0;
  return m;
}

// The record of one ray.  xf_obj: per xforms[] record the object it came from
// (rt_scene.h xform_objects).  t_max is compared with the search's minimum
// afterwards: the search itself is the render's, unlimited.
template <unsigned F>
RT_HD RT_FI rt_ray_hit query_ray(const DScene &S, const int32_t *xf_obj, const rt_ray &q, int *stk) {
  static_assert(F == query_features(F), "a query instance has no media, lights or noise");
  rt_ray_hit out = miss_record();
  if (!ray_valid(q)) return out;
  const Ray r{ld3(q.origin), ld3(q.direction), q.time};
  const double limit = q.t_max > 0.0 ? q.t_max : kInf;
  double closest;
  int best;
  Counters cnt{};
  trace_closest<false, F>(S, r, closest, best, stk, (const RT_LDS DNode *)nullptr, cnt);
  if (best < 0 || !(closest <= limit)) return out;
  Hit h;
  trace_tail<false, F>(S, r, h, Key{}, 0u, closest, best, cnt);
  const DItem it = S.items[best];
  out.t = h.t;
  out.p[0] = h.p.x, out.p[1] = h.p.y, out.p[2] = h.p.z;
  out.n[0] = h.n.x, out.n[1] = h.n.y, out.n[2] = h.n.z;
  out.object = it.id;
  out.chain_object = -1;
  if constexpr ((F & F_XFORM) != 0) {
    if (it.xf_count) out.chain_object = xf_obj[it.xf_first];
  }
  out.material = h.mat;
  out.front = h.front ? 1 : 0;
  return out;
}

} // namespace rtq
#endif
