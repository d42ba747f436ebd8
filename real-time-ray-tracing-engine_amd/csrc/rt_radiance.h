// rt_radiance.h — path-traced light along caller rays (rt_radiance_device;
// DESIGN.md §7o).
//
// Sample s of ray k is the render's own path: PathState{Ray{origin, direction,
// time}, T = 1, bounce = 0} run through segment<false, F, false, MS> (rt_path.h)
// until it ends, under Key{seed; first_key + k, first_sample + s} -- the
// render's range (0.001, inf), media draws, light sampling, max_depth rule
// (advance) and miss -> background; its value is the terminal ps.T.  A ray's
// samples are added in ascending s onto +0.0 (or onto the buffer's value:
// accumulate), each channel separately, by the one lane that owns the ray, so
// the sum is a property of the ray, its key and the tables alone.  RT_HD code
// like rt_query.h: the gfx950 kernel (rt_radiance.hip) and the host build
// (tests/native/rt_radiance_emu.cpp) compile this one source with
// -ffp-contract=off; the kernel runs radiance_trip under a __ballot, the host
// runs it to completion ray by ray.
#ifndef RT_RADIANCE_H
#define RT_RADIANCE_H
#include "rt_query.h"

namespace rtr {

using namespace rtq;

// The fields of rt_radiance_params a launch reads, as the kernel takes them
// (the background and max_depth travel in a DCamera, where segment reads them).
struct DRadiance {
  int64_t n;
  uint32_t seed_lo, seed_hi;
  uint32_t first_key;
  int32_t first_sample;
  int32_t samples;
  int32_t accumulate;
};
RT_HD RT_FI DRadiance radiance_launch(const rt_radiance_params &p, int64_t n) {
  return DRadiance{n,        (uint32_t)p.seed, (uint32_t)(p.seed >> 32), p.first_key, p.first_sample,
                   p.samples, p.accumulate};
}

// The DCamera of a radiance call: what segment and advance read of one, the
// background and the depth budget (the library and the host twin alike).
RT_HD RT_FI DCamera radiance_camera(const rt_radiance_params &p) {
  DCamera C{};
  C.bg[0] = p.background.x, C.bg[1] = p.background.y, C.bg[2] = p.background.z;
  C.max_depth = p.max_depth;
  return C;
}

// The material set of a scene's instance: render_instance's rule (rt_kernel.hip)
// -- the Lambertian-only twin for the plain flat world of a diffuse-only table.
RT_HD RT_FI bool diffuse_twin(int features) {
  return (features & RT_FEAT_DIFFUSE) && (unsigned)(features & F_ALL) == F_FLAT;
}

// `S` as the paths read it: nodes and the Perlin table from memory, as
// guide_scene / query_scene -- a block needs LDS for its traversal stacks only.
RT_HD RT_FI DScene radiance_scene(const DScene &S) { return query_scene(S); }

// One lane's state: the path of the sample it is on, that sample's key, the
// ray's three sums and the number of samples started.
struct RadianceState {
  PathState ps;
  Key key;
  double sum[3];
  int32_t next; // samples started so far; == samples: none left
};

// Ray k of the launch before its first trip.  px: the ray's three doubles in
// the output.  A ray that fails ray_valid's test of origin, direction and time
// (t_max is not read here, NaN or not) has no samples: it draws nothing and
// adds nothing.  max_depth <= 0: no sample runs a segment, every sample is 0.
RT_HD RT_FI RadianceState radiance_begin(const DCamera &C, const DRadiance &P, int64_t k, const rt_ray &q,
                                         const double *px) {
  RadianceState st;
  st.ps.active = false;
  st.ps.bounce = 0;
  st.ps.slot = 0;
  st.ps.sample = 0;
  st.key = Key{P.seed_lo, P.seed_hi, P.first_key + (uint32_t)k, 0u};
#pragma unroll
  for (int c = 0; c < 3; ++c) st.sum[c] = P.accumulate ? px[c] : 0.0;
  rt_ray v = q;
  v.t_max = 0.0; // ray_valid's own rule for t_max does not apply to a radiance ray
  st.next = (ray_valid(v) && C.max_depth > 0) ? 0 : P.samples;
  return st;
}

// Whether the lane has anything left: a path under way or a sample to start.
RT_HD RT_FI bool radiance_more(const RadianceState &st, const DRadiance &P) {
  return st.ps.active || st.next < P.samples;
}

// One trip of one lane.  An idle lane with samples left starts its next sample
// from the ray as it stands in memory (it is only read; not held in registers
// across the path); an active lane runs one segment; a lane whose path ended
// in this trip adds ps.T to its sums.  A lane with nothing left does nothing.
//
// Termination: every trip either raises an active lane's ps.bounce (shade's
// `return advance(...)`) or ends its path; advance ends a path once bounce
// reaches max_depth; a lane starts at most `samples` paths, one per trip in
// which it is idle.  So a lane makes at most samples * max_depth trips with a
// segment -- and the loop around this, which runs while any lane has
// radiance_more, at most samples * max_depth + samples trips.
template <unsigned F, MatSet MS>
RT_HD RT_FI void radiance_trip(const DScene &S, const DCamera &C, const DRadiance &P, const rt_ray *q,
                               RadianceState &st, int *stk) {
  if (!st.ps.active && st.next < P.samples) {
    st.key.sample = (uint32_t)(P.first_sample + st.next);
    ++st.next;
    st.ps.ray = Ray{ld3(q->origin), ld3(q->direction), q->time};
    st.ps.T = v3(1.0, 1.0, 1.0);
    st.ps.bounce = 0;
    st.ps.active = true; // max_depth > 0: radiance_begin
  }
  if (st.ps.active) {
    Counters cnt{};
    const bool cont = segment<false, F, false, MS>(S, C, st.ps, st.key, stk, (const RT_LDS DNode *)nullptr, cnt);
    if (!cont) {
      st.sum[0] += st.ps.T.x;
      st.sum[1] += st.ps.T.y;
      st.sum[2] += st.ps.T.z;
      st.ps.active = false;
    }
  }
}

// The host form: ray k to completion.  px is read (accumulate) and written once.
template <unsigned F, MatSet MS>
RT_HD RT_FI void radiance_ray(const DScene &S, const DCamera &C, const DRadiance &P, int64_t k, const rt_ray *q,
                              int *stk, double *px) {
  RadianceState st = radiance_begin(C, P, k, *q, px);
  while (radiance_more(st, P)) radiance_trip<F, MS>(S, C, P, q, st, stk);
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = st.sum[c];
}

} // namespace rtr
#endif
