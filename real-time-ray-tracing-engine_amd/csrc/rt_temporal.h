// rt_temporal.h — temporal reprojection of the displayed frame, one pixel
// (rt_temporal_device; statement of record: rtx/temporal.py NumpyOps.temporal,
// DESIGN.md §7e).
//
// RT_HD code: the gfx950 kernel (rt_temporal.hip) and the host twin
// (tests/native/rt_temporal_emu.cpp, g++) compile this one source, both with
// -ffp-contract=off.  Everything is fp64 except the history planes, which are
// two fp32 float4 planes: col (e.r, e.g, e.b, count) and geo (n.x, n.y, n.z, z).
// A pixel reads its own rgb / guides and at most four taps of the previous
// planes (two 16-B loads each) and writes its own col, geo and out once: no
// atomics, no shared memory, nothing read that another pixel writes.  A
// variance history (rt_temporal_variance_device) adds a third plane, var: the
// fp32 variance of e's luminance, one 4-B load per tap and one store.
#ifndef RT_TEMPORAL_H
#define RT_TEMPORAL_H
#include <math.h>
#include <stdint.h>

#include "../../include/rt_api.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef RT_HD // as rt_path.h defines them
#if defined(__HIPCC__)
#define RT_HD __host__ __device__
#define RT_FI __forceinline__
#else
#define RT_HD
#define RT_FI inline
#endif
#endif

namespace rtt {

struct alignas(16) F4 {
  float x, y, z, w;
};

struct D3 {
  double x, y, z;
};
RT_HD RT_FI D3 d3(const rt_vec3 &v) { return D3{v.x, v.y, v.z}; }
RT_HD RT_FI D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
RT_HD RT_FI D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RT_HD RT_FI D3 operator*(double t, D3 a) { return D3{t * a.x, t * a.y, t * a.z}; }
RT_HD RT_FI double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RT_HD RT_FI D3 cross(D3 a, D3 b) {
  return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// what the reprojection reads of an rt_frame
struct Cam {
  D3 c, p00, du, dv;
};
RT_HD RT_FI Cam cam_of(const rt_frame &f) {
  return Cam{d3(f.center), d3(f.pixel00_loc), d3(f.pixel_delta_u), d3(f.pixel_delta_v)};
}

// the resolved rt_temporal_params: a sigma < 0 is a test switched off
struct Coef {
  double max_history, sigma_z, sigma_n2, hit_min;
  int depth_on, normal_on;
};

// params may be null; zero fields take the RT_TEMPORAL_* defaults (the caller has refused max_history < 0)
inline Coef coef_of(const rt_temporal_params *params) {
  rt_temporal_params q{};
  if (params) q = *params;
  const double sz = q.sigma_depth == 0.0 ? RT_TEMPORAL_SIGMA_DEPTH : q.sigma_depth;
  const double sn = q.sigma_normal == 0.0 ? RT_TEMPORAL_SIGMA_NORMAL : q.sigma_normal;
  Coef K;
  K.max_history = (double)(q.max_history == 0 ? RT_TEMPORAL_MAX_HISTORY : q.max_history);
  K.sigma_z = sz;
  K.sigma_n2 = sn * sn;
  K.hit_min = q.hit_min == 0.0 ? RT_TEMPORAL_HIT_MIN : q.hit_min;
  K.depth_on = sz >= 0.0;
  K.normal_on = sn >= 0.0;
  return K;
}

// the first-hit point a pixel-centre ray of `C` reaches at distance z
RT_HD RT_FI D3 centre_point(const Cam &C, int i, int j, double z) {
  const D3 d = C.p00 + (double)i * C.du + (double)j * C.dv - C.c;
  return C.c + (z / sqrt(dot(d, d))) * d;
}

RT_HD RT_FI bool finite1(double x) { return fabs(x) < __builtin_huge_val(); }

// One pixel (i, j) of a W x H frame: the projection, the tap loop and the blend,
// stated once for temporal_pixel and temporal_variance_pixel.  pcol / pgeo: the
// previous history's planes, both null when there is none.  out may be rgb.
// VAR (rt_temporal_variance_device; rtx/temporal.py NumpyOps.temporal_variance,
// DESIGN.md §7g) carries the luminance variance of e beside the colour: pvar /
// ovar are the histories' third planes (fp32 scalars; pvar null with pcol),
// v_now / v_out [H][W] double planes.  Without VAR none of them is touched and
// the colour arithmetic is the same operations in the same order.
// MOT (rt_temporal_motion_device, rt_temporal_variance_motion_device; DESIGN.md
// §7q): `motion` is rt_motion_device's plane.  A surface pixel (|n|^2 >= 0.25)
// whose record is a hit and whose d and dn are not all zero projects P + d, tests
// n + dn against the taps' normals and the taps' points against the plane through
// P + d with normal (n + dn) / |n + dn|; every other pixel takes P and n
// themselves (selected, not added: P + 0 could turn a -0 into +0), so an all-zero
// plane gives the bits of the form without MOT.  What is written (geo = (n, z)
// included) is the current pose's.  Without MOT `motion` is not touched.
template <bool VAR, bool MOT = false>
RT_HD RT_FI void temporal_core(const Cam &now, const Cam &prev, int W, int H, int i, int j, const double *rgb,
                                 double scale, const int32_t *tile_strata, int strata_now,
                                 const double *guides, double g, const F4 *pcol, const F4 *pgeo,
                                 const float *pvar, const Coef &K, F4 *ocol, F4 *ogeo, double *out,
                                 const double *v_now, float *ovar, double *v_out,
                                 const rt_motion *motion = nullptr) {
  const int64_t p = (int64_t)j * W + i;
  double s = scale, n_c = (double)strata_now;
  if (tile_strata != nullptr) { // rt_to_bytes_tiles_device's scale; the tile's own count
    const int t = tile_strata[(j >> 3) * ((W + 7) >> 3) + (i >> 3)];
    s = 1.0 / (double)(t > 1 ? t : 1);
    n_c = (double)(t > 0 ? t : 0);
  }
  const double *G = guides + 8 * p;
  double e[3], ad[3];
  for (int c = 0; c < 3; ++c) {
    const double a = G[c] / g; // divisions, as the statement of record: h meets a threshold
    ad[c] = a > 0.01 ? a : 0.01;
    e[c] = rgb[3 * p + c] * s / ad[c];
  }
  const double hits = G[7];
  const double h = hits / g;
  const D3 n = D3{G[3] / g, G[4] / g, G[5] / g};
  const double z = G[6] / (hits > 1.0 ? hits : 1.0);

  double n_h = 0.0, eh[3] = {0.0, 0.0, 0.0}, v_h = 0.0;
  if (pcol != nullptr && h >= K.hit_min) {
    D3 P = centre_point(now, i, j, z);
    D3 nt = n; // the normal the taps' normals are held to
    bool moved = false;
    if (MOT) {
      const rt_motion m = motion[p];
      const D3 d = D3{m.d[0], m.d[1], m.d[2]}, dn = D3{m.dn[0], m.dn[1], m.dn[2]};
      moved = dot(n, n) >= 0.25 && m.object >= 0 &&
              (d.x != 0.0 || d.y != 0.0 || d.z != 0.0 || dn.x != 0.0 || dn.y != 0.0 || dn.z != 0.0);
      if (moved) {
        P = P + d;
        nt = n + dn;
      }
    }
    const D3 v = P - prev.c;
    const D3 Np = cross(prev.du, prev.dv);
    const double num = dot(prev.p00 - prev.c, Np), den = dot(v, Np);
    if (den * num > 0.0) {
      const D3 q = prev.c + (num / den) * v - prev.p00;
      const double x = dot(q, prev.du) / dot(prev.du, prev.du);
      const double y = dot(q, prev.dv) / dot(prev.dv, prev.dv);
      // a tap can only lie inside the image for x in (-1, W), y in (-1, H); NaN fails
      if (x > -1.0 && x < (double)W && y > -1.0 && y < (double)H) {
        const double r = sqrt(dot(v, v));
        const double fx = floor(x), fy = floor(y);
        const int x0 = (int)fx, y0 = (int)fy;
        const double wx = x - fx, wy = y - fy;
        const double nn = dot(n, n);
        const bool plane = nn >= 0.25;
        D3 nu = plane ? (1.0 / sqrt(nn)) * n : n;
        if (MOT) {
          if (moved) nu = (1.0 / sqrt(dot(nt, nt))) * nt;
        }
        double Wv = 0.0, cnt = 0.0, se[3] = {0.0, 0.0, 0.0}, sv = 0.0;
        for (int b = 0; b < 2; ++b) {
          const int qy = y0 + b;
          if (qy < 0 || qy >= H) continue;
          for (int a = 0; a < 2; ++a) {
            const int qx = x0 + a;
            if (qx < 0 || qx >= W) continue;
            const double w = (a ? wx : 1.0 - wx) * (b ? wy : 1.0 - wy);
            const int64_t t = (int64_t)qy * W + qx;
            const F4 cq = pcol[t], gq = pgeo[t];
            bool ok = cq.w > 0.0f && finite1((double)cq.x) && finite1((double)cq.y) && finite1((double)cq.z);
            if (K.normal_on) {
              const D3 dn = nt - D3{(double)gq.x, (double)gq.y, (double)gq.z};
              ok = ok && dot(dn, dn) <= K.sigma_n2;
            }
            if (K.depth_on) {
              const double zq = (double)gq.w;
              double dist;
              if (plane) {
                dist = fabs(dot(nu, centre_point(prev, qx, qy, zq) - P));
              } else {
                dist = fabs(zq - r);
              }
              ok = ok && dist <= K.sigma_z * r;
            }
            if (ok) {
              Wv += w;
              cnt += w * (double)cq.w;
              se[0] += w * (double)cq.x;
              se[1] += w * (double)cq.y;
              se[2] += w * (double)cq.z;
              if (VAR) { // linear, not w^2: neighbouring history pixels share taps
                const float vq = pvar[t];
                // a NaN or negative v': 0; a tap of weight 0 adds nothing (0 inf is not a variance)
                if (w > 0.0) sv += w * (double)(vq > 0.0f ? vq : 0.0f);
              }
            }
          }
        }
        if (Wv > 0.0) {
          n_h = cnt < K.max_history ? cnt : K.max_history;
          for (int c = 0; c < 3; ++c) eh[c] = se[c] / Wv;
          if (VAR) v_h = sv / Wv; // the cap bounds the count, not the variance
        }
      }
    }
  }

  const double total = n_h + n_c;
  double eo[3];
  bool fin = true;
  for (int c = 0; c < 3; ++c) {
    eo[c] = total > 0.0 ? (n_h * eh[c] + n_c * e[c]) / total : 0.0; // a non-finite e passes through
    fin = fin && finite1(eo[c]);
    out[3 * p + c] = eo[c] * ad[c];
  }
  const double count = (h >= K.hit_min && fin) ? total : 0.0;
  ocol[p] = F4{(float)eo[0], (float)eo[1], (float)eo[2], (float)count};
  ogeo[p] = F4{(float)n.x, (float)n.y, (float)n.z, (float)z};
  if (VAR) {
    const double vn = v_now[p];
    const double v_c = vn > 0.0 ? vn : 0.0; // a NaN or negative variance: 0
    double vo = 0.0;
    if (total > 0.0) { // a term whose count is 0 is dropped, not multiplied (0 inf)
      const double a = n_h / total, b = n_c / total;
      if (n_h > 0.0) vo = (a * a) * v_h;
      if (n_c > 0.0) vo = vo + (b * b) * v_c; // no history: b = 1, v_c itself
    }
    v_out[p] = vo;
    ovar[p] = count > 0.0 ? (float)vo : 0.0f;
  }
}

RT_HD RT_FI void temporal_pixel(const Cam &now, const Cam &prev, int W, int H, int i, int j, const double *rgb,
                                  double scale, const int32_t *tile_strata, int strata_now,
                                  const double *guides, double g, const F4 *pcol, const F4 *pgeo,
                                  const Coef &K, F4 *ocol, F4 *ogeo, double *out) {
  temporal_core<false>(now, prev, W, H, i, j, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo, nullptr, K,
                       ocol, ogeo, out, nullptr, nullptr, nullptr);
}

// temporal_pixel with the variance carried along: every colour output is
// temporal_pixel's, bit for bit.  v_out may not be v_now.
RT_HD RT_FI void temporal_variance_pixel(const Cam &now, const Cam &prev, int W, int H, int i, int j,
                                           const double *rgb, double scale, const int32_t *tile_strata,
                                           int strata_now, const double *guides, double g, const F4 *pcol,
                                           const F4 *pgeo, const float *pvar, const Coef &K, F4 *ocol, F4 *ogeo,
                                           float *ovar, double *out, const double *v_now, double *v_out) {
  temporal_core<true>(now, prev, W, H, i, j, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo, pvar, K,
                      ocol, ogeo, out, v_now, ovar, v_out);
}

// The two pixels above with object motion (temporal_core's MOT).
RT_HD RT_FI void temporal_motion_pixel(const Cam &now, const Cam &prev, int W, int H, int i, int j, const double *rgb,
                                         double scale, const int32_t *tile_strata, int strata_now,
                                         const double *guides, double g, const F4 *pcol, const F4 *pgeo,
                                         const rt_motion *motion, const Coef &K, F4 *ocol, F4 *ogeo, double *out) {
  temporal_core<false, true>(now, prev, W, H, i, j, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo,
                             nullptr, K, ocol, ogeo, out, nullptr, nullptr, nullptr, motion);
}
RT_HD RT_FI void temporal_variance_motion_pixel(const Cam &now, const Cam &prev, int W, int H, int i, int j,
                                                  const double *rgb, double scale, const int32_t *tile_strata,
                                                  int strata_now, const double *guides, double g, const F4 *pcol,
                                                  const F4 *pgeo, const float *pvar, const rt_motion *motion,
                                                  const Coef &K, F4 *ocol, F4 *ogeo, float *ovar, double *out,
                                                  const double *v_now, double *v_out) {
  temporal_core<true, true>(now, prev, W, H, i, j, rgb, scale, tile_strata, strata_now, guides, g, pcol, pgeo, pvar,
                            K, ocol, ogeo, out, v_now, ovar, v_out, motion);
}

} // namespace rtt
#endif
