// rt_guides.h — first-hit feature sums for the denoised display
// (rt_render_guides_device).
//
// One guide sample is the render's own camera ray of stratum k of pixel (i, j)
// -- the same Key{seed; pixel, k} and camera_ray as render_tiles, so jitter,
// defocus and ray time are the render's -- traced to its first hit with the
// render's trace<false, F> at bounce 0: a constant medium is hit or passed
// exactly where the render's primary segment hits or passes it.  No shading,
// no second segment.  RT_HD code like rt_path.h: the gfx950 kernel
// (rt_guides.hip) and the host build (tests/native/rt_guides_emu.cpp) compile
// this one source with -ffp-contract=off, which is what makes the device
// buffer reproducible on the host bit for bit.
#ifndef RT_GUIDES_H
#define RT_GUIDES_H
#include "rt_path.h"

namespace rtg {

using namespace rtp;

constexpr int kGuideChannels = 8; // RT_GUIDE_CHANNELS: albedo rgb, normal xyz, depth, hits

// The guide instance of a scene's feature bits: light sampling belongs to
// shading, which a guide sample never reaches.
constexpr unsigned guide_features(unsigned f) { return f & ~(unsigned)F_LIGHTS; }

// `S` as the guide walks read it: nodes and the Perlin table from memory
// (trace's and tex_value's own unstaged forms: rt_tuning.lds_nodes < 0,
// no_lds_perlin), so a guide block needs LDS for its traversal stacks only.
RT_HD RT_FI DScene guide_scene(const DScene &S) {
  DScene G = S;
  G.n_lds_nodes = 0;
  G.lds_perlin = 0;
  return G;
}

// Adds stratum k of pixel (i, j) to that pixel's eight sums g.
//   miss:                     albedo (1,1,1), normal 0, depth 0, hits 0
//   lambertian:               tex_value(M.tex, h.p), h.n, h.t |d|, 1
//   metal:                    M.albedo,              h.n, h.t |d|, 1
//   dielectric, diffuse_light (1,1,1),               h.n, h.t |d|, 1
//   isotropic (a medium):     tex_value(M.tex, h.p), 0,   h.t |d|, 1
template <unsigned F>
RT_HD RT_FI void guide_sample(const DScene &S, const DCamera &C, Key &key, int i, int j, int k, int *stk,
                              double g[kGuideChannels]) {
  key.pixel = (uint32_t)(j * C.W + i);
  key.sample = (uint32_t)k;
  const Ray r = camera_ray<RT_KB_F(F), RT_KCONST_MODE(F)>(C, key, i, j, k);
  Hit h;
  Counters cnt{};
  const bool hit = trace<false, F>(S, r, h, key, 0u, stk, (const RT_LDS DNode *)nullptr, cnt);
  V3 a = v3(1.0, 1.0, 1.0), n = v3(0.0, 0.0, 0.0);
  double depth = 0.0, hits = 0.0;
  if (hit) {
    const DMat M = S.mats[h.mat];
    if (M.kind == RT_MAT_LAMBERTIAN || M.kind == RT_MAT_ISOTROPIC) a = tex_value<F>(S, M.tex, h.p);
    else if (M.kind == RT_MAT_METAL) a = ld3(M.albedo);
    if (M.kind != RT_MAT_ISOTROPIC) n = h.n;
    depth = h.t * sqrt(len2(r.d));
    hits = 1.0;
  }
  g[0] += a.x;
  g[1] += a.y;
  g[2] += a.z;
  g[3] += n.x;
  g[4] += n.y;
  g[5] += n.z;
  g[6] += depth;
  g[7] += hits;
}

// Strata [s0, s0 + sc) of one pixel, in ascending order, onto the pixel's
// current sums (`accumulate`) or onto 0 -- the one place that fixes the order
// of the additions, so [0,4) equals [0,2) then [2,4) accumulated bit for bit.
template <unsigned F>
RT_HD RT_FI void guide_pixel(const DScene &S, const DCamera &C, uint32_t seed_lo, uint32_t seed_hi, int i,
                             int j, int s0, int sc, int accumulate, int *stk, double *px) {
  double g[kGuideChannels];
#pragma unroll
  for (int c = 0; c < kGuideChannels; ++c) g[c] = accumulate ? px[c] : 0.0;
  Key key{seed_lo, seed_hi, 0, 0};
  for (int k = s0; k < s0 + sc; ++k) guide_sample<F>(S, C, key, i, j, k, stk, g);
#pragma unroll
  for (int c = 0; c < kGuideChannels; ++c) px[c] = g[c];
}

} // namespace rtg
#endif
