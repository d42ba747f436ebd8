// tests/native/rt_temporal_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The temporal reprojection's own per-pixel source (real-time-ray-tracing-
// engine_amd/csrc/rt_temporal.h: temporal_pixel) on the host, one pixel at a
// time -- the host twin of rt_temporal.hip, with rt_temporal_device's argument
// order and history layout (two float4 planes, each padded to 256 B).
// tests/test_temporal.py holds it to rtx.temporal.NumpyOps;
// tests/test_temporal_gpu.py holds the gfx950 kernel to it.  Built by
// temporal.mk with g++ -ffp-contract=off: as a shared library for the tests,
// and with -DRT_TEMPORAL_MAIN as a stand-alone program that runs a random case
// with a moved camera, for `make sanitize` (ASan + UBSan).
#include "../../real-time-ray-tracing-engine_amd/csrc/rt_temporal.h"

#include <stddef.h>

using namespace rtt;

static size_t plane_bytes(const rt_frame *f) {
  return (((size_t)f->image_width * f->image_height * sizeof(F4)) + 255) & ~(size_t)255;
}

extern "C" int64_t emu_history_bytes(const rt_frame *f) { return (int64_t)(2 * plane_bytes(f)); }

// rt_temporal_device on host memory; 0, or -1 on an argument rt_temporal_device refuses
extern "C" int emu_temporal(const rt_frame *now, const double *rgb, double scale, const int32_t *tile_strata,
                            int32_t strata_now, const double *guides, int32_t guide_strata, const rt_frame *prev,
                            const void *history_prev, const rt_temporal_params *params, void *history_out,
                            double *out) {
  if (!now || !rgb || !guides || !history_out || !out || guide_strata < 1) return -1;
  if ((prev == nullptr) != (history_prev == nullptr)) return -1;
  const int W = now->image_width, H = now->image_height;
  if (W < 1 || H < 1 || (prev && (prev->image_width != W || prev->image_height != H))) return -1;
  if (params && params->max_history < 0) return -1;
  const size_t plane = plane_bytes(now);
  const Coef K = coef_of(params);
  const F4 *pcol = static_cast<const F4 *>(history_prev);
  const F4 *pgeo = history_prev ? reinterpret_cast<const F4 *>(static_cast<const char *>(history_prev) + plane)
                                : nullptr;
  F4 *ocol = static_cast<F4 *>(history_out);
  F4 *ogeo = reinterpret_cast<F4 *>(static_cast<char *>(history_out) + plane);
  const Cam cn = cam_of(*now), cp = cam_of(prev ? *prev : *now);
  for (int j = 0; j < H; ++j)
    for (int i = 0; i < W; ++i)
      temporal_pixel(cn, cp, W, H, i, j, rgb, scale, tile_strata, strata_now, guides, (double)guide_strata, pcol,
                     pgeo, K, ocol, ogeo, out);
  return 0;
}

#ifdef RT_TEMPORAL_MAIN
// The sanitizer stage: exactly-sized heap buffers (no padding beyond the
// planes' own), a random 70 x 33 case in the manner of tests/test_denoise.py
// random_case, a first history at pose A, then pose B (a lateral step and a
// yaw, so that taps fall off every image border) with and without tile strata,
// and a half turn (nothing in front of the previous camera).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static double u01(uint64_t &s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) * (1.0 / 9007199254740992.0);
}

static rt_frame pinhole(int W, int H, double cx, double yaw) {
  rt_frame f;
  memset(&f, 0, sizeof f);
  f.image_width = W;
  f.image_height = H;
  f.sqrt_spp = 2;
  f.max_depth = 8;
  f.pixel_samples_scale = 0.25;
  const double px = 2.0 / W; // a viewport 2 wide at distance 1
  const double c = cos(yaw), s = sin(yaw);
  const rt_vec3 right = {c, 0.0, -s}, fwd = {-s, 0.0, -c};
  f.center = rt_vec3{cx, 0.0, 0.0};
  f.pixel_delta_u = rt_vec3{px * right.x, 0.0, px * right.z};
  f.pixel_delta_v = rt_vec3{0.0, -px, 0.0};
  f.pixel00_loc = rt_vec3{cx + fwd.x - 0.5 * (W - 1) * f.pixel_delta_u.x, 0.5 * (H - 1) * px,
                          fwd.z - 0.5 * (W - 1) * f.pixel_delta_u.z};
  return f;
}

int main() {
  const int W = 70, H = 33, g = 4;
  uint64_t seed = 11;
  std::vector<double> rgb((size_t)W * H * 3), guides((size_t)W * H * 8), out((size_t)W * H * 3);
  for (double &v : rgb) v = 2.0 * g * u01(seed);
  for (int p = 0; p < W * H; ++p) {
    double *G = &guides[8 * (size_t)p];
    const int i = p % W, j = p / W;
    const double hits = (j < H / 4 && i < W / 5) ? 0.0 : (j == H / 4 ? g / 2.0 : (double)g);
    for (int c = 0; c < 3; ++c) G[c] = hits > 0 ? g * (0.2 + 0.7 * u01(seed)) : (double)g;
    G[3] = i < W / 2 ? 0.0 : hits;
    G[5] = i < W / 2 ? hits : 0.0;
    G[6] = hits * (5.0 + 0.02 * i + (j > H / 2 ? 0.3 : 0.0));
    G[7] = hits;
    if (i == 40 && j == 20) rgb[3 * (size_t)p + 1] = __builtin_nan(""); // a NaN sample passes through
  }
  std::vector<int32_t> tiles((size_t)((W + 7) / 8) * ((H + 7) / 8));
  for (size_t t = 0; t < tiles.size(); ++t) tiles[t] = (int32_t)((t * 7) % 6);
  const rt_frame A = pinhole(W, H, 0.0, 0.0), B = pinhole(W, H, 0.4, 0.05), T = pinhole(W, H, 0.0, 3.14159265358979);
  const size_t hb = (size_t)emu_history_bytes(&A);
  char *h0 = static_cast<char *>(aligned_alloc(256, hb)), *h1 = static_cast<char *>(aligned_alloc(256, hb));
  int rc = emu_temporal(&A, rgb.data(), 1.0 / g, nullptr, g, guides.data(), g, nullptr, nullptr, nullptr, h0,
                        out.data());
  rt_temporal_params off;
  memset(&off, 0, sizeof off);
  off.sigma_depth = off.sigma_normal = off.hit_min = -1.0;
  const rt_temporal_params *ps[2] = {nullptr, &off};
  double sum = 0.0;
  size_t kept = 0;
  for (const rt_frame *f : {&B, &A, &T})
    for (const rt_temporal_params *p : ps)
      for (const int32_t *ts : {(const int32_t *)nullptr, (const int32_t *)tiles.data()}) {
        rc |= emu_temporal(f, rgb.data(), 1.0 / g, ts, 1, guides.data(), g, &A, h0, p, h1, out.data());
        const F4 *col = reinterpret_cast<const F4 *>(h1);
        for (int q = 0; q < W * H; ++q) {
          kept += col[q].w > 1.5f;
          if (out[3 * (size_t)q] == out[3 * (size_t)q]) sum += out[3 * (size_t)q];
        }
      }
  rc |= emu_temporal(&B, out.data(), 1.0, nullptr, 1, guides.data(), g, &A, h0, nullptr, h1, out.data()); // in place
  free(h0);
  free(h1);
  printf("rt_temporal_emu: rc %d, %zu pixels kept history, checksum %.6f\n", rc, kept, sum);
  return rc != 0 || kept == 0;
}
#endif
