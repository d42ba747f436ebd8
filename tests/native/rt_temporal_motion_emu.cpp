// tests/native/rt_temporal_motion_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The motion forms of the two temporal twins (rt_temporal_emu.cpp,
// rt_temporal_variance_emu.cpp): csrc/rt_temporal.h temporal_motion_pixel and
// temporal_variance_motion_pixel on the host, one pixel at a time, with
// rt_temporal_motion_device's and rt_temporal_variance_motion_device's argument
// order and the parents' history layouts.  tests/test_motion.py holds them to
// rtx.temporal.NumpyOps(motion=) and, on an all-zero plane, to the parent
// twins' bytes; tests/test_temporal_motion_gpu.py holds the gfx950 kernels to
// them.  Built by temporal_motion.mk with g++ -ffp-contract=off.
#include "../../real-time-ray-tracing-engine_amd/csrc/rt_temporal.h"

#include <stddef.h>

using namespace rtt;

static size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t plane_bytes(const rt_frame *f) { return pad256((size_t)f->image_width * f->image_height * sizeof(F4)); }

static bool refused(const rt_frame *now, const double *rgb, const double *guides, int32_t guide_strata,
                    const rt_frame *prev, const void *history_prev, const rt_motion *motion,
                    const rt_temporal_params *params, const void *history_out, const double *out) {
  if (!now || !rgb || !guides || !history_out || !out || !motion || guide_strata < 1) return true;
  if ((prev == nullptr) != (history_prev == nullptr)) return true;
  const int W = now->image_width, H = now->image_height;
  if (W < 1 || H < 1 || (prev && (prev->image_width != W || prev->image_height != H))) return true;
  return params && params->max_history < 0;
}

// rt_temporal_motion_device on host memory; 0, or -1 on an argument that function refuses
extern "C" int emu_temporal_motion(const rt_frame *now, const double *rgb, double scale, const int32_t *tile_strata,
                                   int32_t strata_now, const double *guides, int32_t guide_strata,
                                   const rt_frame *prev, const void *history_prev, const rt_motion *motion,
                                   const rt_temporal_params *params, void *history_out, double *out) {
  if (refused(now, rgb, guides, guide_strata, prev, history_prev, motion, params, history_out, out)) return -1;
  const int W = now->image_width, H = now->image_height;
  const size_t plane = plane_bytes(now);
  const Coef K = coef_of(params);
  const char *hp = static_cast<const char *>(history_prev);
  char *ho = static_cast<char *>(history_out);
  const F4 *pcol = reinterpret_cast<const F4 *>(hp);
  const F4 *pgeo = hp ? reinterpret_cast<const F4 *>(hp + plane) : nullptr;
  const Cam cn = cam_of(*now), cp = cam_of(prev ? *prev : *now);
  for (int j = 0; j < H; ++j)
    for (int i = 0; i < W; ++i)
      temporal_motion_pixel(cn, cp, W, H, i, j, rgb, scale, tile_strata, strata_now, guides, (double)guide_strata,
                            pcol, pgeo, motion, K, reinterpret_cast<F4 *>(ho), reinterpret_cast<F4 *>(ho + plane),
                            out);
  return 0;
}

// rt_temporal_variance_motion_device on host memory
extern "C" int emu_temporal_variance_motion(const rt_frame *now, const double *rgb, double scale,
                                            const int32_t *tile_strata, int32_t strata_now, const double *guides,
                                            int32_t guide_strata, const rt_frame *prev, const void *history_prev,
                                            const rt_motion *motion, const double *variance_now,
                                            const rt_temporal_params *params, void *history_out, double *out,
                                            double *variance_out) {
  if (refused(now, rgb, guides, guide_strata, prev, history_prev, motion, params, history_out, out)) return -1;
  if (!variance_now || !variance_out || variance_out == variance_now) return -1;
  const int W = now->image_width, H = now->image_height;
  const size_t plane = plane_bytes(now);
  const Coef K = coef_of(params);
  const char *hp = static_cast<const char *>(history_prev);
  char *ho = static_cast<char *>(history_out);
  const F4 *pcol = reinterpret_cast<const F4 *>(hp);
  const F4 *pgeo = hp ? reinterpret_cast<const F4 *>(hp + plane) : nullptr;
  const float *pvar = hp ? reinterpret_cast<const float *>(hp + 2 * plane) : nullptr;
  const Cam cn = cam_of(*now), cp = cam_of(prev ? *prev : *now);
  for (int j = 0; j < H; ++j)
    for (int i = 0; i < W; ++i)
      temporal_variance_motion_pixel(cn, cp, W, H, i, j, rgb, scale, tile_strata, strata_now, guides,
                                     (double)guide_strata, pcol, pgeo, pvar, motion, K, reinterpret_cast<F4 *>(ho),
                                     reinterpret_cast<F4 *>(ho + plane), reinterpret_cast<float *>(ho + 2 * plane),
                                     out, variance_now, variance_out);
  return 0;
}
