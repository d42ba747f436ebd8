// rt_denoise.hip — edge-avoiding a-trous filter of the displayed frame
// (rt_denoise_device; statement of record: rtx/denoise.py NumpyOps.denoise,
// DESIGN.md §7d).
//
// The fp64 accumulator is read once and never written.  `prepare` demodulates
// the scaled frame by the first-hit albedo and packs what the passes need into
// the caller's workspace as fp32, 64 B per pixel in four float4 planes:
//   col[0], col[1]  (e.r, e.g, e.b, h)   the ping-pong pair; h = hits / g rides
//                                        along so a tap is two 16-B loads
//   geo             (n.x, n.y, n.z, z)   mean normal (not renormalised), mean hit depth
//   alb             (a_d.r, a_d.g, a_d.b, 0)  the remodulation factor max(a, 0.01)
// Pass k gathers the 5x5 B3-spline taps at step 2^k: one lane per pixel, no
// atomics, blocks of 64 x 4 pixels so that every tap of a wavefront is one
// contiguous 64-pixel row segment (a coalesced 16-B-per-lane load) whatever
// the step.  One native fp32 exponential per tap.  The last pass multiplies by
// a_d and widens to the fp64 output.
//
// The variance-guided filter (rt_denoise_variance_device) follows below: the
// same passes with the colour term normalised by the standard deviation of the
// pixel's estimate, 68 B per pixel; geo_terms / edge_weight / luma state the
// tap code once for both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"

namespace {

constexpr int kBX = 64, kBY = 4;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

__global__ void __launch_bounds__(256)
    denoise_prepare_kernel(const double *rgb, double scale, const int32_t *tile_strata, const double *guides,
                           double inv_g, int W, int H, int tiles_x, float4 *col, float4 *geo, float4 *alb) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  double s = scale;
  if (tile_strata != nullptr) { // rt_to_bytes_tiles_device's scale
    const int i = (int)(p % W), j = (int)(p / W);
    s = 1.0 / (double)max(1, tile_strata[(j >> 3) * tiles_x + (i >> 3)]);
  }
  const double *G = guides + 8 * p;
  float e[3], ad[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = G[c] * inv_g;
    const double a_d = a > 0.01 ? a : 0.01; // max(a, 0.01)
    e[c] = (float)(rgb[3 * p + c] * s / a_d);
    ad[c] = (float)a_d;
  }
  const double hits = G[7];
  col[p] = make_float4(e[0], e[1], e[2], (float)(hits * inv_g));
  geo[p] = make_float4((float)(G[3] * inv_g), (float)(G[4] * inv_g), (float)(G[5] * inv_g),
                       (float)(G[6] / (hits > 1.0 ? hits : 1.0)));
  alb[p] = make_float4(ad[0], ad[1], ad[2], 0.0f);
}

// the edge-stopping coefficients of one pass; a term that is off has coefficient 0
struct PassCoef {
  float inv_sn2; // 1 / sigma_n^2
  float inv_sz;  // 1 / sigma_z
  float inv_sh2; // 1 / sigma_h^2
  float inv_sc2; // 1 / (sigma_c 2^-k)^2
};

// the normal, depth and hit terms of one tap at distance d = step max(|di|, |dj|)
__device__ __forceinline__ float geo_terms(const float4 gp, const float4 gq, float hp, float hq, float d,
                                           const PassCoef K) {
  const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
  float t = (nx * nx + ny * ny + nz * nz) * K.inv_sn2;
  t += __fdividef(fabsf(gp.w - gq.w) * K.inv_sz, fmaxf(fmaxf(gp.w, gq.w), 1e-30f) * d);
  const float dh = hp - hq;
  t += dh * dh * K.inv_sh2;
  return t;
}

// exp(-min(t, 80)); a NaN exponent: no weight (fminf would give 80)
__device__ __forceinline__ float edge_weight(float t) {
  const float w = __expf(-fminf(t, 80.0f));
  return t == t ? w : 0.0f;
}

__device__ __forceinline__ float luma(const float4 e) { return 0.2126f * e.x + 0.7152f * e.y + 0.0722f * e.z; }

__global__ void __launch_bounds__(kBX *kBY)
    denoise_pass_kernel(const float4 *__restrict__ in, const float4 *__restrict__ geo,
                        const float4 *__restrict__ alb, int W, int H, int step, PassCoef K,
                        float4 *__restrict__ out, double *__restrict__ out_rgb) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  const int64_t p = (int64_t)y * W + x;
  const float4 ep = in[p], gp = geo[p];
  const bool p_ok = finite3(ep.x, ep.y, ep.z);
  const float yp = luma(ep);
  // the colour term's per-pixel factor; a non-finite centre has no colour term
  const float cw = p_ok ? __fdividef(K.inv_sc2, yp * yp + 1e-4f) : 0.0f;
  const float b[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
  for (int dj = -2; dj <= 2; ++dj) {
    const int qy = y + dj * step;
    if (qy < 0 || qy >= H) continue; // wave-uniform: a wave is one row segment
#pragma unroll
    for (int di = -2; di <= 2; ++di) {
      const int qx = x + di * step;
      if (qx < 0 || qx >= W) continue;
      float w = b[di + 2] * b[dj + 2];
      float4 eq = ep;
      if (di != 0 || dj != 0) {
        const int64_t q = (int64_t)qy * W + qx;
        eq = in[q];
        const float4 gq = geo[q];
        float t = geo_terms(gp, gq, ep.w, eq.w, (float)(step * max(abs(di), abs(dj))), K);
        const float cr = ep.x - eq.x, cg = ep.y - eq.y, cb = ep.z - eq.z;
        t += p_ok ? (cr * cr + cg * cg + cb * cb) * cw : 0.0f;
        w *= edge_weight(t);
      }
      if (!finite3(eq.x, eq.y, eq.z)) w = 0.0f;
      if (w > 0.0f) {
        sw += w;
        sr += w * eq.x;
        sg += w * eq.y;
        sb += w * eq.z;
      }
    }
  }
  float4 r = ep; // no weight at all: the pixel keeps its own value
  if (sw > 0.0f) {
    const float inv = 1.0f / sw;
    r = make_float4(sr * inv, sg * inv, sb * inv, ep.w);
  }
  if (out_rgb != nullptr) { // the last pass: remodulate, widen
    const float4 a = alb[p];
    out_rgb[3 * p + 0] = (double)r.x * (double)a.x;
    out_rgb[3 * p + 1] = (double)r.y * (double)a.y;
    out_rgb[3 * p + 2] = (double)r.z * (double)a.z;
  } else {
    out[p] = r;
  }
}

// passes < 0: prepare + remodulate only
__global__ void __launch_bounds__(256)
    denoise_remodulate_kernel(const float4 *col, const float4 *alb, int64_t n, double *out_rgb) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float4 e = col[p], a = alb[p];
  out_rgb[3 * p + 0] = (double)e.x * (double)a.x;
  out_rgb[3 * p + 1] = (double)e.y * (double)a.y;
  out_rgb[3 * p + 2] = (double)e.z * (double)a.z;
}

// ---- the variance-guided filter (rt_denoise_variance_device; statement of
// record: rtx/denoise.py NumpyOps.denoise_variance) ----------
// 68 B per pixel: the four float4 planes above with the variance v of e's
// luminance in the w slot of the ping-pong pair, col = (e.r, e.g, e.b, v), and
// h moved to a float plane of its own, so a tap stays 36 B (16 + 16 + 4).

// prepare, and v from the batch moments where the pixel's tile has enough
// batches (tile_batches >= min_batches >= 2; fp64, rounded once); 0 elsewhere:
// variance_spatial_kernel fills those in
__global__ void __launch_bounds__(256)
    variance_prepare_kernel(const double *rgb, double scale, const int32_t *tile_strata, const double *guides,
                            double inv_g, const double *s1, const double *s2, int batch_strata, int min_batches,
                            int W, int H, int tiles_x, float4 *col, float4 *geo, float4 *alb, float *hit) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  double s = scale;
  int strata = 0;
  if (tile_strata != nullptr) {
    const int i = (int)(p % W), j = (int)(p / W);
    strata = tile_strata[(j >> 3) * tiles_x + (i >> 3)];
    s = 1.0 / (double)max(1, strata);
  }
  const double *G = guides + 8 * p;
  float e[3];
  double ad[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = G[c] * inv_g;
    ad[c] = a > 0.01 ? a : 0.01;
    e[c] = (float)(rgb[3 * p + c] * s / ad[c]);
  }
  float v = 0.0f;
  if (s1 != nullptr && finite3(e[0], e[1], e[2])) {
    const int b = strata / batch_strata;
    if (b >= min_batches) {
      const double fb = (double)b, a1 = s1[p], a2 = s2[p];
      double var = (a2 - a1 * a1 / fb) / (fb - 1.0);
      var = var > 0.0 ? var : 0.0; // a NaN moment: 0
      const double la = 0.2126 * ad[0] + 0.7152 * ad[1] + 0.0722 * ad[2];
      v = (float)(var / fb / (la * la));
    }
  }
  const double hits = G[7];
  col[p] = make_float4(e[0], e[1], e[2], v);
  geo[p] = make_float4((float)(G[3] * inv_g), (float)(G[4] * inv_g), (float)(G[5] * inv_g),
                       (float)(G[6] / (hits > 1.0 ? hits : 1.0)));
  alb[p] = make_float4((float)ad[0], (float)ad[1], (float)ad[2], 0.0f);
  hit[p] = (float)(hits * inv_g);
}

// variance_prepare_kernel with v given by the caller (rt_denoise_given_variance_device,
// DESIGN.md §7g): the moments block is one load; a NaN or negative value is 0,
// and so is v where e is not finite.  Nothing is left for variance_spatial_kernel.
__global__ void __launch_bounds__(256)
    variance_prepare_given_kernel(const double *rgb, double scale, const int32_t *tile_strata, const double *guides,
                                  double inv_g, const double *variance, int W, int H, int tiles_x, float4 *col,
                                  float4 *geo, float4 *alb, float *hit) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  double s = scale;
  if (tile_strata != nullptr) {
    const int i = (int)(p % W), j = (int)(p / W);
    s = 1.0 / (double)max(1, tile_strata[(j >> 3) * tiles_x + (i >> 3)]);
  }
  const double *G = guides + 8 * p;
  float e[3];
  double ad[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = G[c] * inv_g;
    ad[c] = a > 0.01 ? a : 0.01;
    e[c] = (float)(rgb[3 * p + c] * s / ad[c]);
  }
  const double vp = variance[p];
  const float v = (vp > 0.0 && finite3(e[0], e[1], e[2])) ? (float)vp : 0.0f;
  const double hits = G[7];
  col[p] = make_float4(e[0], e[1], e[2], v);
  geo[p] = make_float4((float)(G[3] * inv_g), (float)(G[4] * inv_g), (float)(G[5] * inv_g),
                       (float)(G[6] / (hits > 1.0 ? hits : 1.0)));
  alb[p] = make_float4((float)ad[0], (float)ad[1], (float)ad[2], 0.0f);
  hit[p] = (float)(hits * inv_g);
}

// three floats of a col entry: the spatial kernel reads e while other lanes
// store their own v beside it, so it never touches the w slot of another pixel
__device__ __forceinline__ float4 load_e(const float4 *col, int64_t q) {
  const float *c = reinterpret_cast<const float *>(col + q);
  return make_float4(c[0], c[1], c[2], 0.0f);
}

// v of the pixels without enough batches: the weighted variance of y over the
// 7x7 window at step 1.  One lane per pixel in 64 x 4 blocks as the passes, so
// a tap of a wavefront is one row segment; the moments / spatial choice is per
// 8x8 tile: uniform over 8-lane spans, and a wave whose tiles all have moments
// leaves at once.  Moments of d = y_q - y_p: exact on a flat window.
__global__ void __launch_bounds__(kBX *kBY)
    variance_spatial_kernel(float4 *col, const float4 *__restrict__ geo, const float *__restrict__ hit,
                            const int32_t *tile_strata, int batch_strata, int min_batches, int W, int H,
                            int tiles_x, PassCoef K) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  if (batch_strata > 0 && tile_strata[(y >> 3) * tiles_x + (x >> 3)] / batch_strata >= min_batches) return;
  const int64_t p = (int64_t)y * W + x;
  const float4 ep = load_e(col, p), gp = geo[p];
  if (!finite3(ep.x, ep.y, ep.z)) return; // v stays 0
  const float hp = hit[p], yp = luma(ep);
  float sw = 1.0f, m1 = 0.0f, m2 = 0.0f; // the centre: weight 1, d = 0
#pragma unroll
  for (int dj = -3; dj <= 3; ++dj) {
    const int qy = y + dj;
    if (qy < 0 || qy >= H) continue;
#pragma unroll
    for (int di = -3; di <= 3; ++di) {
      const int qx = x + di;
      if (qx < 0 || qx >= W || (di == 0 && dj == 0)) continue;
      const int64_t q = (int64_t)qy * W + qx;
      const float4 eq = load_e(col, q);
      if (!finite3(eq.x, eq.y, eq.z)) continue;
      const float w = edge_weight(geo_terms(gp, geo[q], hp, hit[q], (float)max(abs(di), abs(dj)), K));
      if (w > 0.0f) {
        const float d = luma(eq) - yp;
        sw += w;
        m1 += w * d;
        m2 += w * d * d;
      }
    }
  }
  const float inv = 1.0f / sw, m = m1 * inv;
  const float v = m2 * inv - m * m;
  reinterpret_cast<float *>(col + p)[3] = v > 0.0f ? v : 0.0f;
}

// denoise_pass_kernel with the colour term |y_p - y_q| / (sigma_l sqrt(v~_p) + 1e-6),
// v~ the 3x3 Gaussian of v over the finite in-image neighbours (sigma_l <= 0:
// term off, no blur), and v carried along: v' = sum w^2 v_q / (sum w)^2
__global__ void __launch_bounds__(kBX *kBY)
    variance_pass_kernel(const float4 *__restrict__ in, const float4 *__restrict__ geo,
                         const float *__restrict__ hit, const float4 *__restrict__ alb, int W, int H, int step,
                         PassCoef K, float sigma_l, float4 *__restrict__ out, double *__restrict__ out_rgb,
                         double *__restrict__ out_var) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  const int64_t p = (int64_t)y * W + x;
  const float4 ep = in[p], gp = geo[p];
  const float hp = hit[p];
  const bool p_ok = finite3(ep.x, ep.y, ep.z);
  const float yp = luma(ep);
  float cw = 0.0f; // a non-finite centre has no colour term
  if (sigma_l > 0.0f && p_ok) {
    const float g3[3] = {0.25f, 0.5f, 0.25f};
    float sg = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      const int qy = y + dj;
      if (qy < 0 || qy >= H) continue;
#pragma unroll
      for (int di = -1; di <= 1; ++di) {
        const int qx = x + di;
        if (qx < 0 || qx >= W) continue;
        const float4 c = (di != 0 || dj != 0) ? in[(int64_t)qy * W + qx] : ep;
        if (!finite3(c.x, c.y, c.z)) continue;
        const float g = g3[di + 1] * g3[dj + 1];
        sg += g;
        sv += g * c.w;
      }
    }
    cw = 1.0f / (sigma_l * sqrtf(sv / sg) + 1e-6f); // sg >= 1/4: the centre is finite
  }
  const float b[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dj = -2; dj <= 2; ++dj) {
    const int qy = y + dj * step;
    if (qy < 0 || qy >= H) continue; // wave-uniform: a wave is one row segment
#pragma unroll
    for (int di = -2; di <= 2; ++di) {
      const int qx = x + di * step;
      if (qx < 0 || qx >= W) continue;
      float w = b[di + 2] * b[dj + 2];
      float4 eq = ep;
      if (di != 0 || dj != 0) {
        const int64_t q = (int64_t)qy * W + qx;
        eq = in[q];
        float t = geo_terms(gp, geo[q], hp, hit[q], (float)(step * max(abs(di), abs(dj))), K);
        t += p_ok ? fabsf(yp - luma(eq)) * cw : 0.0f;
        w *= edge_weight(t);
      }
      if (!finite3(eq.x, eq.y, eq.z)) w = 0.0f;
      if (w > 0.0f) {
        sw += w;
        sr += w * eq.x;
        sg += w * eq.y;
        sb += w * eq.z;
        sv += w * w * eq.w;
      }
    }
  }
  float4 r = ep; // no weight at all: the pixel keeps its own value and variance
  if (sw > 0.0f) {
    const float inv = 1.0f / sw;
    r = make_float4(sr * inv, sg * inv, sb * inv, sv * (inv * inv));
  }
  if (out_rgb != nullptr) { // the last pass: remodulate, widen
    const float4 a = alb[p];
    out_rgb[3 * p + 0] = (double)r.x * (double)a.x;
    out_rgb[3 * p + 1] = (double)r.y * (double)a.y;
    out_rgb[3 * p + 2] = (double)r.z * (double)a.z;
    if (out_var != nullptr) out_var[p] = (double)r.w;
  } else {
    out[p] = r;
  }
}

// passes < 0: prepare + remodulate only
__global__ void __launch_bounds__(256)
    variance_remodulate_kernel(const float4 *col, const float4 *alb, int64_t n, double *out_rgb, double *out_var) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float4 e = col[p], a = alb[p];
  out_rgb[3 * p + 0] = (double)e.x * (double)a.x;
  out_rgb[3 * p + 1] = (double)e.y * (double)a.y;
  out_rgb[3 * p + 2] = (double)e.z * (double)a.z;
  if (out_var != nullptr) out_var[p] = (double)e.w;
}

} // namespace

static size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t rtk_denoise_variance_workspace_bytes(int W, int H) {
  return 4 * pad256((size_t)W * H * sizeof(float4)) + pad256((size_t)W * H * sizeof(float));
}

namespace {

// the workspace's planes
struct VarianceWs {
  float4 *col[2], *geo, *alb;
  float *hit;
};
VarianceWs variance_ws(void *workspace, int64_t n) {
  const size_t plane = pad256((size_t)n * sizeof(float4));
  char *ws = static_cast<char *>(workspace);
  return VarianceWs{{reinterpret_cast<float4 *>(ws), reinterpret_cast<float4 *>(ws + plane)},
                    reinterpret_cast<float4 *>(ws + 2 * plane), reinterpret_cast<float4 *>(ws + 3 * plane),
                    reinterpret_cast<float *>(ws + 4 * plane)};
}

PassCoef variance_coef(double sigma_n, double sigma_z, double sigma_h) {
  PassCoef K;
  K.inv_sn2 = sigma_n > 0 ? (float)(1.0 / (sigma_n * sigma_n)) : 0.0f;
  K.inv_sz = sigma_z > 0 ? (float)(1.0 / sigma_z) : 0.0f;
  K.inv_sh2 = sigma_h > 0 ? (float)(1.0 / (sigma_h * sigma_h)) : 0.0f;
  K.inv_sc2 = 0.0f;
  return K;
}

// the passes (or, passes <= 0, the remodulation alone) over a prepared workspace whose col[0] holds v
hipError_t variance_passes(const VarianceWs &ws, int W, int H, int passes, PassCoef K, double sigma_l, double *out,
                           double *var_out, hipStream_t stream) {
  const int64_t n = (int64_t)W * H;
  if (passes <= 0) {
    hipLaunchKernelGGL(variance_remodulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       ws.col[0], ws.alb, n, out, var_out);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
  for (int k = 0; k < passes; ++k) {
    const bool last = k == passes - 1;
    hipLaunchKernelGGL(variance_pass_kernel, grid, dim3(kBX * kBY), 0, stream, ws.col[k & 1], ws.geo, ws.hit, ws.alb,
                       W, H, 1 << k, K, sigma_l > 0 ? (float)sigma_l : 0.0f, ws.col[(k & 1) ^ 1],
                       last ? out : nullptr, last ? var_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace

extern "C" hipError_t rtk_launch_denoise_variance(int W, int H, const double *rgb, double scale,
                                                  const int32_t *tile_strata, const double *guides,
                                                  int guide_strata, const double *s1, const double *s2,
                                                  int batch_strata, int min_batches, int passes, double sigma_n,
                                                  double sigma_z, double sigma_h, double sigma_l, void *workspace,
                                                  double *out, double *var_out, hipStream_t stream) {
  const int64_t n = (int64_t)W * H;
  if (n <= 0) return hipSuccess;
  const VarianceWs ws = variance_ws(workspace, n);
  const int tiles_x = (W + 7) / 8;
  if (!(s1 && s2 && tile_strata && batch_strata >= 1)) { // no moments: every pixel takes the spatial estimate
    s1 = s2 = nullptr;
    batch_strata = 0;
  }
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(variance_prepare_kernel, dim3(blocks), dim3(256), 0, stream, rgb, scale, tile_strata, guides,
                     1.0 / (double)guide_strata, s1, s2, batch_strata, min_batches, W, H, tiles_x, ws.col[0], ws.geo,
                     ws.alb, ws.hit);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const PassCoef K = variance_coef(sigma_n, sigma_z, sigma_h);
  const dim3 grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
  hipLaunchKernelGGL(variance_spatial_kernel, grid, dim3(kBX * kBY), 0, stream, ws.col[0], ws.geo, ws.hit,
                     tile_strata, batch_strata, min_batches, W, H, tiles_x, K);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return variance_passes(ws, W, H, passes, K, sigma_l, out, var_out, stream);
}

// the same passes on a variance plane the caller gives: no estimation stage
extern "C" hipError_t rtk_launch_denoise_given_variance(int W, int H, const double *rgb, double scale,
                                                        const int32_t *tile_strata, const double *guides,
                                                        int guide_strata, const double *variance, int passes,
                                                        double sigma_n, double sigma_z, double sigma_h,
                                                        double sigma_l, void *workspace, double *out,
                                                        double *var_out, hipStream_t stream) {
  const int64_t n = (int64_t)W * H;
  if (n <= 0) return hipSuccess;
  const VarianceWs ws = variance_ws(workspace, n);
  hipLaunchKernelGGL(variance_prepare_given_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rgb,
                     scale, tile_strata, guides, 1.0 / (double)guide_strata, variance, W, H, (W + 7) / 8, ws.col[0],
                     ws.geo, ws.alb, ws.hit);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return variance_passes(ws, W, H, passes, variance_coef(sigma_n, sigma_z, sigma_h), sigma_l, out, var_out, stream);
}

extern "C" size_t rtk_denoise_workspace_bytes(int W, int H) {
  const size_t plane = (((size_t)W * H * sizeof(float4)) + 255) & ~(size_t)255;
  return 4 * plane;
}

extern "C" hipError_t rtk_launch_denoise(int W, int H, const double *rgb, double scale,
                                         const int32_t *tile_strata, const double *guides, int guide_strata,
                                         int passes, double sigma_n, double sigma_z, double sigma_h,
                                         double sigma_c, void *workspace, double *out, hipStream_t stream) {
  const int64_t n = (int64_t)W * H;
  if (n <= 0) return hipSuccess;
  const size_t plane = rtk_denoise_workspace_bytes(W, H) / 4;
  float4 *col[2] = {reinterpret_cast<float4 *>(workspace),
                    reinterpret_cast<float4 *>(static_cast<char *>(workspace) + plane)};
  float4 *geo = reinterpret_cast<float4 *>(static_cast<char *>(workspace) + 2 * plane);
  float4 *alb = reinterpret_cast<float4 *>(static_cast<char *>(workspace) + 3 * plane);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3(blocks), dim3(256), 0, stream, rgb, scale, tile_strata,
                     guides, 1.0 / (double)guide_strata, W, H, (W + 7) / 8, col[0], geo, alb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (passes <= 0) {
    hipLaunchKernelGGL(denoise_remodulate_kernel, dim3(blocks), dim3(256), 0, stream, col[0], alb, n, out);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)((W + kBX - 1) / kBX), (unsigned)((H + kBY - 1) / kBY));
  for (int k = 0; k < passes; ++k) {
    PassCoef K;
    K.inv_sn2 = sigma_n > 0 ? (float)(1.0 / (sigma_n * sigma_n)) : 0.0f;
    K.inv_sz = sigma_z > 0 ? (float)(1.0 / sigma_z) : 0.0f;
    K.inv_sh2 = sigma_h > 0 ? (float)(1.0 / (sigma_h * sigma_h)) : 0.0f;
    const double sc = sigma_c / (double)(1 << k);
    K.inv_sc2 = sigma_c > 0 ? (float)(1.0 / (sc * sc)) : 0.0f;
    const bool last = k == passes - 1;
    hipLaunchKernelGGL(denoise_pass_kernel, grid, dim3(kBX * kBY), 0, stream, col[k & 1], geo, alb, W, H, 1 << k,
                       K, col[(k & 1) ^ 1], last ? out : nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
