// rt_denoise.hip — the edge-avoiding a-trous filters of the displayed frame
// (rt_denoise_device, rt_denoise_variance_device, rt_denoise_given_variance_device;
// statement of record: rtx/denoise.py NumpyOps).
//
// The fp64 accumulator is read once and never written.  `prepare` demodulates
// the scaled frame by the first-hit albedo and packs what the passes need into
// the caller's workspace as fp32, in float4 planes:
//   col[0], col[1]  (e.r, e.g, e.b, w)   the ping-pong pair
//   geo             (n.x, n.y, n.z, z)   mean normal (not renormalised), mean hit depth
//   alb             (a_d.r, a_d.g, a_d.b, 0)  the remodulation factor max(a, 0.01)
// Pass k gathers the 5x5 B3-spline taps at step 2^k: one lane per pixel, no
// atomics, blocks of 64 x 4 pixels so that every tap of a wavefront is one
// contiguous 64-pixel row segment (a coalesced 16-B-per-lane load) whatever
// the step.  One native fp32 exponential per tap.  The last pass multiplies by
// a_d and widens to the fp64 output.
//
// Two layouts, one statement of every stage (prepare_kernel<VSource>,
// pass_kernel<VAR>, remodulate_kernel, FilterWs, pass_coef, run_passes):
//   plain     64 B per pixel: w = h = hits / g rides along in col, so a tap is
//             two 16-B loads; the colour term is |e_p - e_q|^2 over the
//             pixel's own luminance
//   variance  68 B per pixel: w = v, the variance of e's luminance, and h in a
//             float plane of its own, so a tap is 36 B (16 + 16 + 4); the
//             colour term is |y_p - y_q| over the standard deviation of the
//             pixel's estimate, and v is filtered with the colour.  v comes
//             from the batch moments and variance_spatial_kernel, or from the
//             caller's plane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"

namespace {

constexpr int kBX = 64, kBY = 4;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

// where prepare takes v from: the plain layout has none (col.w = h); the batch
// moments va = s1, vb = s2; the caller's plane va
enum VSource { V_NONE, V_MOMENTS, V_GIVEN };

// V_MOMENTS: v where the pixel's tile has enough batches (tile_batches >=
// min_batches >= 2; fp64, rounded once), 0 elsewhere: variance_spatial_kernel
// fills those in.  V_GIVEN: a NaN or negative value is 0, nothing is left for
// variance_spatial_kernel.  Both: v = 0 where e is not finite.
template <VSource VS>
__global__ void __launch_bounds__(256)
    prepare_kernel(const double *rgb, double scale, const int32_t *tile_strata, const double *guides, double inv_g,
                   const double *va, const double *vb, int batch_strata, int min_batches, int W, int H, int tiles_x,
                   float4 *col, float4 *geo, float4 *alb, float *hit) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  double s = scale;
  int strata = 0;
  if (tile_strata != nullptr) { // rt_to_bytes_tiles_device's scale
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
    ad[c] = a > 0.01 ? a : 0.01; // max(a, 0.01)
    e[c] = (float)(rgb[3 * p + c] * s / ad[c]);
  }
  float v = 0.0f;
  if constexpr (VS == V_MOMENTS) {
    if (va != nullptr && finite3(e[0], e[1], e[2])) {
      const int b = strata / batch_strata;
      if (b >= min_batches) {
        const double fb = (double)b, a1 = va[p], a2 = vb[p];
        double var = (a2 - a1 * a1 / fb) / (fb - 1.0);
        var = var > 0.0 ? var : 0.0; // a NaN moment: 0
        const double la = 0.2126 * ad[0] + 0.7152 * ad[1] + 0.0722 * ad[2];
        v = (float)(var / fb / (la * la));
      }
    }
  } else if constexpr (VS == V_GIVEN) {
    const double vp = va[p];
    v = (vp > 0.0 && finite3(e[0], e[1], e[2])) ? (float)vp : 0.0f;
  }
  const double hits = G[7];
  const float h = (float)(hits * inv_g);
  col[p] = make_float4(e[0], e[1], e[2], VS == V_NONE ? h : v);
  geo[p] = make_float4((float)(G[3] * inv_g), (float)(G[4] * inv_g), (float)(G[5] * inv_g),
                       (float)(G[6] / (hits > 1.0 ? hits : 1.0)));
  alb[p] = make_float4((float)ad[0], (float)ad[1], (float)ad[2], 0.0f);
  if constexpr (VS != V_NONE) hit[p] = h;
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

// One pass.  VAR false, the plain layout: h is in[].w and is carried along;
// the colour term is |e_p - e_q|^2 K.inv_sc2 / (y_p^2 + 1e-4).  VAR true, the
// variance layout: h is hit[], in[].w is v; the colour term is
// |y_p - y_q| / (sigma_l sqrt(v~_p) + 1e-6), v~ the 3x3 Gaussian of v over the
// finite in-image neighbours (sigma_l <= 0: term off, no blur), and v is
// carried along: v' = sum w^2 v_q / (sum w)^2.  hit, sigma_l and out_var are
// VAR's alone.
template <bool VAR>
__global__ void __launch_bounds__(kBX *kBY)
    pass_kernel(const float4 *__restrict__ in, const float4 *__restrict__ geo, const float *__restrict__ hit,
                const float4 *__restrict__ alb, int W, int H, int step, PassCoef K, float sigma_l,
                float4 *__restrict__ out, double *__restrict__ out_rgb, double *__restrict__ out_var) {
  const int x = blockIdx.x * kBX + (threadIdx.x & (kBX - 1));
  const int y = blockIdx.y * kBY + (threadIdx.x / kBX);
  if (x >= W || y >= H) return;
  const int64_t p = (int64_t)y * W + x;
  const float4 ep = in[p], gp = geo[p];
  const float hp = VAR ? hit[p] : ep.w;
  const bool p_ok = finite3(ep.x, ep.y, ep.z);
  const float yp = luma(ep);
  // the colour term's per-pixel factor; a non-finite centre has no colour term
  float cw = 0.0f;
  if constexpr (VAR) {
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
  } else {
    cw = p_ok ? __fdividef(K.inv_sc2, yp * yp + 1e-4f) : 0.0f;
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
        const float4 gq = geo[q];
        float t = geo_terms(gp, gq, hp, VAR ? hit[q] : eq.w, (float)(step * max(abs(di), abs(dj))), K);
        if constexpr (VAR) {
          t += p_ok ? fabsf(yp - luma(eq)) * cw : 0.0f;
        } else {
          const float cr = ep.x - eq.x, cg = ep.y - eq.y, cb = ep.z - eq.z;
          t += p_ok ? (cr * cr + cg * cg + cb * cb) * cw : 0.0f;
        }
        w *= edge_weight(t);
      }
      if (!finite3(eq.x, eq.y, eq.z)) w = 0.0f;
      if (w > 0.0f) {
        sw += w;
        sr += w * eq.x;
        sg += w * eq.y;
        sb += w * eq.z;
        if constexpr (VAR) sv += w * w * eq.w;
      }
    }
  }
  float4 r = ep; // no weight at all: the pixel keeps its own value (and variance)
  if (sw > 0.0f) {
    const float inv = 1.0f / sw;
    r = make_float4(sr * inv, sg * inv, sb * inv, VAR ? sv * (inv * inv) : ep.w);
  }
  if (out_rgb != nullptr) { // the last pass: remodulate, widen
    const float4 a = alb[p];
    out_rgb[3 * p + 0] = (double)r.x * (double)a.x;
    out_rgb[3 * p + 1] = (double)r.y * (double)a.y;
    out_rgb[3 * p + 2] = (double)r.z * (double)a.z;
    if constexpr (VAR)
      if (out_var != nullptr) out_var[p] = (double)r.w;
  } else {
    out[p] = r;
  }
}

// passes < 0: prepare + remodulate only; out_var (the variance layout's v) may be null
__global__ void __launch_bounds__(256)
    remodulate_kernel(const float4 *col, const float4 *alb, int64_t n, double *out_rgb, double *out_var) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float4 e = col[p], a = alb[p];
  out_rgb[3 * p + 0] = (double)e.x * (double)a.x;
  out_rgb[3 * p + 1] = (double)e.y * (double)a.y;
  out_rgb[3 * p + 2] = (double)e.z * (double)a.z;
  if (out_var != nullptr) out_var[p] = (double)e.w;
}

size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// the workspace: four float4 planes, each padded to 256 B, and in the variance layout a float plane after them
struct FilterWs {
  float4 *col[2], *geo, *alb;
  float *hit; // the variance layout's; null in the plain one
};
size_t ws_bytes(int W, int H, bool variance) {
  const size_t n = (size_t)W * H;
  return 4 * pad256(n * sizeof(float4)) + (variance ? pad256(n * sizeof(float)) : 0);
}
FilterWs ws_carve(void *workspace, int64_t n, bool variance) {
  const size_t plane = pad256((size_t)n * sizeof(float4));
  char *ws = static_cast<char *>(workspace);
  return FilterWs{{reinterpret_cast<float4 *>(ws), reinterpret_cast<float4 *>(ws + plane)},
                  reinterpret_cast<float4 *>(ws + 2 * plane), reinterpret_cast<float4 *>(ws + 3 * plane),
                  variance ? reinterpret_cast<float *>(ws + 4 * plane) : nullptr};
}

// the geometry coefficients; the plain filter sets its per-pass inv_sc2 on top
PassCoef pass_coef(const FilterLaunch &a) {
  PassCoef K;
  K.inv_sn2 = a.sigma_n > 0 ? (float)(1.0 / (a.sigma_n * a.sigma_n)) : 0.0f;
  K.inv_sz = a.sigma_z > 0 ? (float)(1.0 / a.sigma_z) : 0.0f;
  K.inv_sh2 = a.sigma_h > 0 ? (float)(1.0 / (a.sigma_h * a.sigma_h)) : 0.0f;
  K.inv_sc2 = 0.0f;
  return K;
}

// the passes (or, passes <= 0, the remodulation alone) over a prepared workspace
hipError_t run_passes(const FilterLaunch &a, const FilterWs &ws, PassCoef K, hipStream_t stream) {
  const bool variance = a.kind != RTK_FILTER_PLAIN;
  const int64_t n = (int64_t)a.W * a.H;
  double *var_out = variance ? a.var_out : nullptr;
  if (a.passes <= 0) {
    hipLaunchKernelGGL(remodulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws.col[0], ws.alb,
                       n, a.out, var_out);
    return hipGetLastError();
  }
  const auto kernel = variance ? pass_kernel<true> : pass_kernel<false>;
  const float sigma_l = variance && a.sigma_c > 0 ? (float)a.sigma_c : 0.0f;
  const dim3 grid((unsigned)((a.W + kBX - 1) / kBX), (unsigned)((a.H + kBY - 1) / kBY));
  for (int k = 0; k < a.passes; ++k) {
    if (!variance) {
      const double sc = a.sigma_c / (double)(1 << k);
      K.inv_sc2 = a.sigma_c > 0 ? (float)(1.0 / (sc * sc)) : 0.0f;
    }
    const bool last = k == a.passes - 1;
    hipLaunchKernelGGL(kernel, grid, dim3(kBX * kBY), 0, stream, ws.col[k & 1], ws.geo, ws.hit, ws.alb, a.W, a.H,
                       1 << k, K, sigma_l, ws.col[(k & 1) ^ 1], last ? a.out : nullptr, last ? var_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace

extern "C" size_t rtk_denoise_workspace_bytes(int W, int H) { return ws_bytes(W, H, false); }
extern "C" size_t rtk_denoise_variance_workspace_bytes(int W, int H) { return ws_bytes(W, H, true); }

extern "C" hipError_t rtk_launch_filter(const FilterLaunch *args, hipStream_t stream) {
  const FilterLaunch &a = *args;
  const int64_t n = (int64_t)a.W * a.H;
  if (n <= 0) return hipSuccess;
  const FilterWs ws = ws_carve(a.workspace, n, a.kind != RTK_FILTER_PLAIN);
  const PassCoef K = pass_coef(a);
  const int tiles_x = (a.W + 7) / 8;
  const double inv_g = 1.0 / (double)a.guide_strata;
  const dim3 blocks((unsigned)((n + 255) / 256));
  if (a.kind == RTK_FILTER_PLAIN) {
    hipLaunchKernelGGL(prepare_kernel<V_NONE>, blocks, dim3(256), 0, stream, a.rgb, a.scale, a.tile_strata, a.guides,
                       inv_g, nullptr, nullptr, 0, 0, a.W, a.H, tiles_x, ws.col[0], ws.geo, ws.alb, ws.hit);
  } else if (a.kind == RTK_FILTER_GIVEN) {
    hipLaunchKernelGGL(prepare_kernel<V_GIVEN>, blocks, dim3(256), 0, stream, a.rgb, a.scale, a.tile_strata, a.guides,
                       inv_g, a.variance, nullptr, 0, 0, a.W, a.H, tiles_x, ws.col[0], ws.geo, ws.alb, ws.hit);
  } else {
    // no moments: every pixel takes the spatial estimate
    const bool moments = a.s1 && a.s2 && a.tile_strata && a.batch_strata >= 1;
    const int batch_strata = moments ? a.batch_strata : 0;
    hipLaunchKernelGGL(prepare_kernel<V_MOMENTS>, blocks, dim3(256), 0, stream, a.rgb, a.scale, a.tile_strata,
                       a.guides, inv_g, moments ? a.s1 : nullptr, moments ? a.s2 : nullptr, batch_strata,
                       a.min_batches, a.W, a.H, tiles_x, ws.col[0], ws.geo, ws.alb, ws.hit);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((a.W + kBX - 1) / kBX), (unsigned)((a.H + kBY - 1) / kBY));
    hipLaunchKernelGGL(variance_spatial_kernel, grid, dim3(kBX * kBY), 0, stream, ws.col[0], ws.geo, ws.hit,
                       a.tile_strata, batch_strata, a.min_batches, a.W, a.H, tiles_x, K);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return run_passes(a, ws, K, stream);
}
