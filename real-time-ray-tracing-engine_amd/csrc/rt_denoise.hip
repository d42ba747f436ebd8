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
  const float yp = 0.2126f * ep.x + 0.7152f * ep.y + 0.0722f * ep.z;
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
        const float d = (float)(step * max(abs(di), abs(dj)));
        const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
        float t = (nx * nx + ny * ny + nz * nz) * K.inv_sn2;
        t += __fdividef(fabsf(gp.w - gq.w) * K.inv_sz, fmaxf(fmaxf(gp.w, gq.w), 1e-30f) * d);
        const float dh = ep.w - eq.w;
        t += dh * dh * K.inv_sh2;
        const float cr = ep.x - eq.x, cg = ep.y - eq.y, cb = ep.z - eq.z;
        t += p_ok ? (cr * cr + cg * cg + cb * cb) * cw : 0.0f;
        w *= __expf(-fminf(t, 80.0f));
        if (!(t == t)) w = 0.0f; // a NaN exponent: no weight (fminf would give 80)
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

} // namespace

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
