// SSIM pieces shared by ssim.hip (the general kernels, the standalone patch term) and loss.hip (the patch term folded into the
// C3 step's loss tail).  The statement they implement (pytorch-msssim 0.2.1 `_ssim`, restated in DESIGN.md §SSIM):
//   mu_x = f(X), mu_y = f(Y), s_xx = f(X*X) - mu_x^2, s_yy = f(Y*Y) - mu_y^2, s_xy = f(X*Y) - mu_x mu_y   (single pass, fp32)
//   cs = (2 s_xy + C2) / (s_xx + s_yy + C2),  S = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs
// f = valid 1-D correlation with the normalised Gaussian window along H, then W, each skipped when that side is shorter than the
// window.  Derivatives of S used by the backward (l = the luminance factor, B1 / B2 its and cs's denominators):
//   dS/d f(x^2) = dS/d f(y^2) = -S / B2,   dS/d f(xy) = 2 l / B2,
//   dS/d mu_x = cs 2 (mu_y - l mu_x) / B1 + 2 mu_x S / B2 - 2 l mu_y / B2   (and x <-> y)
// and dX = f^T(dS/dmu_x) + 2 X f^T(dS/df(x^2)) + Y f^T(dS/df(xy)), f^T the zero-padded full correlation.
// MS-SSIM keeps the mean of cs at every level but the last, so its backward needs the same four derivatives of cs
// (cn_ssim_pixel_cs) and, per level, a quarter of the next (2x2 average-pooled) level's gradient on top of dX.
#pragma once
#include "common.hpp"

constexpr int CN_SSIM_MAX_WIN = 31;

// pytorch-msssim's _fspecial_gauss_1d in fp32: coords = arange(size) - size // 2; g = exp(-coords^2 / (2 sigma^2)); g / sum(g)
__host__ __device__ inline void cn_ssim_window(int size, float sigma, float* g) {
  const float den = (float)(2.0 * (double)sigma * (double)sigma);
  float s = 0.f;
  for (int t = 0; t < size; ++t) {
    const float c = (float)(t - size / 2);
    g[t] = expf(-(c * c) / den);
    s += g[t];
  }
  for (int t = 0; t < size; ++t) g[t] = g[t] / s;
}

struct CnSsimPix {
  float S, cs;
  float ax, ay, b, c;   // dS/dmu_x, dS/dmu_y, dS/df(x^2) (= dS/df(y^2)), dS/df(xy)
};

// S and cs of one output pixel from the five filtered quantities, in the reference's order of operations; with `grad` the four
// coefficients as well
// (from the means and the single-pass variances)
__device__ __forceinline__ CnSsimPix cn_ssim_pixel_var(float mx, float my, float sxx, float syy, float sxy, float C1, float C2,
                                                      bool grad) {
  CnSsimPix o;
  const float mxx = mx * mx, myy = my * my, mxy = mx * my;
  const float B2 = sxx + syy + C2, B1 = mxx + myy + C1;
  o.cs = (2.f * sxy + C2) / B2;
  const float l = (2.f * mxy + C1) / B1;
  o.S = l * o.cs;
  if (grad) {
    o.b = -o.S / B2;
    o.c = 2.f * l / B2;
    o.ax = o.cs * 2.f * (my - l * mx) / B1 + 2.f * mx * o.S / B2 - 2.f * l * my / B2;
    o.ay = o.cs * 2.f * (mx - l * my) / B1 + 2.f * my * o.S / B2 - 2.f * l * mx / B2;
  } else {
    o.ax = o.ay = o.b = o.c = 0.f;
  }
  return o;
}

// The same pixel with the four coefficients of a seed on cs instead of S (MS-SSIM's levels below the last keep the mean of cs):
//   d cs/d f(x^2) = d cs/d f(y^2) = -cs / B2,   d cs/d f(xy) = 2 / B2,   d cs/d mu_x = 2 (mu_x cs - mu_y) / B2   (and x <-> y)
__device__ __forceinline__ CnSsimPix cn_ssim_pixel_cs(float mx, float my, float sxx, float syy, float sxy, float C1, float C2) {
  CnSsimPix o;
  const float B2 = sxx + syy + C2, B1 = mx * mx + my * my + C1;
  o.cs = (2.f * sxy + C2) / B2;
  o.S = (2.f * (mx * my) + C1) / B1 * o.cs;
  o.b = -o.cs / B2;
  o.c = 2.f / B2;
  o.ax = 2.f * (mx * o.cs - my) / B2;
  o.ay = 2.f * (my * o.cs - mx) / B2;
  return o;
}

__device__ __forceinline__ CnSsimPix cn_ssim_pixel(float mx, float my, float exx, float eyy, float exy, float C1, float C2,
                                                  bool grad) {
  return cn_ssim_pixel_var(mx, my, exx - mx * mx, eyy - my * my, exy - mx * my, C1, C2, grad);
}

// ---- V's patch term (V:1699-1701): ssim(img_pred, img_gt, data_range=1, size_average=False) on a [1, 16, 16, 3] NHWC patch that
// the library reads as NCHW: C = 16 (ray / 16), H = 16 (ray % 16, filtered to 6 rows), W = 3 (RGB, unfiltered: 3 < 11).
// One wave64 per patch: lane = (C index) * 3 + (W index) for lanes < 48, each one 1-D problem of 16 inputs and 6 outputs.
// Returns (all lanes) ssim_p = the mean of the 16 x 6 x 3 map; writes d[768] = scale * d ssim_p / d x when d != nullptr.
constexpr int CN_PATCH_SSIM_RAYS = 256;
__device__ __forceinline__ float cn_patch_ssim_wave(const float* __restrict__ x, const float* __restrict__ y, float scale,
                                                    float* __restrict__ d, int lane) {
  constexpr int WS = 11, HI = 16, HO = HI - WS + 1;
  constexpr float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);   // (K * data_range)^2 in double, data_range = 1
  float g[WS];
  cn_ssim_window(WS, 1.5f, g);
  const bool live = lane < 48;
  const int cc = lane / 3, w = lane - 3 * (lane / 3);
  float xs[HI], ys[HI];
#pragma unroll
  for (int h = 0; h < HI; ++h) {
    const int i = (cc * HI + h) * 3 + w;
    xs[h] = live ? x[i] : 0.f;
    ys[h] = live ? y[i] : 0.f;
  }
  float ax[HO], bb[HO], cf[HO];
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < HO; ++j) {
    float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
    for (int k = 0; k < WS; ++k) {
      const float a = xs[j + k], bv = ys[j + k];
      mx += g[k] * a; my += g[k] * bv;
      exx += g[k] * (a * a); eyy += g[k] * (bv * bv); exy += g[k] * (a * bv);
    }
    const CnSsimPix p = cn_ssim_pixel(mx, my, exx, eyy, exy, C1, C2, d != nullptr);
    if (live) sum += (double)p.S;
    ax[j] = p.ax * scale; bb[j] = p.b * scale; cf[j] = p.c * scale;
  }
  const float ssim_p = (float)(wave_sum(sum) / (double)(HO * HI * 3));
  if (d && live) {
#pragma unroll
    for (int i = 0; i < HI; ++i) {
      float fa = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
      for (int j = 0; j < HO; ++j) {
        const int k = i - j;
        if (k >= 0 && k < WS) { fa += g[k] * ax[j]; fb += g[k] * bb[j]; fc += g[k] * cf[j]; }
      }
      d[(cc * HI + i) * 3 + w] = fa + 2.f * xs[i] * fb + ys[i] * fc;
    }
  }
  return ssim_p;
}

// d ssim_level / d rgb of one patch value: ssim_level = (sum_p ssim_p) / 4 (V's literal 4), ssim_p = mean of 16 x 6 x 3 values
constexpr float CN_PATCH_SSIM_SCALE = 1.f / (4.f * 288.f);
