// The loss terms of ConsistentNeRF that exist BOTH as launches of their own (loss.hip: masked_loss_k / masked_part_k / masked_fin_k,
// soft_lp_k, softmask_k) and folded into the compositing launches (composite.hip: composite_fwd_k / composite_bwd_k, finished by
// loss.hip's closs_tail_k): ONE definition of every fp32 / fp64 expression, included by each of those kernels.  The two routes give
// the same bits because they run the same code here, not because their authors kept copies in step (the build uses
// -ffp-contract=off: inlining an expression cannot change its rounding).  Statement (V:1645-1648, V:1737, V:1786-1788, V:1865):
//   e_i = sum_c (rgb_ic - tgt_ic)^2 (fp32, c = 0, 1, 2),  r_i = depth_i / far - prior_i / far (fp32);  sums over rays in fp64
//   img = fp32(sum_{m=1} e / (3 N1)) [+ coef fp32(sum_{m=0} e / (3 N0)) iff N0 > 0],  dep = fp32(sum_{m=1} r^2 / N1)
//   d img / d rgb_ic = w_m (rgb_ic - tgt_ic), w_1 = fp32(2 / (3 N1)), w_0 = coef fp32(2 / (3 N0));  d dep / d depth_i = wd r_i on
//   m = 1, wd = fp32(2 / N1) / far.  A mask value other than 0 and 1 puts its ray into neither set.
#pragma once
#include "common.hpp"

// ---- partial sums of a level: slots 0..4 of every route, 5..9 of the loss forms only (cnerf_lossform, include/cnerf.h) ----------
enum : int {
  LT_S1 = 0,     // sum of e over m == 1
  LT_S0 = 1,     // sum of e over m == 0
  LT_SD = 2,     // the depth term's main sum: squared residuals (over m == 1, or all rays: norm / plain), sum(w d^4) for softmask
  LT_N1 = 3,     // rays with m == 1
  LT_N0 = 4,     // rays with m == 0
  LT_D_W = 5,    // depth form's second set: squared residuals over m == 0 (hardmask_coef) | sum(w) (softlp / softmask)
  LT_D_WD2 = 6,  //                          sum(w d^2)
  LT_C_W = 7,    // colour form (softlp / softmask): sum(w)
  LT_C_WD2 = 8,  //                                  sum(w d^2)
  LT_C_WD4 = 9,  //                                  sum(w d^4)
};
constexpr int LT_MASKED_SLOTS = 5;
static_assert(LT_C_WD4 + 1 == CNERF_LOSSFORM_SLOTS, "slot names and cnerf.h disagree");

// ---- per-ray terms ---------------------------------------------------------------------------------------------------------------
// e = d0^2 + d1^2 + d2^2 in fp32, from 0 in channel order
__device__ __forceinline__ float lt_sq_err3(const float* x, const float* y) {
  float e = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float d = x[c] - y[c];
    e += d * d;
  }
  return e;
}
// The depth residual of the v6 terms: two divisions.  The loss forms' one below multiplies by 1 / far, as ATen divides a tensor by
// a scalar: the two round differently ON PURPOSE (each reproduces its own reference lines) and stay two functions.
__device__ __forceinline__ float lt_depth_res(float depth, float prior, float far) { return depth / far - prior / far; }
__device__ __forceinline__ float lt_depth_res_form(float depth, float prior, float inv_far) { return depth * inv_far - prior * inv_far; }

// a ray with mask value m into the partials t[LT_MASKED_SLOTS]
__device__ __forceinline__ void lt_accum_counts(double* t, float m) {
  if (m == 1.f) t[LT_N1] += 1.0;
  if (m == 0.f) t[LT_N0] += 1.0;
}
__device__ __forceinline__ void lt_accum_colour(double* t, float m, float e) {
  if (m == 1.f) t[LT_S1] += (double)e;
  if (m == 0.f) t[LT_S0] += (double)e;
}
__device__ __forceinline__ void lt_accum_depth(double* t, float m, float r) {
  if (m == 1.f) t[LT_SD] += (double)(r * r);
}
__device__ __forceinline__ void lt_accum_ray(double* t, float m, float e) {
  lt_accum_counts(t, m);
  lt_accum_colour(t, m, e);
}

// ---- normalisation ---------------------------------------------------------------------------------------------------------------
// fp64 quotient rounded to fp32 once: a mean over N rays (x 3 colour channels) and the weight of its gradient seed
__device__ __forceinline__ float lt_mean(double s, double N) { return (float)(s / N); }
__device__ __forceinline__ float lt_mean3(double s, double N) { return (float)(s / (3.0 * N)); }
__device__ __forceinline__ float lt_seed_w(double N) { return (float)(2.0 / N); }
__device__ __forceinline__ float lt_seed_w3(double N) { return (float)(2.0 / (3.0 * N)); }

struct LtNorm {
  double N1, N0;      // the counts the terms were normalised with
  float img, dep;     // the two loss values (0 without `values`)
  float w1, w0, wd;   // seed weights: colours of the m == 1 / m == 0 rays, depth of the m == 1 rays
};
// t = the five totals; counts = GLOBAL (n1, n0) (e.g. all-reduced over ranks), which override the local ones, or nullptr.
// g_scale multiplies the seed weights FIRST (left-associated, as written): any other placement changes the stand-alone kernels' bits.
// values = this thread writes the loss values: the others of a 1024-thread launch skip their three fp64 divisions, which would sit
// in front of every wave's seed loop (masked_loss_k at 4096 rays: 15 us with them skipped, 18 us without).
__device__ __forceinline__ LtNorm lt_normalise(const double* t, const float* counts, float coef, float far, bool has_depth,
                                               float g_scale, bool values) {
  LtNorm o;
  o.N1 = counts ? (double)counts[0] : t[LT_N1];
  o.N0 = counts ? (double)counts[1] : t[LT_N0];
  o.img = o.dep = 0.f;
  if (values) {
    o.img = lt_mean3(t[LT_S1], o.N1);
    if (o.N0 > 0) o.img += coef * lt_mean3(t[LT_S0], o.N0);
    if (has_depth) o.dep = lt_mean(t[LT_SD], o.N1);
  }
  o.w1 = g_scale * lt_seed_w3(o.N1);
  o.w0 = o.N0 > 0 ? g_scale * coef * lt_seed_w3(o.N0) : 0.f;
  o.wd = g_scale * lt_seed_w(o.N1) / far;
  return o;
}

// ---- per-ray seeds ---------------------------------------------------------------------------------------------------------------
// The stand-alone kernels store these; composite_bwd_k multiplies each by the upstream gradient at its call site (autograd's `d * g`).
__device__ __forceinline__ float lt_ray_w(float m, float w1, float w0) { return m == 1.f ? w1 : (m == 0.f ? w0 : 0.f); }
__device__ __forceinline__ float lt_seed_colour(float w, float x, float y) { return w * (x - y); }
__device__ __forceinline__ float lt_seed_depth(float m, float wd, float depth, float prior, float far) {
  return m == 1.f ? wd * lt_depth_res(depth, prior, far) : 0.f;
}

// ---- soft forms --------------------------------------------------------------------------------------------------------------------
// weight and weighted powers of one residual: softlp (V:58) w = |d|^coef + 1; softmask (V:50) w = exp(d^2 / t)
__device__ __forceinline__ void lt_soft_sums(bool softmask, float d, float coef, float t, double& sw, double& swd2, double& swd4) {
  const float d2 = d * d;
  const float w = softmask ? expf(d2 / t) : powf(fabsf(d), coef) + 1.f;
  sw += (double)w;
  swd2 += (double)(w * d2);
  if (softmask) swd4 += (double)(w * (d2 * d2));
}
// d loss / d residual of the same, times inv = fp32(1 / sum(w)) (the sum of weights is detached in d):
// softlp d (coef |d|^coef + 2 w);  softmask w (2 d + 2 d^3 / t)
__device__ __forceinline__ float lt_soft_seed(bool softmask, float d, float coef, float t, float inv) {
  if (softmask) return (expf((d * d) / t) * (2.f * d + 2.f * ((d * d) * d) / t)) * inv;
  const float p = powf(fabsf(d), coef);
  return (d * (coef * p + 2.f * (p + 1.f))) * inv;
}
// softmask: L = N / Dn with N = sum(w d^2), Dn = sum(w) (detached in d, NOT in t):  dL / dt = -(sum(w d^4) / Dn - L^2) / t^2
__device__ __forceinline__ double lt_softmask_dtemp(double s4, double Dn, double N, double t) {
  const double L = N / Dn;
  return -(s4 / Dn - L * L) / (t * t);
}
