// Camera pose gradients: get_rays (H:164-173) from poses in DEVICE memory for chosen pixels, its backward w.r.t. the poses, and the
// pose parametrisation c2w = [Exp(rot) R0 | t0 + trans] with its backward.  The ray arithmetic is cn_raw_dir of raygen.hpp (the one
// definition: the values equal cnerf_gen_rays bit for bit); compiled without FMA contraction like every file here.
//
// The backward is a reduction over the rays.  No floating-point atomics, one summation order:
//   stage 1  one wave per CHUNK of 64 consecutive rays (a fixed size, so the order of the sums does not depend on the grid: the grid
//            only decides which wave takes which chunk).  Per view the wave sums its rays of that view in fp64 with the xor butterfly
//            and writes one record of 12 doubles at rec[chunk][view][12]; a view none of the 64 rays belongs to gets a zero record.
//   stage 2  one wave per view: lane l adds the records of chunks l, l + 64, ... in order, the 64 lane sums go through the same
//            butterfly, and the 12 results are rounded to fp32 once.
// The products d_d[b][r] * dirs_b[k] of two floats are exact in fp64.
#include "raygen.hpp"

namespace {

constexpr int RG_CHUNK = 64;      // rays per stage-1 record = one wave
constexpr int RG_WAVES = 4;       // waves per stage-1 workgroup

struct PoseCam {                  // what cn_raw_dir reads of a camera
  float fx, fy, cx, cy;
  float r[9];
};

__device__ __forceinline__ void pixel_of(const int64_t* __restrict__ coords, int64_t first, int W, int64_t b, int& j, int& i) {
  if (coords) {
    j = (int)coords[2 * b]; i = (int)coords[2 * b + 1];
  } else {
    const int64_t idx = first + b;
    j = (int)(idx / W); i = (int)(idx - (int64_t)j * W);
  }
}

__global__ void gen_rays_at_k(int W, float fx, float fy, float cx, float cy, const float* __restrict__ c2w,
                              const int64_t* __restrict__ coords, const int64_t* __restrict__ view, int64_t first, int64_t B,
                              float* __restrict__ ro, float* __restrict__ rd) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int j, i;
  pixel_of(coords, first, W, b, j, i);
  const float* p = c2w + (view ? view[b] : 0) * 12;
  PoseCam g;
  g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g.r[3 * r] = p[4 * r]; g.r[3 * r + 1] = p[4 * r + 1]; g.r[3 * r + 2] = p[4 * r + 2];
  }
  float dx, dy, dz;
  cn_raw_dir(g, j, i, dx, dy, dz);
  ro[3 * b] = p[3]; ro[3 * b + 1] = p[7]; ro[3 * b + 2] = p[11];      // rays_o = c2w[:3, -1] (H:172)
  rd[3 * b] = dx; rd[3 * b + 1] = dy; rd[3 * b + 2] = dz;
}

// the 12 sums of one wave, each to lane k: lane k < 12 returns sum k, the other lanes 0
__device__ __forceinline__ double sums_to_lanes(const double (&t)[12], bool mine, int lane) {
  double keep = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const double x = wave_sum(mine ? t[k] : 0.0);
    if (lane == k) keep = x;
  }
  return keep;
}

__global__ __launch_bounds__(RG_CHUNK* RG_WAVES) void gen_rays_at_bwd_k(int W, float fx, float fy, float cx, float cy,
                                                                        const float* __restrict__ d_o, const float* __restrict__ d_d,
                                                                        const int64_t* __restrict__ coords,
                                                                        const int64_t* __restrict__ view, int64_t first, int64_t B,
                                                                        int n_views, int64_t n_chunks, double* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * RG_WAVES;
  for (int64_t c = (int64_t)blockIdx.x * RG_WAVES + (threadIdx.x >> 6); c < n_chunks; c += nwaves) {   // (wave-uniform)
    const int64_t b = c * RG_CHUNK + lane;
    const bool live = b < B;
    double t[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = 0.0;
    int64_t v = -1;
    if (live) {
      int j, i;
      pixel_of(coords, first, W, b, j, i);
      const float dir[3] = {((float)i - cx) / fx, -((float)j - cy) / fy, -1.f};      // H:167, as cn_raw_dir forms it
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double g = (double)d_d[3 * b + r];
        t[4 * r] = g * (double)dir[0]; t[4 * r + 1] = g * (double)dir[1]; t[4 * r + 2] = g * (double)dir[2];
        t[4 * r + 3] = (double)d_o[3 * b + r];
      }
      v = view ? view[b] : 0;
    }
    for (int q = 0; q < n_views; ++q) {
      const bool mine = live && v == q;
      double keep = 0.0;
      if (__ballot(mine) != 0) keep = sums_to_lanes(t, mine, lane);      // (wave-uniform)
      if (lane < 12) rec[(c * n_views + q) * 12 + lane] = keep;
    }
  }
}

__global__ __launch_bounds__(64) void gen_rays_at_reduce_k(const double* __restrict__ rec, int64_t n_chunks, int n_views,
                                                           float* __restrict__ d_c2w) {
  const int q = blockIdx.x, lane = threadIdx.x;
  double s[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) s[k] = 0.0;
  for (int64_t c = lane; c < n_chunks; c += 64) {
    const double* r = rec + (c * n_views + q) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] += r[k];
  }
  const double keep = sums_to_lanes(s, true, lane);
  if (lane < 12) d_c2w[(int64_t)q * 12 + lane] = (float)keep;
}

// ---- Exp(w) = I + A K + Bc K^2, K = [w]x, theta^2 = w . w (Rodrigues) ---------------------------------------------------------------
//   A(t2)  = sin(theta) / theta                  Bc(t2) = (1 - cos theta) / theta^2 = 1/2 (sin(theta/2) / (theta/2))^2 = A(t2 / 4)^2 / 2
//   C(t2)  = A'(theta) / theta  = (theta cos theta - sin theta) / theta^3 = (cos theta - A) / theta^2        (the backward's)
//   D(t2)  = Bc'(theta) / theta = (theta sin theta - 2 (1 - cos theta)) / theta^4 = A(t2 / 4) C(t2 / 4) / 4  (the backward's)
// Written through the half angle, Bc and D cancel nothing, and only A and C remain to be evaluated.  A's closed form is sound for
// every theta > 0, but theta = sqrt(t2) is not once t2 underflows; C's closed form subtracts cos theta - A = -theta^2 / 3 + ...:
// an absolute error of about 1.5 eps (eps = 2^-24: sin, cos, the quotient and the difference round once each) over theta^2 / 3, a
// relative error of 4.5 eps / theta^2 — 5 eps at theta = 1, 4.5e6 eps at 1e-3.  Below the threshold both are therefore power series in t2:
//   A = sum_n (-1)^n t2^n / (2n + 1)!             6 terms; the first one dropped is t2^6 / 13! = 1.6e-10 t2^6
//   C = sum_m (-1)^(m+1) (2m + 2) t2^m / (2m + 3)!   5 terms; the first one dropped is t2^5 / 518918400, relative to |C| ~ 1/3:
//                                                    5.8e-9 t2^5
// The truncation error must stay below eps / 2 = 3.0e-8: 5.8e-9 t2^5 <= 3.0e-8 holds up to t2 = 1.39 (theta = 1.18).  The threshold
// is t2 = 1: there the series is off by 0.1 eps (C) and 0.003 eps (A) before its own Horner roundings (about 1 eps), and from there
// up the closed form of C stays within 5 eps.  At w = 0 exactly the series give A = 1, Bc = 1/2, C = -1/3, D = -1/12: the gradient
// is the three generators applied to R0.  These fp32 coefficients are the BACKWARD's; the forward (pose_compose_k) evaluates A and Bc
// in closed form in fp64 and copies R0 at w = 0.
constexpr float POSE_SERIES_T2 = 1.0f;

__device__ __forceinline__ float pose_A(float t2) {
  if (t2 < POSE_SERIES_T2)
    return 1.f + t2 * (-1.f / 6.f + t2 * (1.f / 120.f + t2 * (-1.f / 5040.f + t2 * (1.f / 362880.f + t2 * (-1.f / 39916800.f)))));
  const float th = sqrtf(t2);
  return sinf(th) / th;
}
__device__ __forceinline__ float pose_C(float t2) {
  if (t2 < POSE_SERIES_T2)
    return -1.f / 3.f + t2 * (1.f / 30.f + t2 * (-1.f / 840.f + t2 * (1.f / 45360.f + t2 * (-1.f / 3991680.f))));
  const float th = sqrtf(t2);
  return (cosf(th) - sinf(th) / th) / t2;
}

__global__ void pose_compose_k(const float* __restrict__ c2w0, const float* __restrict__ rot, const float* __restrict__ trans, int N,
                               float* __restrict__ c2w) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* P = c2w0 + (int64_t)n * 12;
  float* out = c2w + (int64_t)n * 12;
  const float x = rot[3 * n], y = rot[3 * n + 1], z = rot[3 * n + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) out[4 * r + 3] = P[4 * r + 3] + trans[3 * n + r];
  if (x == 0.f && y == 0.f && z == 0.f) {      // Exp(0) = I: R0's own bits (a product with 0 would turn a -0 of R0 into +0)
#pragma unroll
    for (int r = 0; r < 3; ++r) { out[4 * r] = P[4 * r]; out[4 * r + 1] = P[4 * r + 1]; out[4 * r + 2] = P[4 * r + 2]; }
    return;
  }
  // The value is formed in fp64 at the fp32 inputs and rounded to fp32 once (one thread per view: the cost is nothing).  In fp32,
  // E's diagonal 1 - Bc (y^2 + z^2) carries Bc's relative error (five roundings through the half angle's square) times Bc t2, which
  // is 2 at theta = pi: R R^T - I of the composed rotation reached 13 eps there (random axes; 12 eps at theta = 10) against 1.4 eps
  // of the rounded R0 itself.  Rounded once, every element is within half an ulp and R R^T - I stays at R0's own plus 1.7 eps.
  // theta = sqrt(t2) cannot underflow here: the smallest fp32 squares to 2e-90.
  const double xd = x, yd = y, zd = z;
  const double t2 = xd * xd + yd * yd + zd * zd, th = sqrt(t2), hh = 0.5 * th;
  const double A = sin(th) / th, Ah = sin(hh) / hh, Bc = 0.5 * Ah * Ah;
  // E = I + A K + Bc (w w^T - t2 I)
  const double E[9] = {1.0 - Bc * (yd * yd + zd * zd), Bc * xd * yd - A * zd,           Bc * xd * zd + A * yd,
                       Bc * xd * yd + A * zd,           1.0 - Bc * (xd * xd + zd * zd), Bc * yd * zd - A * xd,
                       Bc * xd * zd - A * yd,           Bc * yd * zd + A * xd,           1.0 - Bc * (xd * xd + yd * yd)};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      out[4 * r + k] = (float)(E[3 * r] * (double)P[k] + E[3 * r + 1] * (double)P[4 + k] + E[3 * r + 2] * (double)P[8 + k]);
}

__global__ void pose_compose_bwd_k(const float* __restrict__ c2w0, const float* __restrict__ rot, const float* __restrict__ d_c2w, int N,
                                   float* __restrict__ d_rot, float* __restrict__ d_trans) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* P = c2w0 + (int64_t)n * 12;
  const float* G = d_c2w + (int64_t)n * 12;
  if (d_trans) {
#pragma unroll
    for (int r = 0; r < 3; ++r) d_trans[3 * n + r] = G[4 * r + 3];
  }
  if (!d_rot) return;
  const float w[3] = {rot[3 * n], rot[3 * n + 1], rot[3 * n + 2]};
  const float t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  float dE[9];      // d loss / d Exp(w) = G_R R0^T
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) dE[3 * r + j] = G[4 * r] * P[4 * j] + G[4 * r + 1] * P[4 * j + 1] + G[4 * r + 2] * P[4 * j + 2];
  const float A = pose_A(t2), Ah = pose_A(0.25f * t2), Bc = 0.5f * Ah * Ah, C = pose_C(t2), D = 0.25f * Ah * pose_C(0.25f * t2);
  // <dE, dK / dw_k> = v_k: the antisymmetric part of dE (at w = 0 the whole gradient)
  const float v[3] = {dE[7] - dE[5], dE[2] - dE[6], dE[3] - dE[1]};
  const float tr = dE[0] + dE[4] + dE[8];
  float sw[3];      // (dE + dE^T) w
#pragma unroll
  for (int k = 0; k < 3; ++k)
    sw[k] = (dE[3 * k] + dE[k]) * w[0] + (dE[3 * k + 1] + dE[3 + k]) * w[1] + (dE[3 * k + 2] + dE[6 + k]) * w[2];
  const float wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2];                  // <dE, K>
  const float wEw = 0.5f * (w[0] * sw[0] + w[1] * sw[1] + w[2] * sw[2]);     // w^T dE w
  const float s = C * wv + D * (wEw - t2 * tr) - 2.f * Bc * tr;              // everything that multiplies w
#pragma unroll
  for (int k = 0; k < 3; ++k) d_rot[3 * n + k] = A * v[k] + Bc * sw[k] + s * w[k];
}

inline bool rays_at_args_ok(int H, int W, float fx, float fy, int n_views, const int64_t* coords, int64_t first, int64_t B) {
  if (H <= 0 || W <= 0 || !(fx != 0.f) || !(fy != 0.f) || n_views <= 0 || B <= 0) return false;
  return coords || (first >= 0 && first <= (int64_t)H * W - B);      // the row-major window lies inside the image
}

}  // namespace

extern "C" int cnerf_gen_rays_at(int H, int W, float fx, float fy, float cx, float cy, const float* c2w, int n_views,
                                 const int64_t* coords, const int64_t* view, int64_t first, int64_t B, float* rays_o, float* rays_d,
                                 void* stream) {
  if (!c2w || !rays_o || !rays_d || !rays_at_args_ok(H, W, fx, fy, n_views, coords, first, B)) return CNERF_E_ARG;
  hipLaunchKernelGGL(gen_rays_at_k, dim3((unsigned)cn_div_up(B, 256)), dim3(256), 0, cn_stream(stream), W, fx, fy, cx, cy, c2w, coords,
                     view, first, B, rays_o, rays_d);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int64_t cnerf_gen_rays_at_bwd_ws_floats(int64_t B, int n_views) {
  if (B <= 0 || n_views <= 0) return 0;
  return 2 * 12 * (int64_t)n_views * cn_div_up(B, RG_CHUNK);      // [chunks][n_views][12] doubles
}

extern "C" int cnerf_gen_rays_at_bwd(int H, int W, float fx, float fy, float cx, float cy, const float* d_rays_o, const float* d_rays_d,
                                     int n_views, const int64_t* coords, const int64_t* view, int64_t first, int64_t B, float* d_c2w,
                                     float* workspace, int grid, void* stream) {
  if (!d_rays_o || !d_rays_d || !d_c2w || !workspace || ((uintptr_t)workspace & 7) || grid < 0 ||
      !rays_at_args_ok(H, W, fx, fy, n_views, coords, first, B))
    return CNERF_E_ARG;
  const int64_t n_chunks = cn_div_up(B, RG_CHUNK);
  const int64_t blocks = grid > 0 ? grid : (cn_div_up(n_chunks, RG_WAVES) < 1024 ? cn_div_up(n_chunks, RG_WAVES) : 1024);
  double* rec = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(gen_rays_at_bwd_k, dim3((unsigned)blocks), dim3(RG_CHUNK * RG_WAVES), 0, cn_stream(stream), W, fx, fy, cx, cy,
                     d_rays_o, d_rays_d, coords, view, first, B, n_views, n_chunks, rec);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(gen_rays_at_reduce_k, dim3((unsigned)n_views), dim3(64), 0, cn_stream(stream), rec, n_chunks, n_views, d_c2w);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_pose_compose(const float* c2w0, const float* rot, const float* trans, int n_views, float* c2w, void* stream) {
  if (!c2w0 || !rot || !trans || !c2w || n_views <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(pose_compose_k, dim3((unsigned)cn_div_up(n_views, 64)), dim3(64), 0, cn_stream(stream), c2w0, rot, trans, n_views,
                     c2w);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_pose_compose_bwd(const float* c2w0, const float* rot, const float* d_c2w, int n_views, float* d_rot, float* d_trans,
                                      void* stream) {
  if (!c2w0 || !rot || !d_c2w || (!d_rot && !d_trans) || n_views <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(pose_compose_bwd_k, dim3((unsigned)cn_div_up(n_views, 64)), dim3(64), 0, cn_stream(stream), c2w0, rot, d_c2w,
                     n_views, d_rot, d_trans);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
