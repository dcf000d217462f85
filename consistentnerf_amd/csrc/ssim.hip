// SSIM / MS-SSIM of pytorch-msssim 0.2.1 (the library the reference calls at V:1701, V:1836 and alky/vis_utils.py img2ssim) on
// [N, C, H, W] fp32 planes, the 2x2 average pool between MS-SSIM levels, and V's patch term as a standalone launch.
// The statement and its derivatives are in ssim.hpp.  The forward's five filtered sums accumulate in fp64 and the single-pass
// variances f(XX) - mu^2 are formed there before rounding to fp32: at the coarse MS-SSIM levels the variances are small next to
// mu^2, and with fp32 sums that cancellation turned the rounding of f(XX) into the whole error (3x the reference's own fp32 error
// at 301 x 401).  The backward's transposed filter accumulates with fp32 fused multiply-adds.
//   forward:  ssim_tile_k — one workgroup per (tile of TH x TW output pixels, plane): X / Y tile + the (win - 1) halo into LDS, the
//             vertical pass of the five quantities into LDS, the horizontal pass + S / cs per pixel, one fp64 partial pair per
//             workgroup at a fixed index; ssim_fin_k sums a plane's partials in index order (no float atomics: identical bits).
//   backward: ssim_tile_k<1> writes the four coefficient maps (times the upstream gradient / the map's size), ssim_bwd_k applies the
//             transposed filter (zero-padded full correlation, again through LDS) and combines dX (and dY).
//   MS-SSIM:  the same kernels level by level.  Its backward seeds the last level's S and every other level's cs (ssim_tile_k<2>),
//             and ssim_bwd_k adds the 2x2 average pool's backward of the level after it in its epilogue.
#include "ssim.hpp"

namespace {

constexpr int NT = 256;                  // threads of the tile kernels
constexpr int FTH = 8, FTW = 64;         // forward output tile
constexpr int BTH = 8, BTW = 32;         // backward (input-space) tile

struct SsimWin {
  float gh[CN_SSIM_MAX_WIN], gw[CN_SSIM_MAX_WIN];   // taps along H / W ({1} where that side is skipped)
  int kh, kw;
};

struct SsimShape {
  int H, W, Ho, Wo, tiles_x, ntiles;
  float C1, C2;
};

__device__ __forceinline__ double block_sum256(double v, double* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < NT / 64; ++i) s += sh[i];
  return s;
}

// MODE 0: per-workgroup partial sums of S and cs -> part[(plane * ntiles + tile) * 2 + {0, 1}]
// MODE 1: coefficient maps coef[q][plane][Ho][Wo], q = dS/dmu_x, dS/dmu_y, dS/df(x^2), dS/df(xy), times g[plane] * inv_cnt
// MODE 2: the same four maps of cs instead of S (cn_ssim_pixel_cs): the seed of an MS-SSIM level below the last
template <int MODE>
__global__ __launch_bounds__(NT) void ssim_tile_k(const float* __restrict__ X, const float* __restrict__ Y, SsimShape s, SsimWin win,
                                                  double* __restrict__ part, float* __restrict__ coef, const float* __restrict__ g,
                                                  float inv_cnt, int64_t nplanes) {
  extern __shared__ float lds[];
  __shared__ double red[NT / 64];
  const int64_t plane = blockIdx.y;
  const int tile = blockIdx.x, ty = tile / s.tiles_x, tx = tile - ty * s.tiles_x;
  const int r0 = ty * FTH, c0 = tx * FTW;
  const int IR = FTH + win.kh - 1, IC = FTW + win.kw - 1;
  double* v = reinterpret_cast<double*>(lds);   // [5][FTH][IC]
  float* sx = lds + 2 * 5 * FTH * IC;
  float* sy = sx + IR * IC;
  const float* Xp = X + plane * s.H * s.W;
  const float* Yp = Y + plane * s.H * s.W;
  for (int i = threadIdx.x; i < IR * IC; i += NT) {
    const int r = i / IC, c = i - r * IC, gr = r0 + r, gc = c0 + c;
    const bool in = gr < s.H && gc < s.W;
    sx[i] = in ? Xp[(int64_t)gr * s.W + gc] : 0.f;
    sy[i] = in ? Yp[(int64_t)gr * s.W + gc] : 0.f;
  }
  __syncthreads();
  const int VP = FTH * IC;
  for (int i = threadIdx.x; i < VP; i += NT) {
    const int r = i / IC, c = i - r * IC;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    for (int k = 0; k < win.kh; ++k) {
      const double w = win.gh[k], x = sx[(r + k) * IC + c], y = sy[(r + k) * IC + c];
      a0 = fma(w, x, a0); a1 = fma(w, y, a1); a2 = fma(w, x * x, a2); a3 = fma(w, y * y, a3); a4 = fma(w, x * y, a4);
    }
    v[i] = a0; v[VP + i] = a1; v[2 * VP + i] = a2; v[3 * VP + i] = a3; v[4 * VP + i] = a4;
  }
  __syncthreads();
  double sS = 0.0, sC = 0.0;
  const float gsc = MODE != 0 ? g[plane] * inv_cnt : 0.f;
  for (int i = threadIdx.x; i < FTH * FTW; i += NT) {
    const int r = i / FTW, c = i - r * FTW, orow = r0 + r, ocol = c0 + c;
    if (orow >= s.Ho || ocol >= s.Wo) continue;
    double q[5];
#pragma unroll
    for (int k5 = 0; k5 < 5; ++k5) {
      const double* vq = v + k5 * VP + r * IC + c;
      double a = 0.0;
      for (int k = 0; k < win.kw; ++k) a = fma((double)win.gw[k], vq[k], a);
      q[k5] = a;
    }
    const float mx = (float)q[0], my = (float)q[1], sxx = (float)(q[2] - q[0] * q[0]), syy = (float)(q[3] - q[1] * q[1]),
                sxy = (float)(q[4] - q[0] * q[1]);
    const CnSsimPix p = MODE == 2 ? cn_ssim_pixel_cs(mx, my, sxx, syy, sxy, s.C1, s.C2)
                                  : cn_ssim_pixel_var(mx, my, sxx, syy, sxy, s.C1, s.C2, MODE == 1);
    if (MODE == 0) {
      sS += (double)p.S; sC += (double)p.cs;
    } else {
      const int64_t m = (int64_t)s.Ho * s.Wo, o = plane * m + (int64_t)orow * s.Wo + ocol;
      coef[o] = p.ax * gsc;
      coef[nplanes * m + o] = p.ay * gsc;
      coef[2 * nplanes * m + o] = p.b * gsc;
      coef[3 * nplanes * m + o] = p.c * gsc;
    }
  }
  if (MODE == 0) {
    sS = block_sum256(sS, red);
    __syncthreads();
    sC = block_sum256(sC, red);
    if (threadIdx.x == 0) {
      part[(plane * s.ntiles + tile) * 2 + 0] = sS;
      part[(plane * s.ntiles + tile) * 2 + 1] = sC;
    }
  }
}

// one wave per plane: the plane's partials in index order -> the per-channel means
__global__ __launch_bounds__(64) void ssim_fin_k(const double* __restrict__ part, int ntiles, double cnt, float* __restrict__ ssim,
                                                 float* __restrict__ cs) {
  const int64_t plane = blockIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < ntiles; i += 64) {
    a += part[(plane * ntiles + i) * 2 + 0];
    b += part[(plane * ntiles + i) * 2 + 1];
  }
  a = wave_sum(a); b = wave_sum(b);
  if (threadIdx.x == 0) {
    ssim[plane] = (float)(a / cnt);
    if (cs) cs[plane] = (float)(b / cnt);
  }
}

// dX[i] = f^T(ax)[i] + 2 X[i] f^T(b)[i] + Y[i] f^T(c)[i]  (dY with ay, Y, X): one workgroup per BTH x BTW input-space tile of a plane.
// nX / nY (nullable) [nplanes, nH, nW] = the gradient of the next MS-SSIM level, the 2x2 average pool of this one (padding
// (H % 2, W % 2), counted): its backward, a quarter of the one window pixel (i, j) lies in, is the last addend of the sum.
__global__ __launch_bounds__(NT) void ssim_bwd_k(const float* __restrict__ X, const float* __restrict__ Y, SsimShape s, SsimWin win,
                                                 const float* __restrict__ coef, int64_t nplanes, float* __restrict__ dX,
                                                 float* __restrict__ dY, const float* __restrict__ nX, const float* __restrict__ nY,
                                                 int nH, int nW) {
  extern __shared__ float lds[];
  const int64_t plane = blockIdx.y;
  const int tiles_x = (s.W + BTW - 1) / BTW;
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int r0 = ty * BTH, c0 = tx * BTW;
  const int IR = BTH + win.kh - 1, IC = BTW + win.kw - 1;
  const int NQ = dY ? 4 : 3;                         // planes: ax, b, c (+ ay)
  const int64_t m = (int64_t)s.Ho * s.Wo;
  float* sc = lds;                                   // [NQ][IR][IC]: coefficient rows r0 - (kh - 1) .., cols c0 - (kw - 1) ..
  float* v = sc + NQ * IR * IC;                      // [NQ][BTH][IC]
  for (int i = threadIdx.x; i < NQ * IR * IC; i += NT) {
    const int q = i / (IR * IC), rc = i - q * IR * IC, r = rc / IC, c = rc - r * IC;
    const int gr = r0 + r - (win.kh - 1), gc = c0 + c - (win.kw - 1);
    const int src = q == 0 ? 0 : (q == 1 ? 2 : (q == 2 ? 3 : 1));
    const bool in = gr >= 0 && gr < s.Ho && gc >= 0 && gc < s.Wo;
    sc[i] = in ? coef[src * nplanes * m + plane * m + (int64_t)gr * s.Wo + gc] : 0.f;
  }
  __syncthreads();
  const int VP = BTH * IC;
  for (int i = threadIdx.x; i < NQ * VP; i += NT) {
    const int q = i / VP, rc = i - q * VP, r = rc / IC, c = rc - r * IC;
    const float* col = sc + q * IR * IC + c;
    float a = 0.f;
    for (int k = 0; k < win.kh; ++k) a = fmaf(win.gh[k], col[(r + win.kh - 1 - k) * IC], a);
    v[i] = a;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BTH * BTW; i += NT) {
    const int r = i / BTW, c = i - r * BTW, gr = r0 + r, gc = c0 + c;
    if (gr >= s.H || gc >= s.W) continue;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < NQ; ++q) {
      const float* row = v + q * VP + r * IC + c;
      float a = 0.f;
      for (int k = 0; k < win.kw; ++k) a = fmaf(win.gw[k], row[win.kw - 1 - k], a);
      f[q] = a;
    }
    const int64_t o = plane * s.H * s.W + (int64_t)gr * s.W + gc;
    const float x = X[o], y = Y[o];
    float dx = f[0] + 2.f * x * f[1] + y * f[2];
    float dy = f[3] + 2.f * y * f[1] + x * f[2];
    if (nX) {
      const int64_t n = plane * nH * nW + (int64_t)((gr + (s.H & 1)) >> 1) * nW + ((gc + (s.W & 1)) >> 1);
      dx += 0.25f * nX[n];
      if (dY) dy += 0.25f * nY[n];
    }
    dX[o] = dx;
    if (dY) dY[o] = dy;
  }
}

// avg_pool2d(kernel 2, stride 2, padding (ph, pw)), count_include_pad: the in-range taps summed row by row, / 4
__global__ __launch_bounds__(NT) void avg_pool2_k(const float* __restrict__ X, int64_t nplanes, int H, int W, int ph, int pw, int Ho,
                                                  int Wo, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x, tot = nplanes * Ho * Wo;
  if (i >= tot) return;
  const int64_t plane = i / ((int64_t)Ho * Wo);
  const int rc = (int)(i - plane * Ho * Wo), r = rc / Wo, c = rc - r * Wo;
  const float* p = X + plane * H * W;
  float s = 0.f;
  for (int a = 2 * r - ph; a < 2 * r - ph + 2; ++a)
    for (int b = 2 * c - pw; b < 2 * c - pw + 2; ++b)
      if (a >= 0 && a < H && b >= 0 && b < W) s += p[(int64_t)a * W + b];
  out[i] = s / 4.f;
}

// V's patch term, standalone (the reference-lines route): wave p = patch p; value[0] = (sum_p ssim_p) / 4, d_rgb = its gradient
__global__ void patch_ssim_k(const float* __restrict__ rgb, const float* __restrict__ tgt, int P, float* __restrict__ value,
                             float* __restrict__ d_rgb) {
  __shared__ float part[16];
  const int p = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t off = (int64_t)p * CN_PATCH_SSIM_RAYS * 3;
  const float share = cn_patch_ssim_wave(rgb + off, tgt + off, CN_PATCH_SSIM_SCALE, d_rgb ? d_rgb + off : nullptr, lane);
  if (lane == 0) part[p] = share;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < P; ++k) s += part[k];
    value[0] = s / 4.f;
  }
}

bool make_shape(int64_t N, int64_t C, int64_t H, int64_t W, int win_size, float win_sigma, float C1, float C2, int tw, SsimShape* s,
                SsimWin* w) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || win_size <= 0 || win_size > CN_SSIM_MAX_WIN || win_size % 2 == 0 ||
      !(win_sigma > 0.f) || !(C1 >= 0.f) || !(C2 > 0.f) || N * C > 65535 || H > (1 << 20) || W > (1 << 20) || H * W > ((int64_t)1 << 31))
    return false;
  float g[CN_SSIM_MAX_WIN];
  cn_ssim_window(win_size, win_sigma, g);
  w->kh = H >= win_size ? win_size : 1;
  w->kw = W >= win_size ? win_size : 1;
  for (int k = 0; k < CN_SSIM_MAX_WIN; ++k) {
    w->gh[k] = w->kh == 1 ? (k == 0 ? 1.f : 0.f) : (k < win_size ? g[k] : 0.f);
    w->gw[k] = w->kw == 1 ? (k == 0 ? 1.f : 0.f) : (k < win_size ? g[k] : 0.f);
  }
  s->H = (int)H; s->W = (int)W; s->Ho = (int)(H - w->kh + 1); s->Wo = (int)(W - w->kw + 1);
  s->tiles_x = (int)cn_div_up(s->Wo, tw);
  s->ntiles = s->tiles_x * (int)cn_div_up(s->Ho, FTH);
  s->C1 = C1; s->C2 = C2;
  return true;
}

// the two forward launches of one level: per-tile fp64 partials, then the per-plane means (cs_nc nullable)
int launch_fwd(const float* X, const float* Y, const SsimShape& s, const SsimWin& w, int64_t planes, double* part, float* ssim_nc,
               float* cs_nc, void* stream) {
  const size_t lds = sizeof(float) * (size_t)(2 * (FTH + w.kh - 1) * (FTW + w.kw - 1) + 2 * 5 * FTH * (FTW + w.kw - 1));
  hipLaunchKernelGGL(ssim_tile_k<0>, dim3(s.ntiles, (unsigned)planes), dim3(NT), lds, cn_stream(stream), X, Y, s, w, part,
                     (float*)nullptr, (const float*)nullptr, 0.f, planes);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_fin_k, dim3((unsigned)planes), dim3(64), 0, cn_stream(stream), part, s.ntiles, (double)s.Ho * (double)s.Wo,
                     ssim_nc, cs_nc);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// the two backward launches of one level: the coefficient maps of a seed g on the mean of S (on_cs = false) or of cs (true), then
// the transposed filter + the pooled-back quarter of the next level's gradient nX / nY [planes, nH, nW] (nullable)
int launch_bwd(const float* X, const float* Y, const SsimShape& s, const SsimWin& w, int64_t planes, bool on_cs, const float* g,
               float* coef, float* dX, float* dY, const float* nX, const float* nY, int nH, int nW, void* stream) {
  const size_t lds_f = sizeof(float) * (size_t)(2 * (FTH + w.kh - 1) * (FTW + w.kw - 1) + 2 * 5 * FTH * (FTW + w.kw - 1));
  const float inv_cnt = (float)(1.0 / ((double)s.Ho * (double)s.Wo));
  if (on_cs)
    hipLaunchKernelGGL(ssim_tile_k<2>, dim3(s.ntiles, (unsigned)planes), dim3(NT), lds_f, cn_stream(stream), X, Y, s, w,
                       (double*)nullptr, coef, g, inv_cnt, planes);
  else
    hipLaunchKernelGGL(ssim_tile_k<1>, dim3(s.ntiles, (unsigned)planes), dim3(NT), lds_f, cn_stream(stream), X, Y, s, w,
                       (double*)nullptr, coef, g, inv_cnt, planes);
  CN_CHECK_LAUNCH();
  const int nq = dY ? 4 : 3;
  const size_t lds_b = sizeof(float) * (size_t)(nq * (BTH + w.kh - 1) * (BTW + w.kw - 1) + nq * BTH * (BTW + w.kw - 1));
  const int tiles = (int)(cn_div_up(s.W, BTW) * cn_div_up(s.H, BTH));
  hipLaunchKernelGGL(ssim_bwd_k, dim3(tiles, (unsigned)planes), dim3(NT), lds_b, cn_stream(stream), X, Y, s, w,
                     (const float*)coef, planes, dX, dY, nX, nY, nH, nW);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

constexpr int MS_MAX_LEVELS = 24;

// The MS-SSIM pyramid: level l's sides (l = 0 the input; each next one H / 2 + H % 2), shapes and windows, and where a level >= 1
// of one image starts inside a pyramid buffer [levels 1.. of X][levels 1.. of Y] (`half` floats each).
struct MsPlan {
  int levels;
  int64_t planes, off[MS_MAX_LEVELS], half, max_part, max_coef;
  SsimShape s[MS_MAX_LEVELS];
  SsimWin w[MS_MAX_LEVELS];
};

bool make_plan(int64_t N, int64_t C, int64_t H, int64_t W, int win_size, float win_sigma, float C1, float C2, int levels, MsPlan* p) {
  if (levels < 1 || levels > MS_MAX_LEVELS) return false;
  p->levels = levels; p->planes = N * C; p->half = 0; p->max_part = 0; p->max_coef = 0;
  for (int l = 0; l < levels; ++l) {
    if (H <= 0 || W <= 0 || !make_shape(N, C, H, W, win_size, win_sigma, C1, C2, FTW, &p->s[l], &p->w[l])) return false;
    p->off[l] = p->half;
    if (l > 0) p->half += p->planes * H * W;
    const int64_t part = 2 * p->planes * p->s[l].ntiles, coef = 4 * p->planes * p->s[l].Ho * p->s[l].Wo;
    p->max_part = part > p->max_part ? part : p->max_part;
    p->max_coef = coef > p->max_coef ? coef : p->max_coef;
    H = H / 2 + H % 2; W = W / 2 + W % 2;
  }
  return true;
}

}  // namespace

extern "C" int64_t cnerf_ssim_ws_floats(int64_t N, int64_t C, int64_t H, int64_t W, int win_size) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || win_size <= 0 || win_size > CN_SSIM_MAX_WIN) return 0;
  const int64_t Ho = H >= win_size ? H - win_size + 1 : H, Wo = W >= win_size ? W - win_size + 1 : W;
  return 2 * 2 * N * C * cn_div_up(Ho, FTH) * cn_div_up(Wo, FTW);     // fp64 pairs per tile
}

extern "C" int cnerf_ssim_fwd(const float* X, const float* Y, int64_t N, int64_t C, int64_t H, int64_t W, int win_size,
                              float win_sigma, float C1, float C2, float* ssim_nc, float* cs_nc, float* workspace, void* stream) {
  SsimShape s;
  SsimWin w;
  if (!X || !Y || !ssim_nc || !workspace || ((uintptr_t)workspace & 7) != 0 ||
      !make_shape(N, C, H, W, win_size, win_sigma, C1, C2, FTW, &s, &w))
    return CNERF_E_ARG;
  return launch_fwd(X, Y, s, w, N * C, reinterpret_cast<double*>(workspace), ssim_nc, cs_nc, stream);
}

extern "C" int64_t cnerf_ssim_bwd_ws_floats(int64_t N, int64_t C, int64_t H, int64_t W, int win_size) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || win_size <= 0 || win_size > CN_SSIM_MAX_WIN) return 0;
  const int64_t Ho = H >= win_size ? H - win_size + 1 : H, Wo = W >= win_size ? W - win_size + 1 : W;
  return 4 * N * C * Ho * Wo;
}

extern "C" int cnerf_ssim_bwd(const float* X, const float* Y, int64_t N, int64_t C, int64_t H, int64_t W, int win_size,
                              float win_sigma, float C1, float C2, const float* g_ssim, float* dX, float* dY, float* workspace,
                              void* stream) {
  SsimShape s;
  SsimWin w;
  if (!X || !Y || !g_ssim || !dX || !workspace || !make_shape(N, C, H, W, win_size, win_sigma, C1, C2, FTW, &s, &w))
    return CNERF_E_ARG;
  return launch_bwd(X, Y, s, w, N * C, false, g_ssim, workspace, dX, dY, nullptr, nullptr, 0, 0, stream);
}

extern "C" int cnerf_avg_pool2(const float* X, int64_t N, int64_t C, int64_t H, int64_t W, float* out, void* stream) {
  if (!X || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > (1 << 20) || W > (1 << 20)) return CNERF_E_ARG;
  const int ph = (int)(H % 2), pw = (int)(W % 2);
  const int Ho = (int)((H + 2 * ph - 2) / 2 + 1), Wo = (int)((W + 2 * pw - 2) / 2 + 1);
  const int64_t tot = N * C * Ho * Wo;
  hipLaunchKernelGGL(avg_pool2_k, dim3((unsigned)cn_div_up(tot, NT)), dim3(NT), 0, cn_stream(stream), X, N * C, (int)H, (int)W, ph, pw,
                     Ho, Wo, out);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// ---- MS-SSIM: the level walk.  Forward: cnerf_ssim_fwd's two launches per level and cnerf_avg_pool2's in between (the same bits as
// that sequence of calls), the pooled levels kept in `pyr`.  Backward: from the last level down, one coefficient launch (the last
// level's seed is on the mean of S, every other level's on the mean of cs) and one transposed-filter launch per level, which also
// adds the pooled-back quarter of the level after it: no un-pool pass, no atomics, nothing read back.
extern "C" int64_t cnerf_msssim_ws_floats(int64_t N, int64_t C, int64_t H, int64_t W, int win_size, int levels) {
  MsPlan p;
  return make_plan(N, C, H, W, win_size, 1.5f, 0.f, 1.f, levels, &p) ? 2 * p.max_part : 0;     // fp64 pairs per tile
}

extern "C" int cnerf_msssim_fwd(const float* X, const float* Y, int64_t N, int64_t C, int64_t H, int64_t W, int win_size,
                                float win_sigma, float C1, float C2, int levels, float* v, float* pyr, float* workspace,
                                void* stream) {
  MsPlan p;
  if (!X || !Y || !v || !pyr || !workspace || ((uintptr_t)workspace & 7) != 0 ||
      !make_plan(N, C, H, W, win_size, win_sigma, C1, C2, levels, &p))
    return CNERF_E_ARG;
  const float *x = X, *y = Y;
  for (int l = 0; l < levels; ++l) {
    const bool last = l == levels - 1;
    // below the last level the mean of S lands in v's last row, which the last level then overwrites
    int rc = launch_fwd(x, y, p.s[l], p.w[l], p.planes, reinterpret_cast<double*>(workspace), v + (levels - 1) * p.planes,
                        last ? nullptr : v + l * p.planes, stream);
    if (rc != CNERF_OK) return rc;
    if (!last) {
      float *nx = pyr + p.off[l + 1], *ny = pyr + p.half + p.off[l + 1];
      if ((rc = cnerf_avg_pool2(x, N, C, p.s[l].H, p.s[l].W, nx, stream)) != CNERF_OK) return rc;
      if ((rc = cnerf_avg_pool2(y, N, C, p.s[l].H, p.s[l].W, ny, stream)) != CNERF_OK) return rc;
      x = nx; y = ny;
    }
  }
  return CNERF_OK;
}

extern "C" int64_t cnerf_msssim_bwd_ws_floats(int64_t N, int64_t C, int64_t H, int64_t W, int win_size, int levels) {
  MsPlan p;
  return make_plan(N, C, H, W, win_size, 1.5f, 0.f, 1.f, levels, &p) ? p.max_coef + 2 * p.half : 0;
}

extern "C" int cnerf_msssim_bwd(const float* X, const float* Y, int64_t N, int64_t C, int64_t H, int64_t W, int win_size,
                                float win_sigma, float C1, float C2, int levels, const float* pyr, const float* g_v, float* dX,
                                float* dY, float* workspace, void* stream) {
  MsPlan p;
  if (!X || !Y || !pyr || !g_v || !dX || !workspace || !make_plan(N, C, H, W, win_size, win_sigma, C1, C2, levels, &p))
    return CNERF_E_ARG;
  float *coef = workspace, *wdx = workspace + p.max_coef, *wdy = wdx + p.half;    // the coarser levels' dX / dY, pyr's layout
  for (int l = levels - 1; l >= 0; --l) {
    const bool last = l == levels - 1;
    const float* x = l ? pyr + p.off[l] : X;
    const float* y = l ? pyr + p.half + p.off[l] : Y;
    float* dx = l ? wdx + p.off[l] : dX;
    float* dy = dY ? (l ? wdy + p.off[l] : dY) : nullptr;
    const int rc = launch_bwd(x, y, p.s[l], p.w[l], p.planes, !last, g_v + l * p.planes, coef, dx, dy,
                              last ? nullptr : wdx + p.off[l + 1], (last || !dY) ? nullptr : wdy + p.off[l + 1],
                              last ? 0 : p.s[l + 1].H, last ? 0 : p.s[l + 1].W, stream);
    if (rc != CNERF_OK) return rc;
  }
  return CNERF_OK;
}

extern "C" int cnerf_patch_ssim_loss(const float* rgb, const float* target, int P, float* value, float* d_rgb, void* stream) {
  if (!rgb || !target || !value || P <= 0 || P > 16) return CNERF_E_ARG;
  hipLaunchKernelGGL(patch_ssim_k, dim3(1), dim3(64 * P), 0, cn_stream(stream), rgb, target, P, value, d_rgb);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
