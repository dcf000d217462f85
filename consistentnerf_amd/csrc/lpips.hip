// LPIPS (the `lpips` package's LPIPS(net='vgg'), version 0.1, eval mode, spatial=False, lpips=True; the reference's V:40, V:1699-1728,
// V:2055-2087) on [N, 3, H, W] fp32 images, forward and input gradient.  The statement is DESIGN.md §4e.  Every tensor is NCHW.
//   conv3x3_k      3x3 / pad 1 / stride 1 convolution as an implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): rows =
//                  output channels (A operand: weight panels [K/8][9 taps][Mp][8], one 16-byte load = 4 k-steps), columns = 128
//                  pixels of a block (B operand), K = input channels x 9 taps.  A block owns TI images x TH x TW pixels (powers of
//                  two, product 128: 1 x 8 x 16 on a large image, 128 x 1 x 1 on 1 x 1 maps), stages 8 input channels of that tile
//                  plus its halo in LDS once for the nine taps, and each of its 4 waves holds 64 channels x 32 pixels in two
//                  accumulators.  The same kernel is the input gradient: panels packed transposed with the taps rotated, the
//                  incoming gradient gated by the layer's stored output (> 0) while it is staged.
//   split K        small maps leave few pixel tiles against up to 9.4 MB of weights per layer, so the channel chunks are split over
//                  gridDim.z; every split writes its partial sums at a fixed index and conv_reduce_k adds them in split order (+ bias,
//                  ReLU).  The split count depends on the layer's channels and map size only, never on the batch: one image alone
//                  and the same image inside a batch give identical bits, and so does every call (no atomics anywhere).
//   Branch rules   ReLU backward passes where the stored output is > 0.  The 2x2 / stride 2 max pool (floor) takes the first maximum in
//                  row-major order under strict > (ATen's rule; a NaN is taken), the backward recomputes that choice from the stored
//                  input.  At a pixel whose feature column is all zero the value follows the formula (0 / 1e-10 = 0) and the gradient
//                  through the normalisation is DEFINED as 0 (autograd yields 0 * inf = NaN there).
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int LP_LAYERS = 13, LP_TAPS = 5;
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_TAP_LAYER[LP_TAPS] = {1, 3, 6, 9, 12};
constexpr int LP_TAP_C[LP_TAPS] = {64, 128, 256, 512, 512};
constexpr int64_t LP_MAX_SIDE = 8192, LP_MAX_N = 65535;

inline bool lp_pool_before(int l) { return l == 2 || l == 4 || l == 7 || l == 10; }
inline int lp_tap_of(int l) { return l == 1 ? 0 : l == 3 ? 1 : l == 6 ? 2 : l == 9 ? 3 : l == 12 ? 4 : -1; }
inline int64_t r4(int64_t v) { return cn_round_up(v, 4); }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---- convolution ---------------------------------------------------------------------------------------------------------------
struct ConvP {
  const float* in;      // [N, K, H, W]
  const float* gate;    // nullable, [N, K, H, W]: `in` counts only where gate > 0 (the ReLU backward)
  const float* panel;   // [nch][9][MP][8]
  const float* bias;    // nullable, [M]
  float* out;           // [N, M, H, W]
  float* part;          // nullable: [splits][N, M, H, W]
  int N, K, M, MP, H, W, ltw, lth, TI, tiles_x, tiles_y, nch, cps, relu;
  int64_t total;
};

constexpr int CONV_LDS = 8 * 128 * 9;   // 8 channels x (TI (TH + 2) (TW + 2) <= 128 x 9) floats

__global__ __launch_bounds__(NT) void conv3x3_k(ConvP p) {
  __shared__ float lds[CONV_LDS];
  const int TW = 1 << p.ltw, TH = 1 << p.lth, PW = TW + 2, PH = TH + 2, TI = p.TI;
  const int bx = blockIdx.x, tx = bx % p.tiles_x, t2 = bx / p.tiles_x, ty = t2 % p.tiles_y, ig = t2 / p.tiles_y;
  const int x0 = tx * TW, y0 = ty * TH, n0 = ig * TI;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, hh = lane >> 5;
  const int q = wave * 32 + i, lx = q & (TW - 1), ly = (q >> p.ltw) & (TH - 1), li = q >> (p.ltw + p.lth);
  const int cs = TI * PH * PW;                                  // LDS floats per staged channel
  const int pbase = (li * PH + ly) * PW + lx + 4 * hh * cs;     // this lane's pixel at tap (0, 0), channel 4 hh of the chunk
  const int m0 = blockIdx.y * 64;
  const int c_lo = blockIdx.z * p.cps, c_hi = min(p.nch, c_lo + p.cps);
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  for (int ch = c_lo; ch < c_hi; ++ch) {
    __syncthreads();
    for (int e = threadIdx.x; e < 8 * cs; e += NT) {
      const int c = e / cs, r = e - c * cs, im = r / (PH * PW), r2 = r - im * PH * PW, yy = r2 / PW, xx = r2 - yy * PW;
      const int n = n0 + im, k = ch * 8 + c, gy = y0 + yy - 1, gx = x0 + xx - 1;
      float v = 0.f;
      if (n < p.N && k < p.K && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
        const int64_t idx = (((int64_t)n * p.K + k) * p.H + gy) * p.W + gx;
        v = p.in[idx];
        if (p.gate && !(p.gate[idx] > 0.f)) v = 0.f;
      }
      lds[e] = v;
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap % 3;
      if ((p.H == 1 && dy != 1) || (p.W == 1 && dx != 1)) continue;   // every pixel of this tap is padding
      const float* ap = p.panel + ((((int64_t)ch * 9 + tap) * p.MP + m0 + i) * 8 + 4 * hh);
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(ap + 32 * 8);
      const float* bp = lds + pbase + dy * PW + dx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = bp[j * cs];
        acc0 = mfma(a0[j], b, acc0);
        acc1 = mfma(a1[j], b, acc1);
      }
    }
  }
  const int n = n0 + li, y = y0 + ly, x = x0 + lx;
  if (n >= p.N || y >= p.H || x >= p.W) return;
  float* dst = p.part ? p.part + (int64_t)blockIdx.z * p.total : p.out;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (co >= p.M) continue;
      float v = t == 0 ? acc0[r] : acc1[r];
      if (!p.part) {
        if (p.bias) v += p.bias[co];
        if (p.relu) v = v > 0.f ? v : 0.f;
      }
      dst[(((int64_t)n * p.M + co) * p.H + y) * p.W + x] = v;
    }
  }
}

// the partial sums of the K splits in split order, + bias, ReLU
__global__ __launch_bounds__(NT) void conv_reduce_k(const float* __restrict__ part, int splits, int64_t total, const float* __restrict__ bias,
                                                    int M, int64_t HW, int relu, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  float s = part[idx];
  for (int k = 1; k < splits; ++k) s += part[(int64_t)k * total + idx];
  if (bias) s += bias[(idx / HW) % M];
  if (relu) s = s > 0.f ? s : 0.f;
  out[idx] = s;
}

// w [Cout, Cin, 3, 3] -> panel[chunk][tap][MP][8].  Forward: row m = output channel, k = input channel, the tap as stored.
// Transposed (input gradient): row m = input channel, k = output channel, the tap rotated by 180 degrees.
__global__ __launch_bounds__(NT) void conv_pack_k(const float* __restrict__ w, int Cin, int Cout, int transposed, int MP, int64_t total,
                                                  float* __restrict__ panel) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx & 7), m = (int)((idx >> 3) % MP);
  const int64_t ct = (idx >> 3) / MP;
  const int tap = (int)(ct % 9), k = (int)(ct / 9) * 8 + j;
  const int M = transposed ? Cin : Cout, K = transposed ? Cout : Cin;
  float v = 0.f;
  if (m < M && k < K) v = transposed ? w[((int64_t)k * Cin + m) * 9 + (8 - tap)] : w[((int64_t)m * Cin + k) * 9 + tap];
  panel[idx] = v;
}

inline int p2_log(int64_t v, int cap_log) {   // log2 of the smallest power of two >= v, capped
  int l = 0;
  while (l < cap_log && ((int64_t)1 << l) < v) ++l;
  return l;
}

inline int conv_splits(int64_t K, int64_t H, int64_t W) {   // a function of the layer alone (see the header comment)
  const int64_t nch = cn_div_up(K, 8), hw = H * W;
  if (hw >= 256) return 1;
  const int64_t want = 256 / hw < 16 ? 256 / hw : 16;
  const int64_t s = want < nch ? want : nch;
  const int64_t cps = cn_div_up(nch, s);
  return (int)cn_div_up(nch, cps);
}

inline int64_t conv_part_floats(int64_t N, int64_t K, int64_t M, int64_t H, int64_t W) {
  const int s = conv_splits(K, H, W);
  return s > 1 ? r4((int64_t)s * N * M * H * W) : 0;
}

inline int64_t panel_floats(int64_t K, int64_t M) { return cn_div_up(K, 8) * 9 * cn_round_up(M, 64) * 8; }

inline bool conv_shape_ok(int64_t N, int64_t K, int64_t M, int64_t H, int64_t W) {
  return N > 0 && K > 0 && M > 0 && H > 0 && W > 0 && N <= 2 * LP_MAX_N && K <= 4096 && M <= 4096 && H <= LP_MAX_SIDE && W <= LP_MAX_SIDE &&
         N * (K > M ? K : M) * H * W < ((int64_t)1 << 40);
}

// out[N, M, H, W] = conv(in[N, K, H, W]) with the panel of (K, M); part: conv_part_floats() floats where that is > 0
int launch_conv(const float* in, const float* gate, const float* panel, const float* bias, int relu, int64_t N, int64_t K, int64_t M,
                int64_t H, int64_t W, float* out, float* part, hipStream_t st) {
  ConvP p;
  p.in = in; p.gate = gate; p.panel = panel; p.bias = bias; p.out = out;
  p.N = (int)N; p.K = (int)K; p.M = (int)M; p.MP = (int)cn_round_up(M, 64); p.H = (int)H; p.W = (int)W;
  p.ltw = p2_log(W, 4);
  p.lth = p2_log(H, 3);
  p.TI = 128 >> (p.ltw + p.lth);
  p.tiles_x = (int)cn_div_up(W, 1 << p.ltw);
  p.tiles_y = (int)cn_div_up(H, 1 << p.lth);
  p.nch = (int)cn_div_up(K, 8);
  const int splits = conv_splits(K, H, W);
  p.cps = (int)cn_div_up(p.nch, splits);
  p.relu = relu;
  p.total = N * M * H * W;
  p.part = splits > 1 ? part : nullptr;
  if (splits > 1 && !part) return CNERF_E_ARG;
  const int64_t gx = cn_div_up(N, p.TI) * p.tiles_x * p.tiles_y;
  if (gx > 0x7fffffff) return CNERF_E_ARG;
  hipLaunchKernelGGL(conv3x3_k, dim3((unsigned)gx, (unsigned)(p.MP / 64), (unsigned)splits), dim3(NT), 0, st, p);
  CN_CHECK_LAUNCH();
  if (splits > 1) {
    hipLaunchKernelGGL(conv_reduce_k, dim3((unsigned)cn_div_up(p.total, NT)), dim3(NT), 0, st, part, splits, p.total, bias, (int)M, H * W,
                       relu, out);
    CN_CHECK_LAUNCH();
  }
  return CNERF_OK;
}

// ---- max pool --------------------------------------------------------------------------------------------------------------------
// first maximum of the 2x2 window at (r, c) of plane p in row-major order under strict > (a NaN is taken, as ATen does)
__device__ __forceinline__ int pool_pick(const float* __restrict__ p, int W, int r, int c, float* best) {
  const float* q = p + (int64_t)r * W + c;
  float m = q[0];
  int a = 0;
  float v = q[1];
  if (v > m || v != v) { m = v; a = 1; }
  v = q[W];
  if (v > m || v != v) { m = v; a = 2; }
  v = q[W + 1];
  if (v > m || v != v) { m = v; a = 3; }
  *best = m;
  return a;
}

__global__ __launch_bounds__(NT) void maxpool2_fwd_k(const float* __restrict__ X, int64_t planes, int H, int W, float* __restrict__ out) {
  const int Ho = H / 2, Wo = W / 2;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= planes * Ho * Wo) return;
  const int64_t pl = i / ((int64_t)Ho * Wo);
  const int rc = (int)(i - pl * Ho * Wo), r = rc / Wo, c = rc - r * Wo;
  float m;
  pool_pick(X + pl * H * W, W, 2 * r, 2 * c, &m);
  out[i] = m;
}

// dX = the pool's input gradient (+ add, nullable: a second gradient of the same tensor; add may alias dX)
__global__ __launch_bounds__(NT) void maxpool2_bwd_k(const float* __restrict__ X, const float* __restrict__ g, const float* add, int64_t planes,
                                                     int H, int W, float* dX) {
  const int Ho = H / 2, Wo = W / 2;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= planes * H * W) return;
  const int64_t pl = i / ((int64_t)H * W);
  const int rc = (int)(i - pl * H * W), y = rc / W, x = rc - y * W, r = y >> 1, c = x >> 1;
  float v = 0.f;
  if (r < Ho && c < Wo) {
    float m;
    const int a = pool_pick(X + pl * H * W, W, 2 * r, 2 * c, &m);
    if (a == (y & 1) * 2 + (x & 1)) v = g[pl * Ho * Wo + (int64_t)r * Wo + c];
  }
  if (add) v = add[i] + v;
  dX[i] = v;
}

// ---- scaling layer ---------------------------------------------------------------------------------------------------------------
// in0[b] = (X[b] - shift) / scale for b < Np, (Y[b - Np] - shift) / scale above; sc = {shift[3], scale[3]}
__global__ __launch_bounds__(NT) void lp_scale_k(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ sc,
                                                 int64_t Np, int64_t HW, float* __restrict__ in0) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x, half = Np * 3 * HW;
  if (i >= 2 * half) return;
  const int c = (int)((i / HW) % 3);
  const float v = i < half ? X[i] : Y[i - half];
  in0[i] = (v - sc[c]) / sc[3 + c];
}

__global__ __launch_bounds__(NT) void lp_unscale_k(const float* __restrict__ g, const float* __restrict__ sc, int64_t total, int64_t HW,
                                                   float* __restrict__ dX) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  dX[i] = g[i] / sc[3 + (int)((i / HW) % 3)];
}

// ---- V's patch LPIPS term inside the folded step (cnerf_lpips_pack_patches / cnerf_lpips_seeds) -------------------------------------
// The patch rays of every level as ONE LPIPS batch: image lv * P + p = patch p of level lv (0 = the last level, 1 = coarse), read from
// the ray-major [B, 3] maps as the reference's [1, 16, 16, 3] -> permute(0, 3, 1, 2) does: pred[img][c][y][x] = (rgb[p 256 + y 16 + x][c]
// - 0.5) * 2 (V:1702-1705), gt the same of the target, repeated per level.  One thread per output element.
__global__ __launch_bounds__(NT) void lp_pack_patches_k(const float* __restrict__ rgb0, const float* __restrict__ rgb1,
                                                        const float* __restrict__ tgt, int P, int total, float* __restrict__ pred,
                                                        float* __restrict__ gt) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int img = i / 768, c = (i % 768) / 256, r = i % 256;
  const int lv = img / P, p = img - lv * P;
  const int64_t src = ((int64_t)p * 256 + r) * 3 + c;
  pred[i] = ((lv ? rgb1 : rgb0)[src] - 0.5f) * 2.f;
  gt[i] = (tgt[src] - 0.5f) * 2.f;
}

// seeds[i] = (g * lpips_w) * 0.25: autograd's own steps from the loss to the per-image LPIPS values (loss += lpips_w (sum_p v_p / 4))
__global__ __launch_bounds__(64) void lp_seeds_k(const float* __restrict__ g, float lpips_w, int n, float* __restrict__ seeds) {
  if ((int)threadIdx.x < n) seeds[threadIdx.x] = ((g ? g[0] : 1.f) * lpips_w) * 0.25f;
}

// ---- head ------------------------------------------------------------------------------------------------------------------------
// One thread per pixel of pair n: F0 / F1 = [N, C, HW] feature sets; part[n * nblk + block] = the block's sum over its pixels of
// sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2, in fp64.
__global__ __launch_bounds__(NT) void lp_head_fwd_k(const float* __restrict__ F0, const float* __restrict__ F1, const float* __restrict__ lin,
                                                    int C, int64_t HW, double* __restrict__ part) {
  __shared__ double red[NT / 64];
  const int64_t n = blockIdx.y, pix = (int64_t)blockIdx.x * NT + threadIdx.x;
  double acc = 0.0;
  if (pix < HW) {
    const float* f0 = F0 + n * C * HW + pix;
    const float* f1 = F1 + n * C * HW + pix;
    double s0 = 0.0, s1 = 0.0;
    for (int c = 0; c < C; ++c) {
      const double a = f0[c * HW], b = f1[c * HW];
      s0 += a * a; s1 += b * b;
    }
    const double i0 = 1.0 / (sqrt(s0) + 1e-10), i1 = 1.0 / (sqrt(s1) + 1e-10);
    for (int c = 0; c < C; ++c) {
      const double d = f0[c * HW] * i0 - f1[c * HW] * i1;
      acc += (double)lin[c] * d * d;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct HeadFin {
  int64_t off[LP_TAPS];   // doubles into part
  int nblk[LP_TAPS];
  double hw[LP_TAPS];
  int ntaps;
};

// one wave per pair n: each tap's partials in index order / HW -> per_tap[t * ldt + n] (nullable), their sum -> value[n]
__global__ __launch_bounds__(64) void lp_head_fin_k(const double* __restrict__ part, HeadFin f, int64_t Np, int64_t ldt, float* __restrict__ value,
                                                    float* __restrict__ per_tap) {
  const int64_t n = blockIdx.x;
  double tot = 0.0;
  for (int t = 0; t < f.ntaps; ++t) {
    double a = 0.0;
    for (int k = threadIdx.x; k < f.nblk[t]; k += 64) a += part[f.off[t] + n * f.nblk[t] + k];
    a = wave_sum(a) / f.hw[t];
    if (per_tap && threadIdx.x == 0) per_tap[t * ldt + n] = (float)a;
    tot += a;
  }
  if (threadIdx.x == 0) value[n] = (float)tot;
}

// dF0[n, c, pix] = g[n] / HW * d/df0 of the head's sum at that pixel; 0 where f0 is all zero (see the header comment)
__global__ __launch_bounds__(NT) void lp_head_bwd_k(const float* __restrict__ F0, const float* __restrict__ F1, const float* __restrict__ lin,
                                                    const float* __restrict__ g, int C, int64_t HW, float* __restrict__ dF0) {
  const int64_t n = blockIdx.y, pix = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (pix >= HW) return;
  const float* f0 = F0 + n * C * HW + pix;
  const float* f1 = F1 + n * C * HW + pix;
  float* d0 = dF0 + n * C * HW + pix;
  double s0 = 0.0, s1 = 0.0;
  for (int c = 0; c < C; ++c) {
    const double a = f0[c * HW], b = f1[c * HW];
    s0 += a * a; s1 += b * b;
  }
  if (s0 == 0.0) {
    for (int c = 0; c < C; ++c) d0[c * HW] = 0.f;
    return;
  }
  const double r0 = sqrt(s0), i0 = 1.0 / (r0 + 1e-10), i1 = 1.0 / (sqrt(s1) + 1e-10);
  double T = 0.0;
  for (int c = 0; c < C; ++c) {
    const double a = f0[c * HW];
    T += (double)lin[c] * (a * i0 - f1[c * HW] * i1) * a;
  }
  const double coef = 2.0 * (double)g[n] / (double)HW * i0, back = T * i0 / r0;
  for (int c = 0; c < C; ++c) {
    const double a = f0[c * HW];
    d0[c * HW] = (float)(coef * ((double)lin[c] * (a * i0 - f1[c * HW] * i1) - back * a));
  }
}

// ---- the packed network and the workspace ---------------------------------------------------------------------------------------
struct LpPacked {
  int64_t fwd[LP_LAYERS], bwd[LP_LAYERS], bias[LP_LAYERS], lin[LP_TAPS], sc, total;
};

LpPacked lp_packed() {
  LpPacked k;
  int64_t o = 0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    k.fwd[l] = o; o += panel_floats(LP_CIN[l], LP_COUT[l]);
    k.bwd[l] = o; o += panel_floats(LP_COUT[l], LP_CIN[l]);
    k.bias[l] = o; o += r4(LP_COUT[l]);
  }
  for (int t = 0; t < LP_TAPS; ++t) { k.lin[t] = o; o += r4(LP_TAP_C[t]); }
  k.sc = o; o += 8;
  k.total = o;
  return k;
}

struct LpWs {
  int64_t B2;                       // images a forward pass holds at once: 2 N kept, 2 streamed
  int64_t h[LP_LAYERS], w[LP_LAYERS];
  int64_t in0, act[LP_LAYERS], pool[4], bufA, bufB, part, head, g0, g1, total;
  HeadFin fin;
};

bool lp_shape_ok(int64_t N, int64_t H, int64_t W) {
  return N > 0 && N <= LP_MAX_N && H >= 16 && W >= 16 && H <= LP_MAX_SIDE && W <= LP_MAX_SIDE && N * H * W < ((int64_t)1 << 31);
}

LpWs lp_ws(int64_t N, int64_t H, int64_t W, int keep) {
  LpWs s;
  s.B2 = keep ? 2 * N : 2;
  int64_t hh = H, ww = W, o = 0, maxact = 0, maxpart = 0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    if (lp_pool_before(l)) { hh /= 2; ww /= 2; }
    s.h[l] = hh; s.w[l] = ww;
    const int64_t a = LP_COUT[l] * hh * ww;
    if (a > maxact) maxact = a;
    int64_t pf = conv_part_floats(s.B2, LP_CIN[l], LP_COUT[l], hh, ww);
    if (pf > maxpart) maxpart = pf;
    if (keep) {
      pf = conv_part_floats(N, LP_COUT[l], LP_CIN[l], hh, ww);
      if (pf > maxpart) maxpart = pf;
    }
  }
  s.in0 = o; o += r4(s.B2 * 3 * H * W);
  s.bufA = s.bufB = s.g0 = s.g1 = -1;
  for (int k = 0; k < 4; ++k) s.pool[k] = -1;
  if (keep) {
    int k = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
      if (lp_pool_before(l)) { s.pool[k++] = o; o += r4(s.B2 * LP_CIN[l] * s.h[l] * s.w[l]); }
      s.act[l] = o; o += r4(s.B2 * LP_COUT[l] * s.h[l] * s.w[l]);
    }
    s.g0 = o; o += r4(N * maxact);
    s.g1 = o; o += r4(N * maxact);
  } else {
    for (int l = 0; l < LP_LAYERS; ++l) s.act[l] = -1;
    s.bufA = o; o += r4(2 * maxact);
    s.bufB = o; o += r4(2 * maxact);
  }
  s.part = o; o += maxpart;
  s.head = o;
  const int64_t pairs = keep ? N : 1;
  int64_t d = 0;
  s.fin.ntaps = LP_TAPS;
  for (int t = 0; t < LP_TAPS; ++t) {
    const int l = LP_TAP_LAYER[t];
    const int64_t hw = s.h[l] * s.w[l];
    s.fin.off[t] = d;
    s.fin.nblk[t] = (int)cn_div_up(hw, NT);
    s.fin.hw[t] = (double)hw;
    d += pairs * s.fin.nblk[t];
  }
  o += r4(2 * d);
  s.total = o;
  return s;
}

int launch_pool_fwd(const float* X, int64_t planes, int64_t H, int64_t W, float* out, hipStream_t st) {
  const int64_t tot = planes * (H / 2) * (W / 2);
  if (tot <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(maxpool2_fwd_k, dim3((unsigned)cn_div_up(tot, NT)), dim3(NT), 0, st, X, planes, (int)H, (int)W, out);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

int launch_pool_bwd(const float* X, const float* g, const float* add, int64_t planes, int64_t H, int64_t W, float* dX, hipStream_t st) {
  hipLaunchKernelGGL(maxpool2_bwd_k, dim3((unsigned)cn_div_up(planes * H * W, NT)), dim3(NT), 0, st, X, g, add, planes, (int)H, (int)W, dX);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// one pass of the trunk + heads over `pairs` image pairs held as a batch of 2 * pairs in `in0`; values land at value[0 .. pairs)
int lp_trunk(const float* pk, const LpPacked& k, const LpWs& s, float* ws, int keep, int64_t pairs, float* value, float* per_tap,
             int64_t ldt, hipStream_t st) {
  const int64_t B = 2 * pairs;
  float* bufA = keep ? nullptr : ws + s.bufA;
  float* bufB = keep ? nullptr : ws + s.bufB;
  const float* x = ws + s.in0;
  double* hpart = reinterpret_cast<double*>(ws + s.head);
  auto other = [&](const float* cur) { return cur == bufA ? bufB : bufA; };
  int pool = 0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    const int64_t h = s.h[l], w = s.w[l];
    if (lp_pool_before(l)) {
      float* o = keep ? ws + s.pool[pool] : other(x);
      ++pool;
      const int rc = launch_pool_fwd(x, B * LP_CIN[l], s.h[l - 1], s.w[l - 1], o, st);
      if (rc) return rc;
      x = o;
    }
    float* o = keep ? ws + s.act[l] : other(x);
    const int rc = launch_conv(x, nullptr, pk + k.fwd[l], pk + k.bias[l], 1, B, LP_CIN[l], LP_COUT[l], h, w, o, ws + s.part, st);
    if (rc) return rc;
    x = o;
    const int t = lp_tap_of(l);
    if (t >= 0) {
      const int C = LP_COUT[l];
      hipLaunchKernelGGL(lp_head_fwd_k, dim3((unsigned)s.fin.nblk[t], (unsigned)pairs), dim3(NT), 0, st, x, x + pairs * C * h * w,
                         pk + k.lin[t], C, h * w, hpart + s.fin.off[t]);
      CN_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(lp_head_fin_k, dim3((unsigned)pairs), dim3(64), 0, st, hpart, s.fin, pairs, ldt, value, per_tap);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

}  // namespace

// ---- stand-alone convolution / pool / head ---------------------------------------------------------------------------------------
extern "C" int64_t cnerf_conv3x3_packed_floats(int64_t Cin, int64_t Cout, int transposed) {
  if (Cin <= 0 || Cout <= 0 || Cin > 4096 || Cout > 4096) return 0;
  return transposed ? panel_floats(Cout, Cin) : panel_floats(Cin, Cout);
}

extern "C" int cnerf_conv3x3_pack(const float* w, int64_t Cin, int64_t Cout, int transposed, float* panel, void* stream) {
  if (!w || !panel || Cin <= 0 || Cout <= 0 || Cin > 4096 || Cout > 4096) return CNERF_E_ARG;
  const int64_t tot = cnerf_conv3x3_packed_floats(Cin, Cout, transposed);
  hipLaunchKernelGGL(conv_pack_k, dim3((unsigned)cn_div_up(tot, NT)), dim3(NT), 0, cn_stream(stream), w, (int)Cin, (int)Cout, transposed ? 1 : 0,
                     (int)cn_round_up(transposed ? Cin : Cout, 64), tot, panel);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int64_t cnerf_conv3x3_ws_floats(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W) {
  if (!conv_shape_ok(N, Cin, Cout, H, W)) return 0;
  const int64_t a = conv_part_floats(N, Cin, Cout, H, W), b = conv_part_floats(N, Cout, Cin, H, W);
  return a > b ? a : b;
}

extern "C" int cnerf_conv3x3_fwd(const float* in, const float* panel, const float* bias, int64_t N, int64_t Cin, int64_t Cout, int64_t H,
                                 int64_t W, int relu, float* out, float* workspace, void* stream) {
  if (!in || !panel || !out || !conv_shape_ok(N, Cin, Cout, H, W)) return CNERF_E_ARG;
  return launch_conv(in, nullptr, panel, bias, relu ? 1 : 0, N, Cin, Cout, H, W, out, workspace, cn_stream(stream));
}

extern "C" int cnerf_conv3x3_dgrad(const float* g_out, const float* gate, const float* panel_t, int64_t N, int64_t Cin, int64_t Cout,
                                   int64_t H, int64_t W, float* d_in, float* workspace, void* stream) {
  if (!g_out || !panel_t || !d_in || !conv_shape_ok(N, Cin, Cout, H, W)) return CNERF_E_ARG;
  return launch_conv(g_out, gate, panel_t, nullptr, 0, N, Cout, Cin, H, W, d_in, workspace, cn_stream(stream));
}

extern "C" int cnerf_maxpool2_fwd(const float* X, int64_t N, int64_t C, int64_t H, int64_t W, float* out, void* stream) {
  if (!X || !out || N <= 0 || C <= 0 || H < 2 || W < 2 || H > LP_MAX_SIDE || W > LP_MAX_SIDE || N * C > ((int64_t)1 << 31)) return CNERF_E_ARG;
  return launch_pool_fwd(X, N * C, H, W, out, cn_stream(stream));
}

extern "C" int cnerf_maxpool2_bwd(const float* X, const float* g_out, const float* add, int64_t N, int64_t C, int64_t H, int64_t W,
                                  float* dX, void* stream) {
  if (!X || !g_out || !dX || N <= 0 || C <= 0 || H < 2 || W < 2 || H > LP_MAX_SIDE || W > LP_MAX_SIDE || N * C > ((int64_t)1 << 31))
    return CNERF_E_ARG;
  return launch_pool_bwd(X, g_out, add, N * C, H, W, dX, cn_stream(stream));
}

extern "C" int64_t cnerf_lpips_head_ws_floats(int64_t N, int64_t H, int64_t W) {
  if (N <= 0 || H <= 0 || W <= 0 || H > LP_MAX_SIDE || W > LP_MAX_SIDE) return 0;
  return 2 * N * cn_div_up(H * W, NT);
}

extern "C" int cnerf_lpips_head_fwd(const float* F0, const float* F1, const float* lin, int64_t N, int64_t C, int64_t H, int64_t W,
                                    float* value, float* workspace, void* stream) {
  if (!F0 || !F1 || !lin || !value || !workspace || ((uintptr_t)workspace & 7) != 0 || N <= 0 || N > LP_MAX_N || C <= 0 || C > 4096 ||
      H <= 0 || W <= 0 || H > LP_MAX_SIDE || W > LP_MAX_SIDE)
    return CNERF_E_ARG;
  HeadFin f;
  f.ntaps = 1; f.off[0] = 0; f.nblk[0] = (int)cn_div_up(H * W, NT); f.hw[0] = (double)(H * W);
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(lp_head_fwd_k, dim3((unsigned)f.nblk[0], (unsigned)N), dim3(NT), 0, cn_stream(stream), F0, F1, lin, (int)C, H * W, part);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(lp_head_fin_k, dim3((unsigned)N), dim3(64), 0, cn_stream(stream), part, f, N, N, value, (float*)nullptr);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_lpips_head_bwd(const float* F0, const float* F1, const float* lin, const float* g, int64_t N, int64_t C, int64_t H,
                                    int64_t W, float* dF0, void* stream) {
  if (!F0 || !F1 || !lin || !g || !dF0 || N <= 0 || N > LP_MAX_N || C <= 0 || C > 4096 || H <= 0 || W <= 0 || H > LP_MAX_SIDE ||
      W > LP_MAX_SIDE)
    return CNERF_E_ARG;
  hipLaunchKernelGGL(lp_head_bwd_k, dim3((unsigned)cn_div_up(H * W, NT), (unsigned)N), dim3(NT), 0, cn_stream(stream), F0, F1, lin, g, (int)C,
                     H * W, dF0);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// ---- LPIPS -------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t cnerf_lpips_packed_floats(void) { return lp_packed().total; }

extern "C" int cnerf_lpips_pack(const cnerf_ptrs* tensors, float* packed, void* stream) {
  if (!tensors || !packed) return CNERF_E_ARG;
  for (int i = 0; i < 2 * LP_LAYERS + LP_TAPS + 2; ++i)
    if (!tensors->p[i]) return CNERF_E_ARG;
  const LpPacked k = lp_packed();
  hipStream_t st = cn_stream(stream);
  if (hipMemsetAsync(packed, 0, (size_t)k.total * sizeof(float), st) != hipSuccess) return (int)hipGetLastError();
  for (int l = 0; l < LP_LAYERS; ++l) {
    int rc = cnerf_conv3x3_pack(tensors->p[2 * l], LP_CIN[l], LP_COUT[l], 0, packed + k.fwd[l], stream);
    if (rc) return rc;
    rc = cnerf_conv3x3_pack(tensors->p[2 * l], LP_CIN[l], LP_COUT[l], 1, packed + k.bwd[l], stream);
    if (rc) return rc;
    if (hipMemcpyAsync(packed + k.bias[l], tensors->p[2 * l + 1], LP_COUT[l] * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return (int)hipGetLastError();
  }
  for (int t = 0; t < LP_TAPS; ++t)
    if (hipMemcpyAsync(packed + k.lin[t], tensors->p[2 * LP_LAYERS + t], LP_TAP_C[t] * sizeof(float), hipMemcpyDeviceToDevice, st) !=
        hipSuccess)
      return (int)hipGetLastError();
  for (int i = 0; i < 2; ++i)
    if (hipMemcpyAsync(packed + k.sc + 3 * i, tensors->p[2 * LP_LAYERS + LP_TAPS + i], 3 * sizeof(float), hipMemcpyDeviceToDevice, st) !=
        hipSuccess)
      return (int)hipGetLastError();
  return CNERF_OK;
}

extern "C" int64_t cnerf_lpips_ws_floats(int64_t N, int64_t H, int64_t W, int keep) {
  if (!lp_shape_ok(N, H, W)) return 0;
  return lp_ws(N, H, W, keep ? 1 : 0).total;
}

extern "C" int64_t cnerf_lpips_act_offset(int64_t N, int64_t H, int64_t W, int layer) {
  if (!lp_shape_ok(N, H, W) || layer < 0 || layer >= LP_LAYERS) return -1;
  return lp_ws(N, H, W, 1).act[layer];
}

extern "C" int cnerf_lpips_fwd(const float* X, const float* Y, const float* packed, int64_t N, int64_t H, int64_t W, int keep, float* value,
                               float* per_tap, float* workspace, void* stream) {
  if (!X || !Y || !packed || !value || !workspace || ((uintptr_t)workspace & 15) != 0 || !lp_shape_ok(N, H, W)) return CNERF_E_ARG;
  const LpPacked k = lp_packed();
  const LpWs s = lp_ws(N, H, W, keep ? 1 : 0);
  hipStream_t st = cn_stream(stream);
  const int64_t HW = H * W;
  if (keep) {
    hipLaunchKernelGGL(lp_scale_k, dim3((unsigned)cn_div_up(2 * N * 3 * HW, NT)), dim3(NT), 0, st, X, Y, packed + k.sc, N, HW,
                       workspace + s.in0);
    CN_CHECK_LAUNCH();
    return lp_trunk(packed, k, s, workspace, 1, N, value, per_tap, N, st);
  }
  for (int64_t n = 0; n < N; ++n) {   // image by image in the two-buffer workspace
    hipLaunchKernelGGL(lp_scale_k, dim3((unsigned)cn_div_up(2 * 3 * HW, NT)), dim3(NT), 0, st, X + n * 3 * HW, Y + n * 3 * HW, packed + k.sc,
                       (int64_t)1, HW, workspace + s.in0);
    CN_CHECK_LAUNCH();
    const int rc = lp_trunk(packed, k, s, workspace, 0, 1, value + n, per_tap ? per_tap + n : nullptr, N, st);
    if (rc) return rc;
  }
  return CNERF_OK;
}

extern "C" int cnerf_lpips_bwd(const float* packed, const float* g, int64_t N, int64_t H, int64_t W, float* dX, float* workspace,
                               void* stream) {
  if (!packed || !g || !dX || !workspace || ((uintptr_t)workspace & 15) != 0 || !lp_shape_ok(N, H, W)) return CNERF_E_ARG;
  const LpPacked k = lp_packed();
  const LpWs s = lp_ws(N, H, W, 1);
  hipStream_t st = cn_stream(stream);
  float* ws = workspace;
  float* gc = ws + s.g0;   // gradient w.r.t. the current layer's output
  float* gn = ws + s.g1;
  auto head_bwd = [&](int t, float* dst) -> int {
    const int l = LP_TAP_LAYER[t], C = LP_COUT[l];
    const int64_t hw = s.h[l] * s.w[l];
    const float* F = ws + s.act[l];
    hipLaunchKernelGGL(lp_head_bwd_k, dim3((unsigned)cn_div_up(hw, NT), (unsigned)N), dim3(NT), 0, st, F, F + N * C * hw, packed + k.lin[t], g, C, hw,
                       dst);
    CN_CHECK_LAUNCH();
    return CNERF_OK;
  };
  int rc = head_bwd(LP_TAPS - 1, gc);
  if (rc) return rc;
  for (int l = LP_LAYERS - 1; l >= 0; --l) {
    // gc = d / d act[l]  ->  gn = d / d (the input of conv l), gated by act[l] > 0
    rc = launch_conv(gc, ws + s.act[l], packed + k.bwd[l], nullptr, 0, N, LP_COUT[l], LP_CIN[l], s.h[l], s.w[l], gn, ws + s.part, st);
    if (rc) return rc;
    if (lp_pool_before(l)) {
      // the input was pool(act[l - 1]), a tapped layer: its head gradient into gc, then the pool's gradient of gn added in place
      rc = head_bwd(lp_tap_of(l - 1), gc);
      if (rc) return rc;
      rc = launch_pool_bwd(ws + s.act[l - 1], gn, gc, N * LP_COUT[l - 1], s.h[l - 1], s.w[l - 1], gc, st);
      if (rc) return rc;
    } else {
      float* t = gc; gc = gn; gn = t;
    }
  }
  // gc = d / d (scaled input)
  hipLaunchKernelGGL(lp_unscale_k, dim3((unsigned)cn_div_up(N * 3 * H * W, NT)), dim3(NT), 0, st, gc, packed + k.sc, N * 3 * H * W, H * W, dX);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// ---- V's patch LPIPS term inside the folded step (run_nerf._RenderClossFn) ---------------------------------------------------------
extern "C" int cnerf_lpips_pack_patches(const float* rgb_last, const float* rgb_coarse, const float* target, int P, int64_t B, float* pred,
                                        float* gt, void* stream) {
  if (!rgb_last || !target || !pred || !gt || P <= 0 || P > 8 || (int64_t)P * 256 > B) return CNERF_E_ARG;
  const int total = (rgb_coarse ? 2 : 1) * P * 768;
  hipLaunchKernelGGL(lp_pack_patches_k, dim3((unsigned)cn_div_up(total, NT)), dim3(NT), 0, cn_stream(stream), rgb_last, rgb_coarse, target,
                     P, total, pred, gt);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_lpips_seeds(const float* g_loss, float lpips_w, int n, float* seeds, void* stream) {
  if (!seeds || n <= 0 || n > 16) return CNERF_E_ARG;
  hipLaunchKernelGGL(lp_seeds_k, dim3(1), dim3(64), 0, cn_stream(stream), g_loss, lpips_w, n, seeds);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
