// The depth-map images of the test-set pass (V:2061-2063: lky_visualize_depth -> save_img_u8 of alky/vis_utils.py:59-150) for a
// batch of frames, and the metric inputs of the same pass (cnerf_eval_prep, below).
//
// Per frame, with x = 1 / disp (NaN where acc == 0) and the weights acc:
//   bounds   lo_auto / hi_auto = np.interp(p / 100 * total, cumsum(acc sorted by x), x sorted) at p = 0.5 / 99.5.  np.interp at an
//            abscissa T needs two neighbours of the sorted order only: q, the first element whose inclusive running sum exceeds T,
//            and p, the element just in front of it (a zero-weight one where the running sum stalls).  Both are found by a radix
//            select, no sort: the elements are ordered by the key (order-preserving uint32 image of x, NaN above +inf) * 2^ib + pixel
//            index (what a stable sort gives), and one launch per 4-bit digit, from the top, narrows both percentiles at once:
//              select_k   every thread keeps the weight of its matching elements per digit value in 2 x 16 fp64 registers, a wave
//                         sums them by shuffles, the waves of a workgroup in index order, and the workgroup writes its 32 partials
//                         at a fixed index.  The NEXT launch starts by summing the workgroups' partials in index order (every
//                         workgroup does, redundantly and identically) and picking the digit: no launch in between, no float
//                         atomics, nothing read back.  The weight in front of the chosen digit is carried down, so after the last
//                         digit the state is (key of q, the running sum in front of q, the weight of q).
//              pred_k     resolves the last digit, then takes the largest key below q's (integer maxima, per workgroup).
//              colour_k   resolves p, interpolates in fp64, writes `bounds`, and colours the frame (steps 3-7) in fp32 with every
//                         operation rounded on its own (as numpy rounds them; the reference runs them in float64).
//            All N frames ride in the grid's y dimension of the same launches.  Identical bits call after call.
#include "common.hpp"
#include "turbo_lut.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                   // threads per workgroup
constexpr int MAX_WG = 128;               // workgroups per frame (grid-stride beyond)
constexpr int DIG = 4, NB = 1 << DIG;     // digit width of the select
constexpr int MAX_PASS = 15;              // (32 + 28) / 4
constexpr float EPS32 = 1.1920928955078125e-07f;

struct SelState {                         // one percentile of one frame after a resolved digit
  unsigned long long prefix;              // the digits chosen so far (after the last: the key of q)
  double E, T, w;                         // weight in front of the prefix, the abscissa, the weight of the chosen digit
  int noq, pad;                           // no element's running sum exceeds T (total == 0): np.interp clamps to the last element
};

struct DvShape {
  int64_t HW;
  int ib, passes, G;
};

__device__ __forceinline__ uint32_t value_key(float x) {
  if (x != x) return 0xFFFFFFFFu;         // every NaN last, as np.argsort
  x = x + 0.0f;                           // -0 and +0 are one value
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_value(uint32_t k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// Sums the partials of digit pass `k` over the frame's workgroups in index order and picks both percentiles' digit:
// st[t] = the state after pass k.  Called by every thread of the workgroup; the caller synchronises afterwards.
__device__ void resolve_pass(int k, const double* __restrict__ part, const SelState* __restrict__ prev, int64_t frame, int G,
                             double* sums, SelState* st) {
  if (threadIdx.x < 2 * NB) {
    double s = 0.0;
    const double* p = part + frame * G * 2 * NB + threadIdx.x;
    for (int g = 0; g < G; ++g) s += p[(int64_t)g * 2 * NB];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int t = threadIdx.x;
    SelState s;
    if (k == 0) {
      double total = 0.0;
      for (int b = 0; b < NB; ++b) total += sums[t * NB + b];
      s.prefix = 0; s.E = 0.0; s.w = 0.0; s.noq = 0; s.pad = 0;
      s.T = (t == 0 ? 0.5 : 99.5) * (total / 100.0);
    } else {
      s = prev[frame * 2 + t];
    }
    if (!s.noq) {
      double c = s.E, e_nz = s.E;
      int sel = -1, last_nz = -1;
      for (int b = 0; b < NB; ++b) {
        const double v = sums[t * NB + b];
        if (c + v > s.T) { sel = b; break; }
        if (v > 0.0) { last_nz = b; e_nz = c; }
        c += v;
      }
      // below the first pass the digit's weight was already found to reach past T; if the regrouped sum misses by a rounding, the
      // last weighted digit is the one
      if (sel < 0 && k > 0 && last_nz >= 0) { sel = last_nz; c = e_nz; }
      if (sel < 0) {
        s.noq = 1;
      } else {
        s.prefix = (s.prefix << DIG) | (unsigned long long)sel;
        s.E = c;
        s.w = sums[t * NB + sel];
      }
    }
    st[t] = s;
  }
}

__device__ __forceinline__ unsigned long long elem_key(const float* __restrict__ disp, int64_t base, int64_t i, int ib) {
  const float x = 1.0f / disp[base + i];
  return ((unsigned long long)value_key(x) << ib) | (unsigned long long)i;
}

// digit pass k: resolves pass k - 1 (state slot k - 1), then the per-digit weights of the elements under each percentile's prefix
__global__ __launch_bounds__(NT) void select_k(const float* __restrict__ disp, const float* __restrict__ acc, DvShape sh, int k,
                                               const double* __restrict__ part_in, double* __restrict__ part_out,
                                               SelState* __restrict__ state) {
  __shared__ double sums[2 * NB];
  __shared__ SelState st[2];
  __shared__ double red[NT / 64][2 * NB];
  const int64_t frame = blockIdx.y, base = frame * sh.HW;
  const int g = blockIdx.x, nfr = gridDim.y;
  if (k > 0) {
    resolve_pass(k - 1, part_in, state + (int64_t)(k > 1 ? k - 2 : 0) * nfr * 2, frame, sh.G, sums, st);
    __syncthreads();
    if (g == 0 && threadIdx.x < 2) state[((int64_t)(k - 1) * nfr + frame) * 2 + threadIdx.x] = st[threadIdx.x];
  } else {
    if (threadIdx.x < 2) { st[threadIdx.x].prefix = 0; st[threadIdx.x].noq = 0; }
    __syncthreads();
  }
  const int shift = DIG * (sh.passes - 1 - k);
  const unsigned long long pre0 = st[0].prefix, pre1 = st[1].prefix;
  const bool on0 = !st[0].noq, on1 = !st[1].noq;
  double a0[NB], a1[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) { a0[b] = 0.0; a1[b] = 0.0; }
  for (int64_t i = (int64_t)g * NT + threadIdx.x; i < sh.HW; i += (int64_t)sh.G * NT) {
    const unsigned long long ck = elem_key(disp, base, i, sh.ib);
    const double w = (double)acc[base + i];
    const unsigned long long up = ck >> (shift + DIG);
    const int d = (int)((ck >> shift) & (NB - 1));
    const bool m0 = on0 && up == pre0, m1 = on1 && up == pre1;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      a0[b] += (m0 && d == b) ? w : 0.0;
      a1[b] += (m1 && d == b) ? w : 0.0;
    }
  }
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double s0 = wave_sum(a0[b]), s1 = wave_sum(a1[b]);
    if (lane == 0) { red[wv][b] = s0; red[wv][NB + b] = s1; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * NB) {
    double s = 0.0;
    for (int i = 0; i < NT / 64; ++i) s += red[i][threadIdx.x];
    part_out[(frame * sh.G + g) * 2 * NB + threadIdx.x] = s;
  }
}

// resolves the last digit (state slot passes - 1 = q), then the largest key below q's, + 1 (0 = none), per workgroup
__global__ __launch_bounds__(NT) void pred_k(const float* __restrict__ disp, DvShape sh, const double* __restrict__ part_in,
                                             SelState* __restrict__ state, unsigned long long* __restrict__ pred) {
  __shared__ double sums[2 * NB];
  __shared__ SelState st[2];
  __shared__ unsigned long long red[NT / 64][2];
  const int64_t frame = blockIdx.y, base = frame * sh.HW;
  const int g = blockIdx.x, nfr = gridDim.y, k = sh.passes;
  resolve_pass(k - 1, part_in, state + (int64_t)(k > 1 ? k - 2 : 0) * nfr * 2, frame, sh.G, sums, st);
  __syncthreads();
  if (g == 0 && threadIdx.x < 2) state[((int64_t)(k - 1) * nfr + frame) * 2 + threadIdx.x] = st[threadIdx.x];
  const unsigned long long q0 = st[0].noq ? ~0ull : st[0].prefix, q1 = st[1].noq ? ~0ull : st[1].prefix;
  unsigned long long m0 = 0, m1 = 0;
  for (int64_t i = (int64_t)g * NT + threadIdx.x; i < sh.HW; i += (int64_t)sh.G * NT) {
    const unsigned long long ck = elem_key(disp, base, i, sh.ib);
    if (ck < q0 && ck + 1 > m0) m0 = ck + 1;
    if (ck < q1 && ck + 1 > m1) m1 = ck + 1;
  }
  m0 = wave_max(m0); m1 = wave_max(m1);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[wv][0] = m0; red[wv][1] = m1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long m = 0;
    for (int i = 0; i < NT / 64; ++i) m = red[i][threadIdx.x] > m ? red[i][threadIdx.x] : m;
    pred[(frame * sh.G + g) * 2 + threadIdx.x] = m;
  }
}

// np.interp between the neighbours p and q of the abscissa T (fp64, each operation rounded on its own)
__device__ double interp_bound(const SelState& s, unsigned long long pm, int ib) {
  const double xq = (double)key_value((uint32_t)(s.prefix >> ib));
  if (pm == 0) return xq;                                   // q is the first element: clamped
  const double xp = (double)key_value((uint32_t)((pm - 1) >> ib));
  if (s.noq) return xp;                                     // nothing beyond T: the last element
  if (s.T == s.E) return xp;
  const double slope = (xq - xp) / s.w;
  double r = slope * (s.T - s.E) + xp;
  if (r != r) {
    r = slope * (s.T - (s.E + s.w)) + xq;
    if (r != r && xp == xq) r = xp;
  }
  return r;
}

__device__ __forceinline__ float clip01_nan0(float v) {     // np.clip(np.nan_to_num(v), 0, 1) / nan_to_num(clip(v, 0, 1))
  return v != v ? 0.f : fminf(fmaxf(v, 0.f), 1.f);
}

__global__ __launch_bounds__(NT) void colour_k(const float* __restrict__ disp, const float* __restrict__ acc, DvShape sh, float lo_arg,
                                               float hi_arg, int use_lo, int use_hi, const SelState* __restrict__ state,
                                               const unsigned long long* __restrict__ pred, float* __restrict__ img_f32,
                                               uint8_t* __restrict__ img_u8, float* __restrict__ bounds) {
  __shared__ float bnd[2];
  const int64_t frame = blockIdx.y, base = frame * sh.HW;
  const int g = blockIdx.x, nfr = gridDim.y;
  if (threadIdx.x < 2) {
    unsigned long long m = 0;
    const unsigned long long* p = pred + frame * sh.G * 2 + threadIdx.x;
    for (int i = 0; i < sh.G; ++i) m = p[2 * i] > m ? p[2 * i] : m;
    const SelState s = state[((int64_t)(sh.passes - 1) * nfr + frame) * 2 + threadIdx.x];
    bnd[threadIdx.x] = (float)interp_bound(s, m, sh.ib);
    if (g == 0 && bounds) bounds[frame * 2 + threadIdx.x] = bnd[threadIdx.x];
  }
  __syncthreads();
  if (!img_f32 && !img_u8) return;
  // `lo or (lo_auto - eps)`: a passed 0 counts as not passed
  const float lo = (use_lo && lo_arg != 0.f) ? lo_arg : bnd[0] - EPS32;
  const float hi = (use_hi && hi_arg != 0.f) ? hi_arg : bnd[1] + EPS32;
  const float c_lo = -logf(lo + EPS32), c_hi = -logf(hi + EPS32);
  const float c_min = (c_lo != c_lo || c_hi != c_hi) ? __uint_as_float(0x7FC00000u) : fminf(c_lo, c_hi);
  const float den = fabsf(c_hi - c_lo);
  for (int64_t i = (int64_t)g * NT + threadIdx.x; i < sh.HW; i += (int64_t)sh.G * NT) {
    const float x = 1.0f / disp[base + i], a = acc[base + i];
    const float c = -logf(x + EPS32);
    const float t = clip01_nan0((c - c_min) / den);
    int idx = (int)(t * 256.f);
    idx = idx > 255 ? 255 : idx;
    const float bg = 1.f - a;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = CN_TURBO_LUT[idx][ch] * a + bg;
      if (img_f32) img_f32[(base + i) * 3 + ch] = v;
      if (img_u8) img_u8[(base + i) * 3 + ch] = (uint8_t)(clip01_nan0(v) * 255.f);
    }
  }
}

bool dv_shape(int64_t N, int64_t H, int64_t W, DvShape* s) {
  if (N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > (1 << 20) || W > (1 << 20) || H * W > ((int64_t)1 << 28)) return false;
  s->HW = H * W;
  s->ib = 0;
  while (((int64_t)1 << s->ib) < s->HW) ++s->ib;
  s->passes = (32 + s->ib + DIG - 1) / DIG;
  const int64_t g = cn_div_up(s->HW, NT);
  s->G = (int)(g < MAX_WG ? g : MAX_WG);
  return true;
}

// workspace layout (bytes): two partial buffers [N][G][32] fp64 | pred [N][G][2] u64 | state [MAX_PASS][N][2]
int64_t dv_part_doubles(int64_t N, const DvShape& s) { return N * s.G * 2 * NB; }

// ---- cnerf_eval_prep: [N, H, W, 3] frames -> the SSIM / LPIPS inputs [N, 3, H, W] and the fp64 PSNR partials, one pass --------------
constexpr int EP_MAX_WG = 64;             // workgroups per image

// per-workgroup partials part[(n * G + g) * 3 + {0, 1, 2}] = sum (x - y)^2 over the 3 channels, sum mask * mean_c (x - y)^2, sum mask
__global__ __launch_bounds__(NT) void eval_prep_k(const float* __restrict__ pred, const float* __restrict__ gt,
                                                  const float* __restrict__ mask, int64_t HW, int G, float* __restrict__ ssim_p,
                                                  float* __restrict__ ssim_g, float* __restrict__ lp_p, float* __restrict__ lp_g,
                                                  double* __restrict__ part) {
  __shared__ double red[NT / 64][3];
  const int64_t n = blockIdx.y, base = n * HW;
  const int g = blockIdx.x;
  double se = 0.0, sm = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)g * NT + threadIdx.x; i < HW; i += (int64_t)G * NT) {
    const float m = mask ? mask[base + i] : 1.f;
    const float bg = 1.f - m;
    double e = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float x = pred[(base + i) * 3 + ch], y = gt[(base + i) * 3 + ch];
      const int64_t o = (n * 3 + ch) * HW + i;
      if (ssim_p) ssim_p[o] = mask ? m * x : x;
      if (ssim_g) ssim_g[o] = mask ? m * y : y;
      const float lx = (x - 0.5f) * 2.f, ly = (y - 0.5f) * 2.f;
      if (lp_p) lp_p[o] = mask ? lx * m + bg : lx;
      if (lp_g) lp_g[o] = mask ? ly * m + bg : ly;
      const double d = (double)x - (double)y;
      e += d * d;
    }
    se += e;
    sm += (double)m * (e / 3.0);
    cnt += (double)m;
  }
  if (!part) return;
  se = wave_sum(se); sm = wave_sum(sm); cnt = wave_sum(cnt);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[wv][0] = se; red[wv][1] = sm; red[wv][2] = cnt; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int i = 0; i < NT / 64; ++i) s += red[i][threadIdx.x];
    part[(n * G + g) * 3 + threadIdx.x] = s;
  }
}

// one wave: sums[0] = the squared error of all images, sums[1 + 2 n] / sums[2 + 2 n] = image n's masked error / mask sums; the
// workgroups of an image in index order, the images in index order
__global__ __launch_bounds__(64) void eval_prep_fin_k(const double* __restrict__ part, int64_t N, int G, double* __restrict__ sums) {
  double tot = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (int g = threadIdx.x; g < G; g += 64) {
      a += part[(n * G + g) * 3 + 0]; b += part[(n * G + g) * 3 + 1]; c += part[(n * G + g) * 3 + 2];
    }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    tot += a;
    if (threadIdx.x == 0) { sums[1 + 2 * n] = b; sums[2 + 2 * n] = c; }
  }
  if (threadIdx.x == 0) sums[0] = tot;
}

int ep_wgs(int64_t HW) {
  const int64_t g = cn_div_up(HW, NT);
  return (int)(g < EP_MAX_WG ? g : EP_MAX_WG);
}

}  // namespace

extern "C" int64_t cnerf_depthvis_ws_bytes(int64_t N, int64_t H, int64_t W) {
  DvShape s;
  if (!dv_shape(N, H, W, &s)) return 0;
  return (int64_t)sizeof(double) * 2 * dv_part_doubles(N, s) + (int64_t)sizeof(unsigned long long) * N * s.G * 2 +
         (int64_t)sizeof(SelState) * MAX_PASS * N * 2;
}

extern "C" int cnerf_depthvis(const float* disp, const float* acc, int64_t N, int64_t H, int64_t W, float lo, float hi, int use_lo,
                              int use_hi, float* img_f32, uint8_t* img_u8, float* bounds, void* workspace, void* stream) {
  DvShape s;
  if (!disp || !acc || !workspace || ((uintptr_t)workspace & 7) != 0 || (!img_f32 && !img_u8 && !bounds) || !dv_shape(N, H, W, &s))
    return CNERF_E_ARG;
  double* part[2] = {reinterpret_cast<double*>(workspace), reinterpret_cast<double*>(workspace) + dv_part_doubles(N, s)};
  unsigned long long* pred = reinterpret_cast<unsigned long long*>(part[1] + dv_part_doubles(N, s));
  SelState* state = reinterpret_cast<SelState*>(pred + N * s.G * 2);
  const dim3 grid((unsigned)s.G, (unsigned)N);
  for (int k = 0; k < s.passes; ++k) {
    hipLaunchKernelGGL(select_k, grid, dim3(NT), 0, cn_stream(stream), disp, acc, s, k, (const double*)part[(k + 1) & 1], part[k & 1],
                       state);
    CN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pred_k, grid, dim3(NT), 0, cn_stream(stream), disp, s, (const double*)part[(s.passes - 1) & 1], state, pred);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(colour_k, grid, dim3(NT), 0, cn_stream(stream), disp, acc, s, lo, hi, use_lo, use_hi, (const SelState*)state,
                     (const unsigned long long*)pred, img_f32, img_u8, bounds);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int64_t cnerf_eval_prep_ws_bytes(int64_t N, int64_t H, int64_t W) {
  if (N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > (1 << 20) || W > (1 << 20) || H * W > ((int64_t)1 << 28)) return 0;
  return (int64_t)sizeof(double) * N * ep_wgs(H * W) * 3;
}

extern "C" int cnerf_eval_prep(const float* pred, const float* gt, const float* mask, int64_t N, int64_t H, int64_t W, float* ssim_pred,
                               float* ssim_gt, float* lpips_pred, float* lpips_gt, double* sums, void* workspace, void* stream) {
  if (!pred || !gt || N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > (1 << 20) || W > (1 << 20) || H * W > ((int64_t)1 << 28) ||
      (!ssim_pred && !ssim_gt && !lpips_pred && !lpips_gt && !sums) || (sums && (!workspace || ((uintptr_t)workspace & 7) != 0)))
    return CNERF_E_ARG;
  const int G = ep_wgs(H * W);
  double* part = sums ? reinterpret_cast<double*>(workspace) : nullptr;
  hipLaunchKernelGGL(eval_prep_k, dim3((unsigned)G, (unsigned)N), dim3(NT), 0, cn_stream(stream), pred, gt, mask, H * W, G, ssim_pred,
                     ssim_gt, lpips_pred, lpips_gt, part);
  CN_CHECK_LAUNCH();
  if (sums) {
    hipLaunchKernelGGL(eval_prep_fin_k, dim3(1), dim3(64), 0, cn_stream(stream), (const double*)part, N, G, sums);
    CN_CHECK_LAUNCH();
  }
  return CNERF_OK;
}
