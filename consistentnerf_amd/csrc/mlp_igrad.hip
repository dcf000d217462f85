// Input gradients of the fused encoding+MLP and of the ray batch (autograd of run_network R:37-52 w.r.t. `inputs` / `viewdirs`,
// of render R:97-125 + render_rays R:384 + raw2outputs R:283 w.r.t. rays_o / rays_d).  Four launches, all behind the existing
// backward (nothing of it changes):
//   1. mlp_igrad_k: runs after the dgrad of the same level on the same gradient workspace G[Mp][g_rows] and stash.  One wave64
//      per 32 points computes d gamma(x)^T[in_chp x 32] = W_0^T . dZ_0^T (+ W_{skip+1}[:, :in_ch]^T . dZ_{skip+1}^T) and
//      d gamma(d)^T[dir_chp x 32] = W_v[:, W:]^T . dZ_v^T with v_mfma_f32_32x32x2_f32 (exact fp32), accumulators in registers, and
//      contracts them with the Jacobian of the encoding, whose sin / cos values are the stashed gamma(x) / gamma(d) — the bits the
//      forward used -> d_pts[M,3], d_dirs_pt[M,3].
//   2. rays_igrad_k: one wave per ray sums the per-point gradients into d_o, d_d (x = o + d z) and d_viewdirs.
//   3. composite_norm_k: one wave per ray, the gradient of raw2outputs w.r.t. rays_d through dists * |rays_d| (R:283), from the
//      d_raw that cnerf_composite_bwd already produced.
//   4. pack_rays_bwd_k: one thread per ray, the backward of the non-NDC cnerf_pack_rays (viewdirs = d / |d|).
// The camera chain on the folded training step runs the first three for BOTH levels of one ray batch in one grid each
// (mlp_igrad_pair_k, rays_igrad_pair_k, composite_norm_pair_k): the per-level arithmetic is the single kernels' (the same __device__
// bodies), the two levels' per-ray results are added in fp32 after each was rounded, and every column of the [B, ray_stride] row
// gradient is written (no fill launch in front).
// No atomics anywhere: every sum has a fixed order, results are identical from run to run.
#include "mlp_common.hpp"

namespace {

struct IgradArgs {
  NetGeom g;
  const float* packed;
  const float* stash;
  const float* G;
  float* d_pts;      // [M,3]
  float* d_dirs;     // [M,3] or nullptr
  int64_t M;
};

#define CN_CONST __attribute__((address_space(4)))

__device__ __forceinline__ float buf_load_f(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

// acc[t] += sum_n P(c = 32t + i, n) * dZ[n][m] over the 8*KG columns n of the gradient block at byte column `gcol`.
// A operand: a FORWARD panel P[c/8][NP][8] of the packed buffer, read in place as W^T: MFMA (kg, j) contracts n = 8kg + j
// (half-wave 0) and 8kg + 4 + j (half-wave 1), lane (i, hh) supplies W[n][32t + i] — one dword per MFMA, 8 lanes per 32-byte
// sector.  B operand: this lane's 16 bytes of the tile-major gradient block (columns 8kg + 4hh .. +3 of point m) feed the four
// MFMAs of a group — the pairing of the dgrad that wrote them.  Group kg+1 is loaded while group kg runs.
template <int NCT>
__device__ __forceinline__ void igrad_gemm(f32x16 (&acc)[NCT], rsrc_t wrs, int poff, int NP, rsrc_t grs, int gvo, int gcol,
                                           int KG, int lane) {
  const int i = lane & 31, hh = lane >> 5;
  const int avo = (((i >> 3) * NP + 4 * hh) * 8 + (i & 7)) * 4;
  auto lda = [&](float (&A)[4][NCT], int kg) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < NCT; ++t) A[j][t] = buf_load_f(wrs, avo, (poff + (4 * t * NP + 8 * kg + j) * 8) * 4);
  };
  auto ldb = [&](int kg) __attribute__((always_inline)) { return buf_load(grs, gvo, gcol + kg * 1024); };
  auto mma = [&](const float (&A)[4][NCT], const f32x4& b) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < NCT; ++t) acc[t] = mfma(A[j][t], b[j], acc[t]);
  };
  float A0[4][NCT], A1[4][NCT];
  f32x4 b0, b1;
  lda(A0, 0);
  b0 = ldb(0);
  for (int kg = 0; kg < KG; kg += 2) {   // KG is even (W/8, W/16 of W in {64, 128, 256})
    lda(A1, kg + 1);
    b1 = ldb(kg + 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(A0, b0);
    const int kn = kg + 2 < KG ? kg + 2 : KG - 1;   // (re-read past the end: branch-free)
    lda(A0, kn);
    b0 = ldb(kn);
    __builtin_amdgcn_sched_barrier(0);
    mma(A1, b1);
  }
}

// Column c of an encoding (H:24-45): [v, sin(2^0 v), cos(2^0 v), ..]: 3 + 6k + j is the sin column, 3 + 6k + 3 + j the cos column.
struct EncCol {
  int j;          // coordinate the column depends on
  int partner;    // the column holding d(column)/d(argument) up to sign: cos for a sin column, sin for a cos column; -1: identity
  float coef;     // 2^k for a sin column, -2^k for a cos column, 1 for an identity column
};
__host__ __device__ constexpr EncCol enc_col(int c) {
  if (c < 3) return EncCol{c, -1, 1.f};
  const int t = c - 3, k = t / 6, u = t % 6;
  const float s = (float)(1 << k);
  return u < 3 ? EncCol{u, c + 3, s} : EncCol{u - 3, c - 3, -s};
}

// d[j] = sum over this point's encoding columns of d gamma[c] * d gamma_c / d v_j, from the C-layout accumulators (lane (m, hh),
// register r of tile t <-> column 32t + 8(r>>2) + 4hh + (r&3)) and the stashed encoding block at column `scol` of this tile
// row.  Each lane sums its own columns in register order, then the two half-waves are added: a fixed order.
template <int NCT>
__device__ __forceinline__ void enc_jacobian(const f32x16 (&acc)[NCT], rsrc_t srs, int scol, int ch, int lane, bool valid,
                                             float (&d)[3]) {
  const int m = lane & 31, hh = lane >> 5;
  d[0] = d[1] = d[2] = 0.f;
#pragma unroll
  for (int t = 0; t < NCT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c0 = 32 * t + 8 * (r >> 2) + (r & 3);
      const EncCol e0 = enc_col(c0), e1 = enc_col(c0 + 4);
      const int c = hh ? c0 + 4 : c0;
      const int j = hh ? e1.j : e0.j;
      const int pc = hh ? e1.partner : e0.partner;
      const float coef = hh ? e1.coef : e0.coef;
      const bool on = c < ch;                       // (padding columns carry nothing)
      const int voff = (valid && on && pc >= 0) ? m * 32 + (pc >> 3) * 1024 + (pc & 7) * 4 : TM_OOB;
      const float ld = buf_load_f(srs, voff, tm_col(scol));
      const float gam = pc >= 0 ? ld : 1.f;         // (identity columns: the Jacobian is 1)
      const float term = on ? coef * gam * acc[t][r] : 0.f;
      d[0] += j == 0 ? term : 0.f;
      d[1] += j == 1 ? term : 0.f;
      d[2] += j == 2 ? term : 0.f;
    }
#pragma unroll
  for (int j = 0; j < 3; ++j) d[j] = half_sum(d[j]);
}

template <int NCT>
__device__ __forceinline__ void igrad_x(const CN_CONST IgradArgs& a, rsrc_t wrs, rsrc_t grs, rsrc_t srs, int gvo, int lane,
                                        bool valid, float (&d)[3]) {
  const CN_CONST NetGeom& g = a.g;
  f32x16 acc[NCT];
  zero_acc<NCT>(acc);
  igrad_gemm<NCT>(acc, wrs, (int)g.f_l0, g.W, grs, gvo, tm_col(g.g_z[0]), g.W / 8, lane);
  if (g.skip >= 0) igrad_gemm<NCT>(acc, wrs, (int)g.f_skip, g.W, grs, gvo, tm_col(g.g_z[g.skip + 1]), g.W / 8, lane);
  enc_jacobian<NCT>(acc, srs, g.s_enc, g.in_ch, lane, valid, d);
}

// One wave64: the 32 points of tile `tile` of the level `a` (read in place from the kernarg segment).
__device__ __forceinline__ void igrad_tile(const CN_CONST IgradArgs& a, unsigned tile) {
  const CN_CONST NetGeom& g = a.g;
  const int lane = threadIdx.x, m = lane & 31, hh = lane >> 5;
  const int64_t p0 = (int64_t)tile * 32;
  const int64_t p = p0 + m;
  const bool valid = p < a.M;
  // this tile's rows of the gradient workspace and of the stash; lanes of padding points address out of range (zeros)
  const rsrc_t wrs = make_rsrc(a.packed, (unsigned)(g.total * 4));
  const rsrc_t grs = make_rsrc(a.G + p0 * g.g_rows, (unsigned)(32 * g.g_rows * 4));
  const rsrc_t srs = make_rsrc(a.stash + p0 * g.s_rows, (unsigned)(32 * g.s_rows * 4));
  const int gvo = valid ? m * 32 + hh * 16 : TM_OOB;
  float d[3];
  if (g.in_chp == 64) igrad_x<2>(a, wrs, grs, srs, gvo, lane, valid, d);
  else igrad_x<1>(a, wrs, grs, srs, gvo, lane, valid, d);
  if (valid && hh == 0) {   // padding points of a ragged last tile store nothing
    a.d_pts[p * 3 + 0] = d[0]; a.d_pts[p * 3 + 1] = d[1]; a.d_pts[p * 3 + 2] = d[2];
  }
  if (g.viewdirs && a.d_dirs != nullptr) {
    f32x16 acc[1];
    zero_acc<1>(acc);
    igrad_gemm<1>(acc, wrs, (int)g.f_viewsd, g.Wh, grs, gvo, tm_col(g.g_hv), g.Wh / 8, lane);
    enc_jacobian<1>(acc, srs, g.s_denc, g.dir_ch, lane, valid, d);
    if (valid && hh == 0) {
      a.d_dirs[p * 3 + 0] = d[0]; a.d_dirs[p * 3 + 1] = d[1]; a.d_dirs[p * 3 + 2] = d[2];
    }
  }
}

__global__ __launch_bounds__(64) void mlp_igrad_k(IgradArgs args_by_value) {
  (void)args_by_value;   // read in place from the kernarg segment (scalar loads next to their use)
  igrad_tile(*(const CN_CONST IgradArgs*)__builtin_amdgcn_kernarg_segment_ptr(), blockIdx.x);
}

// Two levels in one grid: workgroups [0, nb0) walk the tiles of lv[0], the rest those of lv[1] (the level is picked by blockIdx.x:
// uniform across the wave, each level with its own geometry, sample count and ragged last tile).
struct IgradPairArgs {
  IgradArgs lv[2];
  unsigned nb0;
};

__global__ __launch_bounds__(64) void mlp_igrad_pair_k(IgradPairArgs args_by_value) {
  (void)args_by_value;
  const CN_CONST IgradPairArgs& args = *(const CN_CONST IgradPairArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const unsigned nb0 = args.nb0;
  const bool second = blockIdx.x >= nb0;
  igrad_tile(args.lv[second ? 1 : 0], blockIdx.x - (second ? nb0 : 0u));
}

// One ray of one level: lane l sums samples l, l + 64, .. in order, then the xor butterfly (a fixed order).  pts: so = sum_s d_pts,
// sd = sum_s z d_pts; dirs: sv = sum_s d_dirs.
__device__ __forceinline__ void rays_level_sums(const float* __restrict__ d_pts, const float* __restrict__ d_dirs,
                                                const float* __restrict__ z, int64_t b, int S, int lane, bool pts, bool dirs,
                                                float (&so)[3], float (&sd)[3], float (&sv)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) so[j] = sd[j] = sv[j] = 0.f;
  for (int s = lane; s < S; s += 64) {
    const int64_t q = b * S + s;
    if (pts) {
      const float zz = z[q];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float gx = d_pts[q * 3 + j];
        so[j] += gx;
        sd[j] += zz * gx;
      }
    }
    if (dirs)
#pragma unroll
      for (int j = 0; j < 3; ++j) sv[j] += d_dirs[q * 3 + j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    so[j] = wave_sum(so[j]); sd[j] = wave_sum(sd[j]); sv[j] = wave_sum(sv[j]);
  }
}

// one wave per ray
__global__ __launch_bounds__(256) void rays_igrad_k(const float* __restrict__ d_pts, const float* __restrict__ d_dirs,
                                                    const float* __restrict__ z, int64_t B, int S, float* __restrict__ d_o,
                                                    float* __restrict__ d_d, float* __restrict__ d_v, int os) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  float so[3], sd[3], sv[3];
  rays_level_sums(d_pts, d_dirs, z, b, S, lane, d_o != nullptr, d_v != nullptr, so, sd, sv);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (d_o != nullptr) { d_o[b * os + j] = so[j]; d_d[b * os + j] = sd[j]; }
      if (d_v != nullptr) d_v[b * os + j] = sv[j];
    }
  }
}

// One wave per ray, both levels of one ray batch: each level's sums as above (rounded to fp32), then level 0 + level 1, into EVERY
// column of the [B, rs] row gradient: origins 0:3, directions 3:6, zeros up to the last three columns, which hold the per-ray
// view-direction sum when the levels carry one (d_dirs0 / d_dirs1: both or neither) and zeros otherwise.
__global__ __launch_bounds__(256) void rays_igrad_pair_k(const float* __restrict__ d_pts0, const float* __restrict__ d_dirs0,
                                                         const float* __restrict__ z0, int S0, const float* __restrict__ d_pts1,
                                                         const float* __restrict__ d_dirs1, const float* __restrict__ z1, int S1,
                                                         int64_t B, float* __restrict__ out, int rs) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const bool dirs = d_dirs0 != nullptr;
  float so0[3], sd0[3], sv0[3], so1[3], sd1[3], sv1[3];
  rays_level_sums(d_pts0, d_dirs0, z0, b, S0, lane, true, dirs, so0, sd0, sv0);
  rays_level_sums(d_pts1, d_dirs1, z1, b, S1, lane, true, dirs, so1, sd1, sv1);
  if (lane == 0) {
    float* r = out + b * rs;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      r[j] = so0[j] + so1[j];
      r[3 + j] = sd0[j] + sd1[j];
    }
    for (int c = 6; c < rs; ++c) r[c] = 0.f;
    if (dirs)
#pragma unroll
      for (int j = 0; j < 3; ++j) r[rs - 3 + j] = sv0[j] + sv1[j];
  }
}

// One ray of one level: alpha_s = 1 - exp(-relu(sigma_s + noise_s) dist_s n), n = |rays_d| (R:283, R:296-298), so
// dL/dn = (1/n) sum_s d_raw[s, sigma] * relu(sigma_s + noise_s) and d rays_d = (rays_d / n) dL/dn.  (A 1e10 tail sample whose
// sigma is positive has alpha = 1 exactly and d_raw[s, sigma] = 0 already.)  -> sum_s d_raw[s, sigma] * relu(..) in every lane.
__device__ __forceinline__ float norm_level_sum(const float* __restrict__ d_raw, const float* __restrict__ raw, int ch,
                                                const float* __restrict__ noise, int64_t b, int S, int lane) {
  float acc = 0.f;
  for (int s = lane; s < S; s += 64) {
    const int64_t q = b * S + s;
    float sg = raw[q * ch + 3];
    if (noise != nullptr) sg = sg + noise[q];
    acc += d_raw[q * ch + 3] * (sg > 0.f ? sg : 0.f);
  }
  return wave_sum(acc);
}

// one wave per ray
__global__ __launch_bounds__(256) void composite_norm_k(const float* __restrict__ d_raw, const float* __restrict__ raw, int ch,
                                                        const float* __restrict__ noise, const float* __restrict__ rays, int rs,
                                                        int64_t B, int S, float* __restrict__ d_d, int os) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const float acc = norm_level_sum(d_raw, raw, ch, noise, b, S, lane);
  if (lane == 0) {
    const float* r = rays + b * rs;
    const float dx = r[3], dy = r[4], dz = r[5];
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    const float gn = acc / n;
    d_d[b * os + 0] = dx / n * gn; d_d[b * os + 1] = dy / n * gn; d_d[b * os + 2] = dz / n * gn;
  }
}

// One wave per ray, both levels of one ray batch (the same rows): each level's term as above, rounded, then level 0 + level 1 into
// columns 3:6 of the [B, rs] row gradient; every other column is written zero.
__global__ __launch_bounds__(256) void composite_norm_pair_k(const float* __restrict__ d_raw0, const float* __restrict__ raw0, int ch0,
                                                             const float* __restrict__ noise0, int S0,
                                                             const float* __restrict__ d_raw1, const float* __restrict__ raw1, int ch1,
                                                             const float* __restrict__ noise1, int S1,
                                                             const float* __restrict__ rays, int rs, int64_t B, float* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const float acc0 = norm_level_sum(d_raw0, raw0, ch0, noise0, b, S0, lane);
  const float acc1 = norm_level_sum(d_raw1, raw1, ch1, noise1, b, S1, lane);
  if (lane == 0) {
    const float* r = rays + b * rs;
    const float dx = r[3], dy = r[4], dz = r[5];
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    const float gn0 = acc0 / n, gn1 = acc1 / n;
    float* o = out + b * rs;
    for (int c = 0; c < rs; ++c)
      if (c < 3 || c >= 6) o[c] = 0.f;
    o[3] = dx / n * gn0 + dx / n * gn1; o[4] = dy / n * gn0 + dy / n * gn1; o[5] = dz / n * gn0 + dz / n * gn1;
  }
}

// one thread per ray: rows [o, d, near, far (, v = d / |d|)] of the non-NDC pack
__global__ void pack_rays_bwd_k(const float* __restrict__ g, int gs, const float* __restrict__ rd, int64_t B, int vd,
                                float* __restrict__ d_o, float* __restrict__ d_d) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* gr = g + b * gs;
  float o[3] = {gr[3], gr[4], gr[5]};
  if (vd) {
    const float dx = rd[b * 3], dy = rd[b * 3 + 1], dz = rd[b * 3 + 2];
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    const float v[3] = {dx / n, dy / n, dz / n};
    const float dot = v[0] * gr[8] + v[1] * gr[9] + v[2] * gr[10];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] += (gr[8 + j] - v[j] * dot) / n;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    d_o[b * 3 + j] = gr[j];
    d_d[b * 3 + j] = o[j];
  }
}

}  // namespace

extern "C" int cnerf_mlp_input_grad(const cnerf_net* net, const float* packed, int64_t B, int S, const float* stash,
                                    const float* workspace, float* d_pts, float* d_dirs_pt, void* stream) {
  IgradArgs a;
  const int rc = cn_make_geom(net, &a.g);
  if (rc) return rc;
  if (!packed || !stash || !workspace || !d_pts || B <= 0 || S <= 0) return CNERF_E_ARG;
  if (d_dirs_pt && !a.g.viewdirs) return CNERF_E_ARG;
  a.packed = packed; a.stash = stash; a.G = workspace; a.d_pts = d_pts; a.d_dirs = d_dirs_pt;
  a.M = B * S;
  hipLaunchKernelGGL(mlp_igrad_k, dim3((unsigned)cn_div_up(a.M, 32)), dim3(64), 0, cn_stream(stream), a);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_rays_input_grad(const float* d_pts, const float* d_dirs_pt, const float* z, int64_t B, int S, float* d_o,
                                     float* d_d, float* d_viewdirs, int out_stride, void* stream) {
  if (B <= 0 || S <= 0 || out_stride < 3) return CNERF_E_ARG;
  const bool pts = d_o != nullptr || d_d != nullptr, dirs = d_viewdirs != nullptr;
  if (!pts && !dirs) return CNERF_E_ARG;
  if (pts && (!d_o || !d_d || !d_pts || !z)) return CNERF_E_ARG;
  if (dirs && !d_dirs_pt) return CNERF_E_ARG;
  hipLaunchKernelGGL(rays_igrad_k, dim3((unsigned)cn_div_up(B, 4)), dim3(256), 0, cn_stream(stream), d_pts, d_dirs_pt, z, B, S,
                     d_o, d_d, d_viewdirs, out_stride);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_composite_norm_grad(const float* d_raw, const float* raw, int raw_ch, const float* noise, const float* rays,
                                         int ray_stride, int64_t B, int S, float* d_d, int out_stride, void* stream) {
  if (!d_raw || !raw || !rays || !d_d || B <= 0 || S <= 0 || raw_ch < 4 || ray_stride < 6 || out_stride < 3) return CNERF_E_ARG;
  hipLaunchKernelGGL(composite_norm_k, dim3((unsigned)cn_div_up(B, 4)), dim3(256), 0, cn_stream(stream), d_raw, raw, raw_ch, noise,
                     rays, ray_stride, B, S, d_d, out_stride);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_pack_rays_bwd(const float* g, const float* rays_d, int64_t B, int use_viewdirs, float* d_o, float* d_d,
                                   void* stream) {
  if (!g || !rays_d || !d_o || !d_d || B <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(pack_rays_bwd_k, dim3((unsigned)cn_div_up(B, 256)), dim3(256), 0, cn_stream(stream), g, use_viewdirs ? 11 : 8,
                     rays_d, B, use_viewdirs ? 1 : 0, d_o, d_d);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// ---- both levels of one ray batch in one grid each (the camera chain on the folded training step) ---------------------------------
extern "C" int cnerf_mlp_input_grad_pair(const cnerf_net* net0, const float* packed0, int64_t B0, int S0, const float* stash0,
                                         const float* workspace0, float* d_pts0, float* d_dirs_pt0, const cnerf_net* net1,
                                         const float* packed1, int64_t B1, int S1, const float* stash1, const float* workspace1,
                                         float* d_pts1, float* d_dirs_pt1, void* stream) {
  IgradPairArgs a;
  int rc = cn_make_geom(net0, &a.lv[0].g);
  if (rc || (rc = cn_make_geom(net1, &a.lv[1].g))) return rc;
  if (!packed0 || !stash0 || !workspace0 || !d_pts0 || B0 <= 0 || S0 <= 0) return CNERF_E_ARG;
  if (!packed1 || !stash1 || !workspace1 || !d_pts1 || B1 <= 0 || S1 <= 0) return CNERF_E_ARG;
  if ((d_dirs_pt0 && !a.lv[0].g.viewdirs) || (d_dirs_pt1 && !a.lv[1].g.viewdirs)) return CNERF_E_ARG;
  a.lv[0].packed = packed0; a.lv[0].stash = stash0; a.lv[0].G = workspace0; a.lv[0].d_pts = d_pts0; a.lv[0].d_dirs = d_dirs_pt0;
  a.lv[1].packed = packed1; a.lv[1].stash = stash1; a.lv[1].G = workspace1; a.lv[1].d_pts = d_pts1; a.lv[1].d_dirs = d_dirs_pt1;
  a.lv[0].M = B0 * S0;
  a.lv[1].M = B1 * S1;
  a.nb0 = (unsigned)cn_div_up(a.lv[0].M, 32);
  hipLaunchKernelGGL(mlp_igrad_pair_k, dim3(a.nb0 + (unsigned)cn_div_up(a.lv[1].M, 32)), dim3(64), 0, cn_stream(stream), a);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_rays_input_grad_pair(const float* d_pts0, const float* d_dirs_pt0, const float* z0, int S0, const float* d_pts1,
                                          const float* d_dirs_pt1, const float* z1, int S1, int64_t B, float* d_rays, int ray_stride,
                                          void* stream) {
  if (!d_pts0 || !z0 || !d_pts1 || !z1 || !d_rays || B <= 0 || S0 <= 0 || S1 <= 0 || ray_stride < 8) return CNERF_E_ARG;
  if ((d_dirs_pt0 != nullptr) != (d_dirs_pt1 != nullptr)) return CNERF_E_ARG;
  if (d_dirs_pt0 && ray_stride < 11) return CNERF_E_ARG;       // (the view directions are the last three columns, behind near / far)
  hipLaunchKernelGGL(rays_igrad_pair_k, dim3((unsigned)cn_div_up(B, 4)), dim3(256), 0, cn_stream(stream), d_pts0, d_dirs_pt0, z0, S0,
                     d_pts1, d_dirs_pt1, z1, S1, B, d_rays, ray_stride);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_composite_norm_grad_pair(const float* d_raw0, const float* raw0, int raw_ch0, const float* noise0, int S0,
                                              const float* d_raw1, const float* raw1, int raw_ch1, const float* noise1, int S1,
                                              const float* rays, int ray_stride, int64_t B, float* d_rays, void* stream) {
  if (!d_raw0 || !raw0 || !d_raw1 || !raw1 || !rays || !d_rays || B <= 0 || S0 <= 0 || S1 <= 0) return CNERF_E_ARG;
  if (raw_ch0 < 4 || raw_ch1 < 4 || ray_stride < 8) return CNERF_E_ARG;
  hipLaunchKernelGGL(composite_norm_pair_k, dim3((unsigned)cn_div_up(B, 4)), dim3(256), 0, cn_stream(stream), d_raw0, raw0, raw_ch0,
                     noise0, S0, d_raw1, raw1, raw_ch1, noise1, S1, rays, ray_stride, B, d_rays);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
