// Backward of the fused encoding+MLP (autograd of run_network R:37-52 / NeRF.forward H:107-130).
// Three launches:
//   1. dgrad (this file): one wave64 per 32 points walks the network backwards with the TRANSPOSED weight
//      panels as the MFMA A operand and the previous gradient's accumulator registers as B (mlp_common.hpp: no
//      LDS, no barriers); it writes the gradient w.r.t. every layer's pre-activation, dZ_l, into the tile-major
//      gradient workspace G[Mp][g_rows].
//   2. wgrad (wgrad.hip): NT GEMMs contracted over points, dW_l = dZ_l^T . H_{l-1}, split over point ranges.
//   3. a fixed-order reduction of the split partials into the parameter gradients (deterministic).
// ReLU masks come from the sign-bit words the forward packed into the stash (1 bit per hidden unit, s_mask).
#include "mlp_bwd_host.hpp"
#include "mlp_common.hpp"
#include "timing.hpp"

namespace {

// One level's operands.  A launch carries up to two levels of the SAME architecture (the coarse and the fine network of a
// training step: independent once the forward is done): blocks [0, nb0) walk level 0, the rest level 1 — one grid, so the
// 8 rounds of the coarse level ride behind the 24 of the fine one instead of paying their own ramp and tail.
struct BwdLevel {
  const float* packed;
  const float* d_raw;
  const float* stash;
  float* G;
  int64_t M, Mp;
  int64_t live_mul;   // points per ray of this level (with BwdArgs::live), 0 = no gating
  int64_t live_sub;   // rays in front of this level's arrays that are not part of the launch (first_ray of the _live calls)
};

struct BwdArgs {
  NetGeom g;
  BwdLevel lv[2];
  unsigned nb0;
  const int* live;    // device count of LIVE rays or nullptr: tiles at or beyond live * live_mul points retire at once (their raw
                      // outputs were zeros, their gradient tile rows are never read: wgrad clips its point ranges the same way)
};

#define CN_CONST __attribute__((address_space(4)))

template <int NT, bool VD>
__global__ __launch_bounds__(64) void mlp_dgrad_k(BwdArgs args_by_value) {
  constexpr int W = NT * 32;
  constexpr int NTH = NT / 2 > 0 ? NT / 2 : 1;
  constexpr int MD = (NT + 1) / 2, MDV = (NTH + 1) / 2;
  (void)args_by_value;   // read in place from the kernarg segment (scalar loads; the level is picked by blockIdx.x)
  const CN_CONST BwdArgs& args = *(const CN_CONST BwdArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const CN_CONST NetGeom& g = args.g;
  const unsigned nb0 = args.nb0;
  const bool second = blockIdx.x >= nb0;
  const CN_CONST BwdLevel& a = args.lv[second ? 1 : 0];
  const int lane = threadIdx.x, m = lane & 31, hh = lane >> 5;
  const int64_t p0 = (int64_t)(blockIdx.x - (second ? nb0 : 0u)) * 32;
  const int64_t p = p0 + m;
  const int nvalid = a.M - p0 < 32 ? (int)(a.M - p0) : 32;
  const int64_t pc = p < a.M ? p : a.M - 1;
  if (args.live != nullptr && a.live_mul > 0 && p0 >= ((int64_t)args.live[0] - a.live_sub) * a.live_mul) return;   // padding rays
  CN_TINIT(1)
  const APanel AP{make_rsrc(a.packed, (unsigned)(g.total * 4)), (m * 8 + 4 * hh) * 4};
  // this workgroup's stash tile row (sign bits) and gradient tile row (tile-major, mlp_common.hpp); lanes of padding
  // points address out of range: their bits read as 0 and their stores are dropped (the launcher zero-fills the last
  // tile row of G for the wgrad DMA)
  const rsrc_t srs = make_rsrc(a.stash + p0 * g.s_rows, (unsigned)(32 * g.s_rows * 4));
  const rsrc_t grs = make_rsrc(a.G + p0 * g.g_rows, (unsigned)(32 * g.g_rows * 4));
  const bool valid = p < a.M;
  const int gvo = valid ? m * 32 + hh * 16 : TM_OOB;
  const int smo = valid ? m * 32 + hh * MD * 4 : TM_OOB;
  f32x16 X[NT], Y[NT];
  f32x4 A[3][NT];   // A-operand register sets of the current transposed panel
  unsigned bits[MD];

  if (VD) {
    const float4 d = *reinterpret_cast<const float4*>(a.d_raw + pc * 4);
    const float dc[4] = {d.x, d.y, d.z, d.w};
    unsigned bv[MDV];
    load_bits<MDV>(srs, valid ? m * 32 + hh * MDV * 4 : TM_OOB, tm_col(g.s_mask + g.s_mb[g.D]), bv);
    a_prefetch3<NT>(A, AP, (int)g.t_views, W, g.Wh / 8 - 1);
    if (hh == 0) buf_store(grs, valid ? m * 32 : TM_OOB, tm_col(g.g_out), f32x4{d.x, d.y, d.z, d.w});
    // rgb_linear^T on the VALU, masked by the view-branch ReLU -> dZv (C-layout registers)
    f32x16 V[NTH];
    {
      f32x4 wq[3][NTH][4];   // all weight quads in flight before the first use: one exposed L2 round trip, not 12*NTH
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < NTH; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            wq[c][t][q] = buf_load(AP.rs, hh * 16, (int)(g.v_rgb + (int64_t)c * g.Wh + 32 * t + 8 * q) * 4);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NTH; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float sacc = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) sacc += wq[c][t][q][j] * dc[c];
            V[t][4 * q + j] = sacc;
          }
    }
    mask_bits<NTH>(V, bv);
    CN_T(0)
    // dF = views_linears^T (feature columns only; gamma(d) needs no gradient) . dZv, no mask (feature_linear is linear)
    gemm_reg3<NTH, NT, false, true>(X, V, A, AP, (int)g.t_views, W, hh, TileStores<NTH, NT>{V, grs, gvo, tm_col(g.g_hv)});
    pin<NT>(X);
    CN_T(2)
    // dZ_{D-1} = relu'(h_{D-1}) * (feature_linear^T . dF + alpha_linear^T . dsigma)
    // (only the first A set before the sigma-head quads: all three next to X, the quads and their products do not fit the
    //  arch-VGPR half of the register file; sets 1 and 2 are needed 32 and 64 MFMAs into the GEMM)
    a_load<NT>(A[0], AP, (int)g.t_feat, W, 0);
    load_bits<MD>(srs, smo, tm_col(g.s_mask + g.s_mb[g.D - 1]), bits);
    {
      // the weight quads land in Y's own registers and are scaled in place (all loads in flight before the first use: one
      // exposed L2 round trip; a separate staging array would be 128 more live registers next to X, Y and A)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 wq = buf_load(AP.rs, hh * 16, (int)(g.v_alpha + 32 * t + 8 * q) * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) Y[t][4 * q + j] = wq[j];
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[t][r] *= dc[3];
      a_load<NT>(A[1], AP, (int)g.t_feat, W, 1);
      a_load<NT>(A[2], AP, (int)g.t_feat, W, 2);
    }
    CN_T(4)
    gemm_reg3<NT, NT, false, false>(Y, X, A, AP, (int)g.t_feat, W, hh, TileStores<NT, NT>{X, grs, gvo, tm_col(g.g_feat)});
    CN_T(2)
  } else {
    load_bits<MD>(srs, smo, tm_col(g.s_mask + g.s_mb[g.D - 1]), bits);
    float dc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dc[c] = c < g.out_ch ? a.d_raw[pc * g.out_ch + c] : 0.f;
    if (hh == 0)
      for (int c = 0; c < g.out_ch; ++c)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dc[c]), grs, valid ? m * 32 : TM_OOB,
                                              tm_col(g.g_out + c), 0);
    // output_linear^T on the VALU
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < g.out_ch) {
            const f32x4 w = buf_load(AP.rs, hh * 16, (int)(g.v_out + (int64_t)c * W + 32 * t + 8 * q) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += w[j] * dc[c];
          }
#pragma unroll
        for (int j = 0; j < 4; ++j) Y[t][4 * q + j] = s[j];
      }
    CN_T(0)
  }
  if (g.D > 1) a_prefetch3<NT>(A, AP, (int)g.t_trunk[g.D - 1], W, W / 8 - 1);
  mask_bits<NT>(Y, bits);
  CN_T(3)
  // trunk: dZ_{l-1} = relu'(h_{l-1}) * (W_l^T . dZ_l) (the gamma(x) columns of the skip layer get no gradient); dZ_l
  // goes out to the workspace while it is the B operand of this GEMM.  X / Y alternate as input and output.
  auto layer = [&](f32x16 (&In)[NT], f32x16 (&Out)[NT], int l) __attribute__((always_inline)) {
    load_bits<MD>(srs, smo, tm_col(g.s_mask + g.s_mb[l - 1]), bits);
    gemm_reg3<NT, NT, false, true>(Out, In, A, AP, (int)g.t_trunk[l], W, hh, TileStores<NT, NT>{In, grs, gvo, tm_col(g.g_z[l])});
    if (l > 1) a_prefetch3<NT>(A, AP, (int)g.t_trunk[l - 1], W, W / 8 - 1);
    CN_T(2)
    mask_bits<NT>(Out, bits);
    CN_T(3)
  };
  int l = g.D - 1;
  for (; l >= 2; l -= 2) {
    layer(Y, X, l);
    layer(X, Y, l - 1);
  }
  if (l == 1) {   // (a third instance of the layer body: cheaper than keeping both sets live behind a flag)
    layer(Y, X, 1);
    store_tiles<NT>(X, grs, gvo, tm_col(g.g_z[0]));
  } else {
    store_tiles<NT>(Y, grs, gvo, tm_col(g.g_z[0]));
  }
  CN_T(3)
  CN_TEND
}

template <int NT>
int launch(const BwdArgs& a, int nlev, hipStream_t st) {
  unsigned grid = 0;
  for (int i = 0; i < nlev; ++i) {
    const BwdLevel& L = a.lv[i];
    grid += (unsigned)cn_div_up(L.M, 32);
    const hipError_t e = cn_zero_padding_tile_row(L.G, L.M, L.Mp, a.g.g_rows, st);
    if (e != hipSuccess) return (int)e;
  }
  if (a.g.viewdirs) hipLaunchKernelGGL((mlp_dgrad_k<NT, true>), dim3(grid), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((mlp_dgrad_k<NT, false>), dim3(grid), dim3(64), 0, st, a);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

int dispatch(const BwdArgs& a, int nlev, hipStream_t st) {
  switch (a.g.NT) {
    case 2: return launch<2>(a, nlev, st);
    case 4: return launch<4>(a, nlev, st);
    case 8: return launch<8>(a, nlev, st);
  }
  return CNERF_E_UNSUPPORTED;
}

// ---- the host path of every cnerf_mlp_{bwd,dgrad,wgrad}* entry point ---------------------------------------------------
// An entry point fills a Call and hands it to run(): validate -> operands -> dgrad and / or wgrad.

// One level as the C ABI passes it: arrays UNSHIFTED, first_ray = rays in front of them that carry zero seeds and are left out.
struct Level {
  const cnerf_net* net;
  const void* packed;        // cnerf_pack_weights floats, or with Call::bf3 cnerf_pack_weights_bf(.., 3, ..) bytes (dgrad)
  const float* d_raw;        // (dgrad)
  int64_t B;
  int S;
  const float* stash;
  float* workspace;
  const cnerf_ptrs* grads;   // (wgrad)
  int64_t first_ray;
};

struct Call {
  Level lv[2];
  int n;                       // 1, or 2: the coarse and the fine network of a training step (independent once the forward is done)
  bool live;                   // a _live form: both levels stop at live_rays[0] rays
  const int32_t* live_rays;    // device
  int bf3, accumulate;
  void* stream;
};

enum { DGRAD = 1, WGRAD = 2 };

bool same_arch(const cnerf_net& a, const cnerf_net& b) {
  return a.D == b.D && a.W == b.W && a.multires == b.multires && a.multires_views == b.multires_views &&
         a.use_viewdirs == b.use_viewdirs && a.output_ch == b.output_ch && a.skip == b.skip;
}

// Every argument rule of the backward, once.  Geometry first (an architecture outside the envelope is CNERF_E_UNSUPPORTED
// whatever else is wrong with the call), then the arguments (CNERF_E_ARG); an empty level (B == 0) is held to the same rules as
// any other and then takes no part in a launch.  Fills nets[i].g.
int validate(const Call& c, int stages, CnBwdNet* nets) {
  for (int i = 0; i < c.n; ++i) {
    int rc = cn_make_geom(c.lv[i].net, &nets[i].g);
    if (rc) return rc;
    if ((stages & DGRAD) && c.bf3 && (rc = cn_dgrad_bf3_supported(nets[i].g))) return rc;
  }
  if (c.live && !c.live_rays) return CNERF_E_ARG;
  if (c.live && c.bf3) return CNERF_E_UNSUPPORTED;      // (the device-side row count is the exact-fp32 bodies')
  for (int i = 0; i < c.n; ++i) {
    const Level& L = c.lv[i];
    if (!L.stash || !L.workspace || L.B < 0 || L.S <= 0) return CNERF_E_ARG;
    if ((stages & DGRAD) && (!L.packed || !L.d_raw)) return CNERF_E_ARG;
    if ((stages & WGRAD) && !L.grads) return CNERF_E_ARG;
    // tile rows are 32 points: a launch that stops at live * S points or starts at first_ray * S needs whole tiles per ray
    if (c.live && L.S % 32 != 0) return CNERF_E_ARG;
    if (L.first_ray && (!c.live || L.first_ray < 0 || L.first_ray >= L.B)) return CNERF_E_ARG;
  }
  if (c.n == 2) {
    if (c.live && c.lv[0].B != c.lv[1].B) return CNERF_E_ARG;      // the two levels of ONE ray batch
    if (stages & WGRAD)      // one gradient tensor in both sets: two reductions into it would race
      for (int i = 0; i < CNERF_MAX_TENSORS; ++i)
        if (c.lv[0].grads->p[i] && c.lv[0].grads->p[i] == c.lv[1].grads->p[i]) return CNERF_E_ARG;
  }
  return CNERF_OK;
}

// A level as the kernels take it — the ONE place where first_ray becomes addresses and counts (dgrad and wgrad must agree on
// them: a mismatch is an out-of-bounds read on the device, not an error code).  The level's first `first_ray` rays are left out:
// d_raw and the stash advance past their points (whole tile rows, validate()), the gradient workspace holds the launched rays'
// rows only, and the device-side live count is reduced by the same number.
void operands(const Level& L, bool live, CnBwdNet& n) {
  const int64_t o = L.first_ray * L.S;
  n.packed = L.packed;
  n.d_raw = L.d_raw ? L.d_raw + o * n.g.out_ch : nullptr;      // (out_ch = 4 with viewdirs: floats per point of d_raw)
  n.stash = L.stash + o * n.g.s_rows;
  n.G = L.workspace;
  n.M = L.B * L.S - o;
  n.Mp = cn_round_up(n.M, 32);
  n.partials = L.workspace + (int64_t)n.g.g_rows * n.Mp;
  n.cap = cn_wgrad_nsplit(n.Mp);
  n.grads = L.grads;
  n.live_mul = live ? L.S : 0;
  n.live_sub = (int)L.first_ray;
}

// nets[0, n) of one architecture in ONE grid: blocks [0, nb0) walk nets[0], the rest nets[1]
int dgrad(const CnBwdNet* nets, int n, const Call& c) {
  if (c.bf3) return cn_dgrad_bf3(nets, n, cn_stream(c.stream));
  BwdArgs a;
  a.g = nets[0].g;
  for (int i = 0; i < 2; ++i) {
    const CnBwdNet& s = nets[i < n ? i : 0];
    a.lv[i] = BwdLevel{static_cast<const float*>(s.packed), s.d_raw, s.stash, s.G, s.M, s.Mp, s.live_mul, s.live_sub};
  }
  a.nb0 = (unsigned)cn_div_up(nets[0].M, 32);
  a.live = c.live_rays;
  return dispatch(a, n, cn_stream(c.stream));
}

// Two non-empty levels of the same architecture share one grid (the 8 rounds of the coarse level ride behind the 24 of the fine
// one); otherwise one launch per non-empty level.
int run_dgrad(const Call& c, const CnBwdNet* nets) {
  if (c.n == 2 && nets[0].M > 0 && nets[1].M > 0 && same_arch(*c.lv[0].net, *c.lv[1].net)) return dgrad(nets, 2, c);
  for (int i = 0; i < c.n; ++i) {
    const int rc = nets[i].M > 0 ? dgrad(&nets[i], 1, c) : CNERF_OK;
    if (rc) return rc;
  }
  return CNERF_OK;
}

// The non-empty levels in one wgrad grid + one reduction, whatever their architectures.
int run_wgrad(const Call& c, const CnBwdNet* nets) {
  CnBwdNet run[2];
  int n = 0;
  for (int i = 0; i < c.n; ++i)
    if (nets[i].M > 0) run[n++] = nets[i];
  return n ? cn_wgrad_launch(run, n, c.accumulate, cn_stream(c.stream), c.bf3, c.live_rays) : CNERF_OK;
}

int run(const Call& c, int stages) {
  CnBwdNet nets[2];
  int rc = validate(c, stages, nets);
  if (rc) return rc;
  for (int i = 0; i < c.n; ++i) operands(c.lv[i], c.live, nets[i]);
  if ((stages & DGRAD) && (rc = run_dgrad(c, nets))) return rc;
  return (stages & WGRAD) ? run_wgrad(c, nets) : CNERF_OK;
}

}  // namespace

#ifdef CN_TIMING
CN_TIMING_ACCESSOR(cnerf_debug_timing_bwd)
#endif

extern "C" int64_t cnerf_mlp_bwd_ws_floats(const cnerf_net* net, int64_t M) {
  NetGeom g;
  if (cn_make_geom(net, &g) || M < 0) return -1;
  const int64_t Mp = cn_round_up(M, 32);
  return (int64_t)g.g_rows * Mp + (int64_t)cn_wgrad_nsplit(Mp) * cn_round_up(cn_param_floats(g), 64);
}

// ---- one network --------------------------------------------------------------------------------------------------------
extern "C" int cnerf_mlp_dgrad(const cnerf_net* net, const float* packed, const float* d_raw, int64_t B, int S,
                               const float* stash, float* workspace, void* stream) {
  return run(Call{{{net, packed, d_raw, B, S, stash, workspace}}, 1, false, nullptr, 0, 0, stream}, DGRAD);
}
extern "C" int cnerf_mlp_wgrad(const cnerf_net* net, int64_t B, int S, const float* stash, float* workspace,
                               const cnerf_ptrs* grads, int accumulate, void* stream) {
  return run(Call{{{net, nullptr, nullptr, B, S, stash, workspace, grads}}, 1, false, nullptr, 0, accumulate, stream}, WGRAD);
}
extern "C" int cnerf_mlp_bwd(const cnerf_net* net, const float* packed, const float* d_raw, int64_t B, int S,
                             const float* stash, float* workspace, const cnerf_ptrs* grads, int accumulate,
                             void* stream) {
  return run(Call{{{net, packed, d_raw, B, S, stash, workspace, grads}}, 1, false, nullptr, 0, accumulate, stream}, DGRAD | WGRAD);
}
// cnerf_mlp_bwd of a batch padded to a fixed capacity of B rays whose LIVE row count sits in device memory (cnerf_mlp_fwd_live)
extern "C" int cnerf_mlp_bwd_live(const cnerf_net* net, const float* packed, const float* d_raw, int64_t B, int S,
                                  const float* stash, float* workspace, const cnerf_ptrs* grads, int accumulate,
                                  const int32_t* live_rays, void* stream) {
  return run(Call{{{net, packed, d_raw, B, S, stash, workspace, grads}}, 1, true, live_rays, 0, accumulate, stream}, DGRAD | WGRAD);
}
// OPT-IN bf16x3 (second bench line only): the dgrad GEMMs, and the wide wgrad GEMMs, on the bf16 matrix cores at three planes per
// operand (mlp_bwd_bf.hip, wgrad.hip)
extern "C" int cnerf_mlp_dgrad_bf(const cnerf_net* net, const void* packed_bf, const float* d_raw, int64_t B, int S,
                                  const float* stash, float* workspace, void* stream) {
  return run(Call{{{net, packed_bf, d_raw, B, S, stash, workspace}}, 1, false, nullptr, 1, 0, stream}, DGRAD);
}
extern "C" int cnerf_mlp_wgrad_bf(const cnerf_net* net, int64_t B, int S, const float* stash, float* workspace,
                                  const cnerf_ptrs* grads, int accumulate, void* stream) {
  return run(Call{{{net, nullptr, nullptr, B, S, stash, workspace, grads}}, 1, false, nullptr, 1, accumulate, stream}, WGRAD);
}

// ---- two networks ---------------------------------------------------------------------------------------------------------
// Backward of TWO independent networks in one dgrad grid + one wgrad grid (+ one reduction): the coarse and the fine
// network of a render_rays training step (R:311-421) — their backward passes share nothing once the forward is done
// (the fine level's sample depths are detached, R:397).  The dgrad grid is shared when both have the same architecture,
// otherwise two dgrad launches; the wgrad grid is always shared.  net0 / net1 must be different parameter sets.
// Workspaces as for cnerf_mlp_bwd, one per network.
extern "C" int cnerf_mlp_dgrad_pair(const cnerf_net* net0, const float* packed0, const float* d_raw0, int64_t B0, int S0,
                                    const float* stash0, float* workspace0, const cnerf_net* net1, const float* packed1,
                                    const float* d_raw1, int64_t B1, int S1, const float* stash1, float* workspace1,
                                    void* stream) {
  return run(Call{{{net0, packed0, d_raw0, B0, S0, stash0, workspace0}, {net1, packed1, d_raw1, B1, S1, stash1, workspace1}},
                  2, false, nullptr, 0, 0, stream}, DGRAD);
}
extern "C" int cnerf_mlp_wgrad_pair(const cnerf_net* net0, int64_t B0, int S0, const float* stash0, float* workspace0,
                                    const cnerf_ptrs* grads0, const cnerf_net* net1, int64_t B1, int S1,
                                    const float* stash1, float* workspace1, const cnerf_ptrs* grads1, int accumulate,
                                    void* stream) {
  return run(Call{{{net0, nullptr, nullptr, B0, S0, stash0, workspace0, grads0}, {net1, nullptr, nullptr, B1, S1, stash1, workspace1, grads1}},
                  2, false, nullptr, 0, accumulate, stream}, WGRAD);
}
extern "C" int cnerf_mlp_bwd_pair(const cnerf_net* net0, const float* packed0, const float* d_raw0, int64_t B0, int S0,
                                  const float* stash0, float* workspace0, const cnerf_ptrs* grads0,
                                  const cnerf_net* net1, const float* packed1, const float* d_raw1, int64_t B1, int S1,
                                  const float* stash1, float* workspace1, const cnerf_ptrs* grads1, int accumulate,
                                  void* stream) {
  return run(Call{{{net0, packed0, d_raw0, B0, S0, stash0, workspace0, grads0}, {net1, packed1, d_raw1, B1, S1, stash1, workspace1, grads1}},
                  2, false, nullptr, 0, accumulate, stream}, DGRAD | WGRAD);
}
extern "C" int cnerf_mlp_dgrad_bf_pair(const cnerf_net* net0, const void* packed_bf0, const float* d_raw0, int64_t B0, int S0,
                                       const float* stash0, float* workspace0, const cnerf_net* net1, const void* packed_bf1,
                                       const float* d_raw1, int64_t B1, int S1, const float* stash1, float* workspace1,
                                       void* stream) {
  return run(Call{{{net0, packed_bf0, d_raw0, B0, S0, stash0, workspace0}, {net1, packed_bf1, d_raw1, B1, S1, stash1, workspace1}},
                  2, false, nullptr, 1, 0, stream}, DGRAD);
}
extern "C" int cnerf_mlp_wgrad_bf_pair(const cnerf_net* net0, int64_t B0, int S0, const float* stash0, float* workspace0,
                                       const cnerf_ptrs* grads0, const cnerf_net* net1, int64_t B1, int S1,
                                       const float* stash1, float* workspace1, const cnerf_ptrs* grads1, int accumulate,
                                       void* stream) {
  return run(Call{{{net0, nullptr, nullptr, B0, S0, stash0, workspace0, grads0}, {net1, nullptr, nullptr, B1, S1, stash1, workspace1, grads1}},
                  2, false, nullptr, 1, accumulate, stream}, WGRAD);
}

// cnerf_mlp_bwd_pair of two levels of ONE ray batch padded to a fixed capacity (B0 == B1 rays) whose LIVE row count sits in device
// memory: both levels' dgrad tiles and wgrad point ranges stop at live_rays * S of their level; and its two halves
extern "C" int cnerf_mlp_dgrad_pair_live(const cnerf_net* net0, const float* packed0, const float* d_raw0, int64_t B0, int S0,
                                         const float* stash0, float* workspace0, const cnerf_net* net1, const float* packed1,
                                         const float* d_raw1, int64_t B1, int S1, const float* stash1, float* workspace1,
                                         const int32_t* live_rays, int64_t first_ray0, int64_t first_ray1, void* stream) {
  return run(Call{{{net0, packed0, d_raw0, B0, S0, stash0, workspace0, nullptr, first_ray0},
                   {net1, packed1, d_raw1, B1, S1, stash1, workspace1, nullptr, first_ray1}},
                  2, true, live_rays, 0, 0, stream}, DGRAD);
}
extern "C" int cnerf_mlp_wgrad_pair_live(const cnerf_net* net0, int64_t B0, int S0, const float* stash0, float* workspace0,
                                         const cnerf_ptrs* grads0, const cnerf_net* net1, int64_t B1, int S1, const float* stash1,
                                         float* workspace1, const cnerf_ptrs* grads1, int accumulate, const int32_t* live_rays,
                                         int64_t first_ray0, int64_t first_ray1, void* stream) {
  return run(Call{{{net0, nullptr, nullptr, B0, S0, stash0, workspace0, grads0, first_ray0},
                   {net1, nullptr, nullptr, B1, S1, stash1, workspace1, grads1, first_ray1}},
                  2, true, live_rays, 0, accumulate, stream}, WGRAD);
}
extern "C" int cnerf_mlp_bwd_pair_live(const cnerf_net* net0, const float* packed0, const float* d_raw0, int64_t B0, int S0,
                                       const float* stash0, float* workspace0, const cnerf_ptrs* grads0,
                                       const cnerf_net* net1, const float* packed1, const float* d_raw1, int64_t B1, int S1,
                                       const float* stash1, float* workspace1, const cnerf_ptrs* grads1, int accumulate,
                                       const int32_t* live_rays, int64_t first_ray0, int64_t first_ray1, void* stream) {
  return run(Call{{{net0, packed0, d_raw0, B0, S0, stash0, workspace0, grads0, first_ray0},
                   {net1, packed1, d_raw1, B1, S1, stash1, workspace1, grads1, first_ray1}},
                  2, true, live_rays, 0, accumulate, stream}, DGRAD | WGRAD);
}

