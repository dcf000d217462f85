// Alpha compositing along rays (raw2outputs, reference R:265-308 / V:392-438) and its backward.
// One wave64 per ray: lane l owns the C = ceil(S/64) consecutive samples [l*C, l*C+C).  The exclusive
// transmittance product is a lane-local sequential product + one wave scan, carried in fp64 and
// rounded to fp32 per sample (the CPU reference's cumprod accumulates fp32 inputs in fp64).
// HBM-bound: 24 B per ray-sample forward (raw 16 + z 4 in, weights 4 out), 40 B backward.
#include "loss_terms.hpp"
#include "raygen.hpp"

namespace {

constexpr int WAVES = 4;

// img2mse(rgb_map, target) (H:9, R:769-775) folded into the compositing of a level.  Forward: every workgroup leaves the fp64 sum of
// its rays' squared colour errors in part[blockIdx.x]; the workgroup that takes the last ticket of `counter` sums the partials IN
// INDEX ORDER (the value does not depend on which workgroup finished last), writes loss[0] = fp32(sum / n) (+ loss_add[0]: the other
// level's term, `img_loss + img_loss0` in fp32 like R:775) and re-arms the counter.  Backward: the seed d loss / d rgb_map =
// (2 / n) (rgb_map - target) * g[0] is formed per ray in registers — same operations, same order as img2mse's own backward, so the
// fused and the separate paths agree bit for bit.
constexpr int MSE_WAVES = CN_CLOSS_RAYS_PER_WG;   // rays per workgroup of the loss form (common.hpp: loss.hip indexes the partials)
constexpr unsigned MSE_GROUP = 64;        // workgroups per first-level ticket counter
constexpr unsigned MSE_CTR_STRIDE = 64;   // uint32 words between counters (256 B: one counter per cache line / channel)
constexpr unsigned MSE_CTR_WORDS = 16384; // the caller's zeroed counter block: top counter + up to 255 group counters
struct MseFwd {
  const float* tgt;      // [B,3]; nullptr = no loss
  double* part;          // [gridDim.x]
  unsigned* counter;     // MSE_CTR_WORDS words, zero on entry, zero on exit
  float* loss;           // [1]
  const float* loss_add; // [1] or nullptr
  double n;              // elements of the mean (3 B)
};
struct MseBwd {
  const float* rgb;      // forward rgb_map [B,3]; nullptr = seeds come from g_rgb
  const float* tgt;
  const float* g;        // upstream gradient of the loss (device scalar) or nullptr = 1
  float w;               // fp32(2 / n)
};

// ConsistentNeRF's masked losses (V:1645-1648, V:1737, V:1786-1788, V:1865) folded into the compositing of a level the same way —
// without tickets: every workgroup leaves FIVE fp64 partials (squared colour error over the rays with m == 1 and with m == 0, squared
// depth error (depth / far - prior / far)^2 over m == 1, and the two counts) in part[k * gridDim.x + blockIdx.x]; the step's loss
// tail (loss.hip closs_tail_k, the next launch on the stream: it also evaluates the monocular patch term, which needs whole
// depth maps) sums them in index order, normalises by the (possibly global) counts and leaves the three seed weights the backward
// uses.  Backward: seed_rgb = (w_m (rgb - target)) * g_rgb, seed_depth = (w_d (depth / far - prior / far)) * g_depth (+ the patch
// term's d_depth * g_patch on the patch rays) — the stand-alone kernels' own per-ray functions (loss_terms.hpp, which both files
// include: that is what makes the two routes agree bit for bit) / patch_depth_loss_k's seeds and autograd's `d * g`.
// The other live loss forms of V / VC (cnerf_lossform, include/cnerf.h): what the FORMS instantiations of the two kernels add.  The
// new depth forms divide by far as ATen divides a tensor by a scalar, x * (1 / far): their literal lines run on ATen.
struct LossForm {
  int rgb_form = CNERF_RGB_HARDMASK, depth_form = CNERF_DEPTH_HARDMASK;
  float lp_coef = 0.f, coef = 0.f;   // (coef = hardmask_coef: the backward's weight of the mask == 0 depth seeds)
  const float* temp_rgb = nullptr;
  const float* temp_depth = nullptr;
};

struct ClossFwd {
  const float* tgt;      // [B,3]
  const float* mask;     // [B] or nullptr (every ray in the m == 1 set)
  const float* prior;    // [B] or nullptr (no depth term)
  float far;
  double* part;          // [5][gridDim.x]; the FORMS kernels: [CNERF_LOSSFORM_SLOTS][gridDim.x]
  LossForm form;         // the FORMS kernels only
};
struct ClossBwd {
  const float* rgb;      // forward rgb_map [B,3]
  const float* depth;    // forward depth_map [B] (with prior)
  const float* tgt;
  const float* mask;
  const float* prior;
  const float* stats;    // device [3]: w1, w0, wd (closs_tail_k); with seg_row > 0: [2][4], the second set for rays >= seg_row
  int64_t seg_row;       // 0, or the first ray of the batch's second segment (cnerf_closs::seg_row: the one-render a15 step)
  const float* g;        // upstream gradient of the total loss (device scalar) or nullptr = 1
  const float* patch_d;  // [n_patch] d patch_loss / d depth of this level, or nullptr
  int64_t n_patch;
  float far, rgb_w, depth_w, patch_w;
  const float* ssim_d;   // [n_ssim * 3] d ssim_level / d rgb of this level (cnerf_closs_finish_ssim), or nullptr
  int64_t n_ssim;
  float ssim_w;
  const float* lpips_d;  // [n_lpips / 256][3][16][16] cnerf_lpips_bwd's gradient w.r.t. this level's patch images, or nullptr
  int64_t n_lpips;
  LossForm form;         // the FORMS kernel only: stats = the level's 8 floats of cnerf_lossform_finish
  const float* d_temp;   // [2] the level's (rgb_w dL_rgb / dt, depth_w dL_depth / dt), or nullptr
  float* g_temp;         // [2] <- d_temp * g
};

struct Sample {
  float e;      // exp(-relu(sigma)*dist)
  float alpha;  // 1 - e
  float x;      // 1 - alpha + 1e-10   (factor of the transmittance product)
  float r, g, b;  // sigmoid colours
  float z, dist, sig;
  bool live;
};

template <int C>
__device__ __forceinline__ void load_samples(Sample (&sm)[C], const float* __restrict__ raw, int ch,
                                             const float* __restrict__ zrow, const float* __restrict__ nrow,
                                             float dnorm, int S, int lane) {
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int s = lane * C + j;
    Sample& q = sm[j];
    q.live = s < S;
    if (!q.live) {
      q.e = 1.f; q.alpha = 0.f; q.x = 1.f; q.r = q.g = q.b = 0.f; q.z = 0.f; q.dist = 0.f; q.sig = 0.f;
      continue;
    }
    float c0, c1, c2, sg;
    if (ch == 4) {
      const float4 v = *reinterpret_cast<const float4*>(raw + (int64_t)s * 4);
      c0 = v.x; c1 = v.y; c2 = v.z; sg = v.w;
    } else {
      const float* p = raw + (int64_t)s * ch;
      c0 = p[0]; c1 = p[1]; c2 = p[2]; sg = p[3];
    }
    q.z = zrow[s];
    float d = (s + 1 < S) ? (zrow[s + 1] - q.z) : 1e10f;   // R:280-281
    q.dist = d * dnorm;                                      // R:283
    if (nrow) sg = sg + nrow[s];                             // R:296
    q.sig = sg;
    const float act = sg > 0.f ? sg : 0.f;
    q.e = expf(-act * q.dist);
    q.alpha = 1.f - q.e;
    q.x = 1.f - q.alpha + 1e-10f;                            // R:298
    q.r = 1.f / (1.f + expf(-c0));
    q.g = 1.f / (1.f + expf(-c1));
    q.b = 1.f / (1.f + expf(-c2));
  }
}

// exclusive product scan over all samples of the ray; T[j] = fp32(prod_{k<s} x_k)
template <int C>
__device__ __forceinline__ void transmittance(const Sample (&sm)[C], float (&T)[C], int lane) {
  double p = 1.0;
#pragma unroll
  for (int j = 0; j < C; ++j) p *= (double)sm[j].x;
  double incl = p;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    double v = __shfl_up(incl, o, 64);
    if (lane >= o) incl *= v;
  }
  double run = __shfl_up(incl, 1, 64);
  if (lane == 0) run = 1.0;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    T[j] = (float)run;
    run *= (double)sm[j].x;
  }
}

__device__ __forceinline__ float ray_norm(const float* __restrict__ ray) {
  const float dx = ray[3], dy = ray[4], dz = ray[5];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// one ray by one wave64; returns (lane 0) the squared colour error against tgt (0 without a target)
template <int C>
__device__ __forceinline__ double composite_ray(const float* __restrict__ raw, int ch, const float* __restrict__ z,
                                               const float* __restrict__ rays, int rs, const float* __restrict__ noise, int64_t b,
                                               int S, int white, float* __restrict__ rgb, float* __restrict__ disp,
                                               float* __restrict__ acc, float* __restrict__ depth, float* __restrict__ weights,
                                               const RayGenDev& cam, const float* __restrict__ tgt, float (&out4)[4]) {
  const int lane = threadIdx.x & 63;
  double err = 0.0;
  Sample sm[C];
  float T[C];
  float dn;
  if (rays != nullptr) {
    dn = ray_norm(rays + b * rs);
  } else {   // the ray of a camera, generated here (raygen.hpp): R:280-283 scales the sample distances by |rays_d|
    float o[3], d[3], v[3];
    cn_gen_ray(cam, cam.first + b, o, d, v);
    dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  }
  load_samples<C>(sm, raw + b * S * ch, ch, z + b * S, noise ? noise + b * S : nullptr, dn, S, lane);
  transmittance<C>(sm, T, lane);
  double sr = 0, sg = 0, sb = 0, sd = 0, sa = 0;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const float w = sm[j].alpha * T[j];
    if (sm[j].live) {
      if (weights) weights[b * S + lane * C + j] = w;
      sr += (double)(w * sm[j].r);
      sg += (double)(w * sm[j].g);
      sb += (double)(w * sm[j].b);
      sd += (double)(w * sm[j].z);
      sa += (double)w;
    }
  }
  sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sd = wave_sum(sd); sa = wave_sum(sa);
  if (lane == 0) {
    const float fa = (float)sa, fd = (float)sd;
    float r = (float)sr, g = (float)sg, bl = (float)sb;
    if (white) { const float bg = 1.f - fa; r += bg; g += bg; bl += bg; }   // R:305-306
    out4[0] = r; out4[1] = g; out4[2] = bl; out4[3] = fd;
    if (rgb) { rgb[b * 3 + 0] = r; rgb[b * 3 + 1] = g; rgb[b * 3 + 2] = bl; }
    if (acc) acc[b] = fa;
    if (depth) depth[b] = fd;
    if (disp) {
      const float q = fd / fa;                          // 0/0 -> NaN propagates like torch.max (R:302)
      disp[b] = (q != q) ? q : 1.f / fmaxf(1e-10f, q);
    }
    if (tgt) {                                          // (x - y)^2 per element in fp32, summed in fp64 like mse_k (loss.hip)
      const float d0 = r - tgt[b * 3 + 0], d1 = g - tgt[b * 3 + 1], d2 = bl - tgt[b * 3 + 2];
      err = (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2);
    }
  }
  return err;
}

// WV = rays (waves) per workgroup: WAVES for the plain form; MSE_WAVES for the loss form (fewer, fatter partials and tickets)
template <int C, int WV, bool FORMS = false>
__global__ __launch_bounds__(WV * 64) void composite_fwd_k(const float* __restrict__ raw, int ch,
                                                              const float* __restrict__ z,
                                                              const float* __restrict__ rays, int rs,
                                                              const float* __restrict__ noise, int64_t B, int S,
                                                              int white, float* __restrict__ rgb,
                                                              float* __restrict__ disp, float* __restrict__ acc,
                                                              float* __restrict__ depth, float* __restrict__ weights,
                                                              RayGenDev cam, MseFwd mse, ClossFwd cl) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * WV + (threadIdx.x >> 6);
  float o4[4] = {0.f, 0.f, 0.f, 0.f};
  if (FORMS || cl.tgt != nullptr) {
    // masked-loss variant: per-ray terms in lane 0 (loss_terms.hpp: the stand-alone kernels' own functions — fp32 terms, fp64 sums),
    // NS partials per workgroup summed over its waves in wave order; no tickets (see ClossFwd).  FORMS: a form per kind of term,
    // CNERF_LOSSFORM_SLOTS partials (cnerf.h)
    constexpr int NS = FORMS ? CNERF_LOSSFORM_SLOTS : LT_MASKED_SLOTS;
    __shared__ double sq[WV][NS];
    double t[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) t[k] = 0.0;
    if (b < B) {
      composite_ray<C>(raw, ch, z, rays, rs, noise, b, S, white, rgb, disp, acc, depth, weights, cam, nullptr, o4);
      if (lane == 0) {
        const float m = cl.mask ? cl.mask[b] : 1.f;
        const float* const tg = cl.tgt + b * 3;
        if constexpr (!FORMS) {
          lt_accum_ray(t, m, lt_sq_err3(o4, tg));
          if (cl.prior) lt_accum_depth(t, m, lt_depth_res(o4[3], cl.prior[b], cl.far));
        } else {
          const LossForm& f = cl.form;
          lt_accum_counts(t, m);
          if (f.rgb_form == CNERF_RGB_HARDMASK) {
            lt_accum_colour(t, m, lt_sq_err3(o4, tg));
          } else {
            const bool sm = f.rgb_form == CNERF_RGB_SOFTMASK;
            const float tr = sm ? f.temp_rgb[0] : 1.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) lt_soft_sums(sm, o4[c] - tg[c], f.lp_coef, tr, t[LT_C_W], t[LT_C_WD2], t[LT_C_WD4]);
          }
          if (cl.prior) {
            const float inv = 1.f / cl.far, p = cl.prior[b];
            if (f.depth_form == CNERF_DEPTH_HARDMASK) {
              lt_accum_depth(t, m, lt_depth_res(o4[3], p, cl.far));
            } else if (f.depth_form == CNERF_DEPTH_HARDMASK_COEF) {
              const float d = lt_depth_res_form(o4[3], p, inv);
              lt_accum_depth(t, m, d);
              if (m == 0.f) t[LT_D_W] = (double)(d * d);
            } else if (f.depth_form == CNERF_DEPTH_NORM) {
              const float d = lt_depth_res_form(o4[3], m == 0.f ? 0.f : p, inv);
              t[LT_SD] = (double)(d * d);
            } else if (f.depth_form == CNERF_DEPTH_PLAIN) {
              const float d = o4[3] - (m == 0.f ? 0.f : p);
              t[LT_SD] = (double)(d * d);
            } else {
              const bool sm = f.depth_form == CNERF_DEPTH_SOFTMASK;
              lt_soft_sums(sm, lt_depth_res_form(o4[3], p, inv), f.lp_coef, sm ? f.temp_depth[0] : 1.f, t[LT_D_W], t[LT_D_WD2], t[LT_SD]);
            }
          }
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) sq[threadIdx.x >> 6][k] = t[k];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
      double s = 0.0;
      for (int w = 0; w < WV; ++w) s += sq[w][threadIdx.x];
      cl.part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
    return;
  }
  if (mse.tgt != nullptr) {
    // loss variant: every wave reaches the workgroup reduction below (a wave past the last ray contributes 0); after it only wave 0
    // stays for the tickets (the others retire: a workgroup that waits ~2 us for two memory round trips must not hold 16 wave slots)
    __shared__ double sq[WV];
    double e = 0.0;
    if (b < B) e = composite_ray<C>(raw, ch, z, rays, rs, noise, b, S, white, rgb, disp, acc, depth, weights, cam, mse.tgt, o4);
    if (lane == 0) sq[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    int is_last = 0;
    if (lane == 0) {
      double s = 0.0;
      for (int w = 0; w < WV; ++w) s += sq[w];
      // Publish the partial, then take a ticket.  Everything that crosses workgroups here is an agent-scope ATOMIC access: the
      // partial is stored write-through (`global_store_dwordx2 ... sc1`), the reducer loads it with sc1, so neither side needs an
      // L2 write-back / invalidate (the agent-scope release fence = `buffer_wbl2 sc1` made every workgroup write back its XCD's
      // L2: 44 us per launch).  What the ticket DOES need is the store's completion: vmcnt(0) between the store and the atomic.
      // A workgroup-scope release fence compiles to NOTHING on gfx950 (the ticket could overtake the partial), so the
      // wait is written out; `scripts/isa_ticket_check.py` asserts the s_waitcnt vmcnt(0) sits between the two in the ISA.
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(mse.part) + blockIdx.x, (unsigned long long)__double_as_longlong(s),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // vmcnt(0): the sc1 store has been acknowledged by the memory side.  Written as inline assembly with a "memory" clobber
      // (ADVICE r05): the mnemonic carries no architecture-specific immediate (the builtin's 0x0f70 is the gfx9 encoding), and the
      // clobber is a compiler-level barrier on BOTH sides — the partial's store cannot sink below the wait, the ticket RMW cannot be
      // hoisted above it — which the s_waitcnt builtin (IntrNoMem) + a sched_barrier after it did not state.  The order in the ISA
      // is asserted at BUILD time (consistentnerf_amd/build.py -> scripts/isa_ticket_check.py), not only by a test.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      // Two-level ticket: same-address atomics at agent scope serialise at ~40 ns each (measured: 8192 workgroups on ONE counter
      // cost 0.36 ms), so a workgroup first tickets inside its group of MSE_GROUP (one counter per group, 256 B apart); the last of
      // a group tickets at the top.  <= MSE_GROUP + ngroups serialised atomics instead of gridDim.x.
      const unsigned grp = blockIdx.x / MSE_GROUP, ngroups = (gridDim.x + MSE_GROUP - 1) / MSE_GROUP;
      const unsigned in_grp = grp + 1 == ngroups ? gridDim.x - grp * MSE_GROUP : MSE_GROUP;
      unsigned* gctr = mse.counter + MSE_CTR_STRIDE * (1 + grp);
      bool last = false;
      if (__hip_atomic_fetch_add(gctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1) {
        __hip_atomic_store(gctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // re-arm (nobody else touches it any more)
        last = __hip_atomic_fetch_add(mse.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1;
      }
      is_last = last;
    }
    is_last = __builtin_amdgcn_readfirstlane(is_last);
    if (is_last) {
      // The tickets form a chain of agent-scope RMWs on device memory: the last ticket was granted after every other workgroup's
      // (its partial complete before it, above).  The partial loads below are agent-scope atomic loads (sc1: served by the memory
      // side, never by this XCD's L2 or the vector L1) and depend on is_last, which came back from the ticket atomic, so they cannot
      // be issued before it returned.
      double s = 0.0;
      for (unsigned i = lane; i < gridDim.x; i += 64)
        s += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(mse.part) + i, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT));
      s = wave_sum(s);
      if (lane == 0) {
        float l = (float)(s / mse.n);
        if (mse.loss_add) l = l + mse.loss_add[0];
        mse.loss[0] = l;
        __hip_atomic_store(mse.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    return;
  }
  if (b >= B) return;
  composite_ray<C>(raw, ch, z, rays, rs, noise, b, S, white, rgb, disp, acc, depth, weights, cam, nullptr, o4);
}

template <int C, bool FORMS = false>
__global__ __launch_bounds__(WAVES * 64) void composite_bwd_k(const float* __restrict__ raw, int ch,
                                                              const float* __restrict__ z,
                                                              const float* __restrict__ rays, int rs,
                                                              const float* __restrict__ noise, int64_t B, int S,
                                                              int white, const float* __restrict__ g_rgb,
                                                              const float* __restrict__ g_disp,
                                                              const float* __restrict__ g_acc,
                                                              const float* __restrict__ g_depth,
                                                              float* __restrict__ d_raw, MseBwd mse, ClossBwd cl) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  Sample sm[C];
  float T[C];
  load_samples<C>(sm, raw + b * S * ch, ch, z + b * S, noise ? noise + b * S : nullptr, ray_norm(rays + b * rs), S,
                  lane);
  transmittance<C>(sm, T, lane);
  float gr = 0.f, gg = 0.f, gb = 0.f, gd = 0.f, ga = 0.f;
  if (g_rgb) { gr = g_rgb[b * 3 + 0]; gg = g_rgb[b * 3 + 1]; gb = g_rgb[b * 3 + 2]; }
  if (mse.rgb) {   // the img2mse seed of this level, formed here: (w * (x - y)) * g — the operations of mse_k then `d_x * g`
    const float g0 = mse.g ? mse.g[0] : 1.f;
    gr += (mse.w * (mse.rgb[b * 3 + 0] - mse.tgt[b * 3 + 0])) * g0;
    gg += (mse.w * (mse.rgb[b * 3 + 1] - mse.tgt[b * 3 + 1])) * g0;
    gb += (mse.w * (mse.rgb[b * 3 + 2] - mse.tgt[b * 3 + 2])) * g0;
  }
  if (g_depth) gd = g_depth[b];
  if (cl.rgb) {    // the masked rgb / depth seeds (+ the patch term's) of this level, formed here (see ClossBwd)
    const float g0 = cl.g ? cl.g[0] : 1.f;
    const float m = cl.mask ? cl.mask[b] : 1.f;
    const float* const st = cl.stats + ((cl.seg_row > 0 && b >= cl.seg_row) ? 4 : 0);
    const float w = lt_ray_w(m, st[0], st[1]);
    const float g_rgb_l = cl.rgb_w * g0;
    bool v6_rgb = true, v6_depth = true;
    if constexpr (FORMS) {
      // the form's seeds: the operations of the literal lines' backward (mse_k's d_x / loss_terms.hpp's soft seeds, autograd's
      // `d_x * g`, then the `* (1 / far)` of ATen's tensor / scalar), see LossForm
      const LossForm& f = cl.form;
      if (b == 0 && lane == 0 && cl.g_temp) { cl.g_temp[0] = cl.d_temp[0] * g0; cl.g_temp[1] = cl.d_temp[1] * g0; }
      if (f.rgb_form != CNERF_RGB_HARDMASK) {
        v6_rgb = false;
        const bool sm = f.rgb_form == CNERF_RGB_SOFTMASK;
        const float tr = sm ? f.temp_rgb[0] : 1.f;
        gr += lt_soft_seed(sm, cl.rgb[b * 3 + 0] - cl.tgt[b * 3 + 0], f.lp_coef, tr, st[4]) * g_rgb_l;
        gg += lt_soft_seed(sm, cl.rgb[b * 3 + 1] - cl.tgt[b * 3 + 1], f.lp_coef, tr, st[4]) * g_rgb_l;
        gb += lt_soft_seed(sm, cl.rgb[b * 3 + 2] - cl.tgt[b * 3 + 2], f.lp_coef, tr, st[4]) * g_rgb_l;
      }
      if (cl.prior && f.depth_form != CNERF_DEPTH_HARDMASK) {
        v6_depth = false;
        const float inv = 1.f / cl.far, p = cl.prior[b], g_d = cl.depth_w * g0;
        if (f.depth_form == CNERF_DEPTH_HARDMASK_COEF) {
          const float x = lt_depth_res_form(cl.depth[b], p, inv);
          if (m == 1.f) gd += ((st[2] * x) * g_d) * inv;
          if (m == 0.f) gd += ((st[3] * x) * (g_d * f.coef)) * inv;
        } else if (f.depth_form == CNERF_DEPTH_NORM) {
          gd += ((st[2] * lt_depth_res_form(cl.depth[b], m == 0.f ? 0.f : p, inv)) * g_d) * inv;
        } else if (f.depth_form == CNERF_DEPTH_PLAIN) {
          gd += (st[2] * (cl.depth[b] - (m == 0.f ? 0.f : p))) * g_d;
        } else {
          const bool sm = f.depth_form == CNERF_DEPTH_SOFTMASK;
          gd += (lt_soft_seed(sm, lt_depth_res_form(cl.depth[b], p, inv), f.lp_coef, sm ? f.temp_depth[0] : 1.f, st[2]) * g_d) * inv;
        }
      }
    }
    if (v6_rgb) {
      gr += lt_seed_colour(w, cl.rgb[b * 3 + 0], cl.tgt[b * 3 + 0]) * g_rgb_l;
      gg += lt_seed_colour(w, cl.rgb[b * 3 + 1], cl.tgt[b * 3 + 1]) * g_rgb_l;
      gb += lt_seed_colour(w, cl.rgb[b * 3 + 2], cl.tgt[b * 3 + 2]) * g_rgb_l;
    }
    if (cl.prior && v6_depth) gd += lt_seed_depth(m, st[2], cl.depth[b], cl.prior[b], cl.far) * (cl.depth_w * g0);
    if (cl.patch_d && b < cl.n_patch) gd += cl.patch_d[b] * (cl.patch_w * g0);
    float sr = 0.f, sg = 0.f, sb = 0.f;
    if (cl.ssim_d) {   // loss -= ssim_w ssim_level: autograd's `d * ((-g) * ssim_w)`, zero past the patch rays (the padded gradient)
      const float gs = (-g0) * cl.ssim_w;
      const bool in = b < cl.n_ssim;
      sr = in ? cl.ssim_d[b * 3 + 0] * gs : 0.f;
      sg = in ? cl.ssim_d[b * 3 + 1] * gs : 0.f;
      sb = in ? cl.ssim_d[b * 3 + 2] * gs : 0.f;
    }
    if (!FORMS && cl.lpips_d) {   // (the loss forms take the term on the lines: run_nerf_view.render_loss)
      // loss += lpips_w lpips_level: the `* 2` of (rgb - 0.5) * 2 on the level's slice of cnerf_lpips_bwd's NCHW gradient, read in place
      // (ray p 256 + y 16 + x, colour c <- dX[p][c][y][x]; the seeds already carry g lpips_w / 4).  On the lines the engine runs the
      // LPIPS chain before the SSIM node and the colour term's last: (lpips + ssim) + colour
      const bool in = b < cl.n_lpips;
      const float* const d = cl.lpips_d + (b >> 8) * 768 + (b & 255);
      sr = (in ? d[0] * 2.f : 0.f) + sr;
      sg = (in ? d[256] * 2.f : 0.f) + sg;
      sb = (in ? d[512] * 2.f : 0.f) + sb;
    }
    if (cl.ssim_d || (!FORMS && cl.lpips_d)) { gr += sr; gg += sg; gb += sb; }
  }
  if (g_acc) ga = g_acc[b];
  if (white) ga -= (gr + gg + gb);
  if (g_disp) {
    // disp = 1/max(1e-10, depth/acc): needs the forward totals
    double sd = 0, sa = 0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const float w = sm[j].alpha * T[j];
      sd += (double)(w * sm[j].z);
      sa += (double)w;
    }
    const float fd = (float)wave_sum(sd), fa = (float)wave_sum(sa);
    const float q = fd / fa;
    if (q > 1e-10f) {
      const float gq = -g_disp[b] / (q * q);
      gd += gq / fa;
      ga += -gq * fd / (fa * fa);
    }
  }
  // v_i = dL/dw_i ; suffix sums S_i = sum_{k>i} w_k v_k (reverse exclusive scan, fp64)
  float v[C];
  double tot = 0.0;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    v[j] = gr * sm[j].r + gg * sm[j].g + gb * sm[j].b + gd * sm[j].z + ga;
    tot += (double)(sm[j].alpha * T[j]) * (double)v[j];
  }
  double incl = tot;   // inclusive suffix over lanes >= l
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    double t = __shfl_down(incl, o, 64);
    if (lane + o < 64) incl += t;
  }
  double suf = incl - tot;   // sum over lanes > l
#pragma unroll
  for (int j = C - 1; j >= 0; --j) {
    const float w = sm[j].alpha * T[j];
    // cumprod backward (as autograd: reverse-cumsum(grad*out)/input) -> dL/dalpha
    const float dalpha = T[j] * v[j] - (float)(suf / (double)sm[j].x);
    suf += (double)w * (double)v[j];
    if (!sm[j].live) continue;
    const float dsig = sm[j].sig > 0.f ? dalpha * sm[j].dist * sm[j].e : 0.f;
    const float dr = gr * w * sm[j].r * (1.f - sm[j].r);
    const float dg = gg * w * sm[j].g * (1.f - sm[j].g);
    const float db = gb * w * sm[j].b * (1.f - sm[j].b);
    float* o = d_raw + (b * S + lane * C + j) * ch;
    if (ch == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(dr, dg, db, dsig);
    } else {
      o[0] = dr; o[1] = dg; o[2] = db; o[3] = dsig;
      for (int c = 4; c < ch; ++c) o[c] = 0.f;
    }
  }
}

template <typename F>
int dispatch_c(int S, F f) {
  const int C = (S + 63) / 64;
  if (C <= 1) return f(std::integral_constant<int, 1>());
  if (C == 2) return f(std::integral_constant<int, 2>());
  if (C == 3) return f(std::integral_constant<int, 3>());
  if (C == 4) return f(std::integral_constant<int, 4>());
  if (C <= 8) return f(std::integral_constant<int, 8>());
  if (C <= 16) return f(std::integral_constant<int, 16>());
  return CNERF_E_UNSUPPORTED;
}

// ---- the host path: every entry point below fills records and goes through launch_fwd / launch_bwd.  Batch = what each starts with;
// cam (the kernel generates the rays: cn_composite_fwd_cam) is the one variation of its check.  An empty batch passes: the plain
// forms answer it with CNERF_OK, the folded losses refuse it themselves.
struct Batch {
  const float* raw; int raw_ch; const float* z; const float* rays; int ray_stride; const float* noise; int64_t B; int S; int white_bkgd;
  bool ok(bool cam = false) const { return raw && z && (cam || (rays && ray_stride >= 6)) && B >= 0 && S > 0 && raw_ch >= 4; }
};
struct FwdOut { float *rgb, *disp, *acc, *depth, *weights; };
struct BwdSeeds { const float *g_rgb, *g_disp, *g_acc, *g_depth; };   // the plain backward's upstream gradients (a folded loss: null)

template <int WV, bool FORMS = false>
int launch_fwd(const Batch& b, const FwdOut& o, const RayGenDev& cam, const MseFwd& m, const ClossFwd& c, hipStream_t st) {
  if (b.B == 0) return CNERF_OK;
  return dispatch_c(b.S, [&](auto cc) -> int {
    constexpr int C = decltype(cc)::value;
    hipLaunchKernelGGL((composite_fwd_k<C, WV, FORMS>), dim3((unsigned)cn_div_up(b.B, WV)), dim3(WV * 64), 0, st, b.raw, b.raw_ch, b.z,
                       b.rays, b.ray_stride, b.noise, b.B, b.S, b.white_bkgd, o.rgb, o.disp, o.acc, o.depth, o.weights, cam, m, c);
    CN_CHECK_LAUNCH();
    return CNERF_OK;
  });
}

template <bool FORMS = false>
int launch_bwd(const Batch& b, const BwdSeeds& g, float* d_raw, const MseBwd& m, const ClossBwd& c, void* stream) {
  if (b.B == 0) return CNERF_OK;
  return dispatch_c(b.S, [&](auto cc) -> int {
    constexpr int C = decltype(cc)::value;
    hipLaunchKernelGGL((composite_bwd_k<C, FORMS>), dim3((unsigned)cn_div_up(b.B, WAVES)), dim3(WAVES * 64), 0, cn_stream(stream),
                       b.raw, b.raw_ch, b.z, b.rays, b.ray_stride, b.noise, b.B, b.S, b.white_bkgd, g.g_rgb, g.g_disp, g.g_acc, g.g_depth,
                       d_raw, m, c);
    CN_CHECK_LAUNCH();
    return CNERF_OK;
  });
}

// cnerf_lossform -> LossForm, or false: cn_lossform_ok's rules (common.hpp), and a softlp form without its exponent, which only
// these launches raise to a power (with_depth: the depth form matters only next to a prior)
bool make_form(const cnerf_lossform* F, bool with_depth, LossForm* f) {
  if (!cn_lossform_ok(F, with_depth)) return false;
  const bool lp = F->rgb_form == CNERF_RGB_SOFTLP || (with_depth && F->depth_form == CNERF_DEPTH_SOFTLP);
  if (lp && !(F->lp_coef > 0.f)) return false;
  f->rgb_form = F->rgb_form; f->depth_form = F->depth_form; f->lp_coef = F->lp_coef; f->temp_rgb = F->temp_rgb;
  f->temp_depth = F->temp_depth;
  return true;
}

// The rules a folded loss adds to Batch::ok, forward and backward alike: rays to sum over, the batch's struct and its target, the
// level's depth map and a far bound next to a prior.  FORMS: one segment only, and a form that make_form takes (-> *f).
template <bool FORMS>
bool closs_ok(const Batch& b, const cnerf_closs* L, const cnerf_lossform* F, const float* depth, LossForm* f) {
  if (!b.ok() || b.B == 0 || !L || !L->target || (L->prior && (!depth || !(L->far > 0.f)))) return false;
  return !FORMS || (L->seg_row == 0 && make_form(F, L->prior != nullptr, f));
}

template <bool FORMS>
int fwd_closs(const Batch& b, const cnerf_closs* L, const cnerf_lossform* F, const FwdOut& o, float* workspace, void* stream) {
  ClossFwd c{};
  if (!closs_ok<FORMS>(b, L, F, o.depth, &c.form) || !o.rgb || !workspace || ((uintptr_t)workspace & 7) != 0) return CNERF_E_ARG;
  c.tgt = L->target; c.mask = L->mask; c.prior = L->prior; c.far = L->far; c.part = reinterpret_cast<double*>(workspace);
  return launch_fwd<MSE_WAVES, FORMS>(b, o, cn_no_raygen(), MseFwd{}, c, cn_stream(stream));
}

// The seeds of a closs backward: what the four entry points pass beyond the batch, in their order.  A group of per-ray seeds covers
// the batch's first n rays (n = 0: no such term); required: the entry point is named after the group (_ssim, _lpips).
struct SeedGroup { const float* d; int64_t n; bool required; };
struct ClossSeeds {
  const cnerf_closs* L;
  const float *rgb, *depth, *stats, *g_loss;      // the level's forward maps, the seed weights of its finish, the upstream gradient
  float rgb_w, depth_w, patch_w;
  SeedGroup patch;
  float ssim_w;
  SeedGroup ssim, lpips;
  const cnerf_lossform* F; float coef; const float* d_temp; float* g_temp;      // _lossform only; the pair: both or neither
};

// A group's rays lie inside the batch, and a required group is there.  strict: a count comes with its seeds — the SSIM and LPIPS
// groups; a patch count without seeds passes and runs without the patch term.
bool group_ok(const SeedGroup& g, int64_t B, bool strict) {
  return g.n >= 0 && g.n <= B && !(g.required && (!g.d || g.n == 0)) && !(strict && g.n > 0 && !g.d);
}

// Every argument rule of a closs backward, once (all of them CNERF_E_ARG; the sample count is the dispatcher's).  Fills *f.
template <bool FORMS>
bool validate(const Batch& b, const ClossSeeds& s, const float* d_raw, LossForm* f) {
  return closs_ok<FORMS>(b, s.L, s.F, s.depth, f) && s.rgb && s.stats && d_raw && group_ok(s.patch, b.B, false) &&
         group_ok(s.ssim, b.B, true) && group_ok(s.lpips, b.B, true) &&
         s.lpips.n % 256 == 0 &&      // whole 16 x 16 patches: the kernel reads cnerf_lpips_bwd's NCHW gradient in place
         (s.d_temp == nullptr) == (s.g_temp == nullptr);
}

void fill(const Batch& b, const ClossSeeds& s, ClossBwd& c) {
  const cnerf_closs& L = *s.L;
  c.rgb = s.rgb; c.depth = s.depth; c.tgt = L.target; c.mask = L.mask; c.prior = L.prior; c.stats = s.stats; c.g = s.g_loss;
  c.seg_row = L.seg_row > 0 && L.seg_row < b.B ? L.seg_row : 0;
  c.far = L.far; c.rgb_w = s.rgb_w; c.depth_w = s.depth_w; c.patch_w = s.patch_w; c.ssim_w = s.ssim_w; c.form.coef = s.coef;
  c.patch_d = s.patch.n > 0 ? s.patch.d : nullptr; c.n_patch = s.patch.n;
  c.ssim_d = s.ssim.n > 0 ? s.ssim.d : nullptr; c.n_ssim = s.ssim.n;
  c.lpips_d = s.lpips.n > 0 ? s.lpips.d : nullptr; c.n_lpips = s.lpips.n;
  c.d_temp = s.d_temp; c.g_temp = s.g_temp;
}

template <bool FORMS = false>
int bwd_closs(const Batch& b, const ClossSeeds& s, float* d_raw, void* stream) {
  ClossBwd c{};
  if (!validate<FORMS>(b, s, d_raw, &c.form)) return CNERF_E_ARG;
  fill(b, s, c);
  return launch_bwd<FORMS>(b, {}, d_raw, MseBwd{}, c, stream);
}
}  // namespace

extern "C" int cnerf_composite_fwd(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride, const float* noise,
                                   int64_t B, int S, int white_bkgd, float* rgb, float* disp, float* acc, float* depth, float* weights,
                                   void* stream) {
  const Batch b{raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd};
  if (!b.ok()) return CNERF_E_ARG;
  return launch_fwd<WAVES>(b, {rgb, disp, acc, depth, weights}, cn_no_raygen(), MseFwd{}, ClossFwd{}, cn_stream(stream));
}

// compositing for the rays of a camera generated in-kernel; used by cnerf_render_fwd_cam
int cn_composite_fwd_cam(const float* raw, int raw_ch, const float* z, const RayGenDev& cam, const float* noise, int64_t B, int S,
                         int white_bkgd, float* rgb, float* disp, float* acc, float* depth, float* weights, hipStream_t st) {
  const Batch b{raw, raw_ch, z, nullptr, 0, noise, B, S, white_bkgd};
  if (!b.ok(true)) return CNERF_E_ARG;
  return launch_fwd<WAVES>(b, {rgb, disp, acc, depth, weights}, cam, MseFwd{}, ClossFwd{}, st);
}

extern "C" int cnerf_composite_bwd(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride, const float* noise,
                                   int64_t B, int S, int white_bkgd, const float* g_rgb, const float* g_disp, const float* g_acc,
                                   const float* g_depth, float* d_raw, void* stream) {
  const Batch b{raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd};
  if (!b.ok() || !d_raw) return CNERF_E_ARG;
  return launch_bwd(b, {g_rgb, g_disp, g_acc, g_depth}, d_raw, MseBwd{}, ClossBwd{}, stream);
}

// ---- compositing with img2mse(rgb_map, target) folded in (R:769-775): see MseFwd / MseBwd above ---------------------------------
extern "C" int64_t cnerf_composite_mse_ws_floats(int64_t B) { return B <= 0 ? 0 : 2 * cn_div_up(B, WAVES) + 2; }
extern "C" int64_t cnerf_composite_mse_counter_words(void) { return MSE_CTR_WORDS; }
extern "C" int64_t cnerf_composite_mse_max_rays(void) { return (int64_t)(MSE_CTR_WORDS / MSE_CTR_STRIDE - 1) * MSE_GROUP * MSE_WAVES; }

extern "C" int cnerf_composite_fwd_mse(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                       const float* noise, int64_t B, int S, int white_bkgd, const float* target,
                                       const float* loss_add, float* rgb, float* disp, float* acc, float* depth, float* weights,
                                       float* loss, float* workspace, unsigned* counter, void* stream) {
  const Batch b{raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd};
  if (!b.ok() || B == 0 || !target || !rgb || !loss || !workspace || !counter || ((uintptr_t)workspace & 7) != 0) return CNERF_E_ARG;
  if (B > cnerf_composite_mse_max_rays()) return CNERF_E_UNSUPPORTED;
  const MseFwd m{target, reinterpret_cast<double*>(workspace), counter, loss, loss_add, 3.0 * (double)B};
  return launch_fwd<MSE_WAVES>(b, {rgb, disp, acc, depth, weights}, cn_no_raygen(), m, ClossFwd{}, cn_stream(stream));
}

extern "C" int cnerf_composite_bwd_mse(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                       const float* noise, int64_t B, int S, int white_bkgd, const float* rgb, const float* target,
                                       const float* g_loss, float* d_raw, void* stream) {
  const Batch b{raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd};
  if (!b.ok() || B == 0 || !rgb || !target || !d_raw) return CNERF_E_ARG;
  return launch_bwd(b, {}, d_raw, MseBwd{rgb, target, g_loss, (float)(2.0 / (3.0 * (double)B))}, ClossBwd{}, stream);
}

// ---- compositing with ConsistentNeRF's masked rgb / depth losses folded in (V:1645-1865): see ClossFwd / ClossBwd above ----------
// ---- and the same with a form per kind of term (cnerf_lossform: the other live loss branches of V / VC) --------------------------
extern "C" int64_t cnerf_closs_ws_floats(int64_t B) { return B <= 0 ? 0 : 2 * LT_MASKED_SLOTS * cn_div_up(B, MSE_WAVES); }
extern "C" int64_t cnerf_lossform_ws_floats(int64_t B) { return B <= 0 ? 0 : 2 * CNERF_LOSSFORM_SLOTS * cn_div_up(B, MSE_WAVES); }

extern "C" int cnerf_composite_fwd_closs(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                         const float* noise, int64_t B, int S, int white_bkgd, const cnerf_closs* L, float* rgb,
                                         float* disp, float* acc, float* depth, float* weights, float* workspace, void* stream) {
  return fwd_closs<false>({raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd}, L, nullptr, {rgb, disp, acc, depth, weights},
                          workspace, stream);
}

extern "C" int cnerf_composite_fwd_lossform(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                            const float* noise, int64_t B, int S, int white_bkgd, const cnerf_closs* L,
                                            const cnerf_lossform* F, float* rgb, float* disp, float* acc, float* depth, float* weights,
                                            float* workspace, void* stream) {
  return fwd_closs<true>({raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd}, L, F, {rgb, disp, acc, depth, weights}, workspace,
                         stream);
}

extern "C" int cnerf_composite_bwd_closs(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                         const float* noise, int64_t B, int S, int white_bkgd, const cnerf_closs* L, const float* rgb,
                                         const float* depth, const float* stats, const float* g_loss, float rgb_w, float depth_w,
                                         float patch_w, const float* patch_d, int64_t n_patch_rays, float* d_raw, void* stream) {
  return bwd_closs({raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd},
                   {L, rgb, depth, stats, g_loss, rgb_w, depth_w, patch_w, {patch_d, n_patch_rays}}, d_raw, stream);
}

extern "C" int cnerf_composite_bwd_closs_ssim(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                              const float* noise, int64_t B, int S, int white_bkgd, const cnerf_closs* L, const float* rgb,
                                              const float* depth, const float* stats, const float* g_loss, float rgb_w, float depth_w,
                                              float patch_w, const float* patch_d, int64_t n_patch_rays, float ssim_w, const float* ssim_d,
                                              int64_t n_ssim_rays, float* d_raw, void* stream) {
  return bwd_closs({raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd},
                   {L, rgb, depth, stats, g_loss, rgb_w, depth_w, patch_w, {patch_d, n_patch_rays}, ssim_w, {ssim_d, n_ssim_rays, true}},
                   d_raw, stream);
}

extern "C" int cnerf_composite_bwd_closs_lpips(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                               const float* noise, int64_t B, int S, int white_bkgd, const cnerf_closs* L, const float* rgb,
                                               const float* depth, const float* stats, const float* g_loss, float rgb_w, float depth_w,
                                               float patch_w, const float* patch_d, int64_t n_patch_rays, float ssim_w, const float* ssim_d,
                                               int64_t n_ssim_rays, const float* lpips_dx, int64_t n_lpips_rays, float* d_raw,
                                               void* stream) {
  return bwd_closs({raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd},
                   {L, rgb, depth, stats, g_loss, rgb_w, depth_w, patch_w, {patch_d, n_patch_rays}, ssim_w, {ssim_d, n_ssim_rays},
                    {lpips_dx, n_lpips_rays, true}}, d_raw, stream);
}

extern "C" int cnerf_composite_bwd_lossform(const float* raw, int raw_ch, const float* z, const float* rays, int ray_stride,
                                            const float* noise, int64_t B, int S, int white_bkgd, const cnerf_closs* L,
                                            const cnerf_lossform* F, const float* rgb, const float* depth, const float* stats8,
                                            const float* g_loss, float rgb_w, float depth_w, float patch_w, float coef,
                                            const float* patch_d, int64_t n_patch_rays, float ssim_w, const float* ssim_d,
                                            int64_t n_ssim_rays, const float* d_temp2, float* g_temp2, float* d_raw, void* stream) {
  return bwd_closs<true>({raw, raw_ch, z, rays, ray_stride, noise, B, S, white_bkgd},
                         {L, rgb, depth, stats8, g_loss, rgb_w, depth_w, patch_w, {patch_d, n_patch_rays}, ssim_w, {ssim_d, n_ssim_rays},
                          /* no LPIPS seeds on the forms */ {}, F, coef, d_temp2, g_temp2}, d_raw, stream);
}
