// Masked photometric / depth losses of ConsistentNeRF (V:1645-1648, V:1737, V:1786-1788, V:1865) and the
// vanilla MSE (R:769), forward value + gradient seeds for the compositing backward in one launch.
// Replaces 4 boolean-index gathers (each a host sync) per level.  One workgroup, fixed reduction order.
#include "common.hpp"
#include "loss_terms.hpp"
#include "ssim.hpp"

namespace {

constexpr int T = 1024;

__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < T / 64; ++i) s += sh[i];
  return s;
}

// ray i of a stand-alone masked-loss launch into the five partials / its gradient seeds: shared by the one-workgroup kernel and the
// two stages of the multi-workgroup form below
__device__ __forceinline__ void masked_accum(double* t, const float* __restrict__ rgb, const float* __restrict__ tgt,
                                             const float* __restrict__ depth, const float* __restrict__ prior,
                                             const float* __restrict__ mask, int64_t i, float far) {
  const float m = mask ? mask[i] : 1.f;
  lt_accum_ray(t, m, lt_sq_err3(rgb + 3 * i, tgt + 3 * i));
  if (depth) lt_accum_depth(t, m, lt_depth_res(depth[i], prior[i], far));
}
__device__ __forceinline__ void masked_seeds(const LtNorm& nm, const float* __restrict__ rgb, const float* __restrict__ tgt,
                                             const float* __restrict__ depth, const float* __restrict__ prior,
                                             const float* __restrict__ mask, int64_t i, float far, float* __restrict__ d_rgb,
                                             float* __restrict__ d_depth) {
  const float m = mask ? mask[i] : 1.f;
  const float w = lt_ray_w(m, nm.w1, nm.w0);
  if (d_rgb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) d_rgb[3 * i + c] = lt_seed_colour(w, rgb[3 * i + c], tgt[3 * i + c]);
  }
  if (d_depth) d_depth[i] = depth ? lt_seed_depth(m, nm.wd, depth[i], prior[i], far) : 0.f;
}

__global__ __launch_bounds__(T) void masked_loss_k(const float* __restrict__ rgb, const float* __restrict__ tgt,
                                                   const float* __restrict__ depth, const float* __restrict__ prior,
                                                   const float* __restrict__ mask, int64_t B, float far, float coef,
                                                   const float* __restrict__ counts, float g_scale,
                                                   float* __restrict__ loss, float* __restrict__ d_rgb,
                                                   float* __restrict__ d_depth) {
  __shared__ double sh[T / 64];
  // pass 1: the five sums (loss_terms.hpp)
  double t[LT_MASKED_SLOTS] = {0, 0, 0, 0, 0};
  for (int64_t i = threadIdx.x; i < B; i += T) masked_accum(t, rgb, tgt, depth, prior, mask, i, far);
  t[LT_N1] = block_sum(t[LT_N1], sh); t[LT_N0] = block_sum(t[LT_N0], sh);
  t[LT_S1] = block_sum(t[LT_S1], sh); t[LT_S0] = block_sum(t[LT_S0], sh); t[LT_SD] = block_sum(t[LT_SD], sh);
  const bool writes = threadIdx.x == 0;
  const LtNorm nm = lt_normalise(t, counts, coef, far, depth != nullptr, g_scale, writes);
  if (writes) { loss[0] = nm.img; loss[1] = nm.dep; }
  for (int64_t i = threadIdx.x; i < B; i += T) masked_seeds(nm, rgb, tgt, depth, prior, mask, i, far, d_rgb, d_depth);
}


// ---- f-5: monocular-depth patch term (V:1678-1720) -------------------------------------------------------------------
// Per patch of n rays: inverse rendered depth pr = nan_to_num(1 / where(d <= 0, 1e-4, d)) and the monocular prior
// gt = nan_to_num(mono) are each min-max normalised over the prior's valid set m = (gt > 0), aligned by the mean
// difference, and the mean squared residual / P / 2 is summed over the P patches.  One wave64 per patch (n = 256 ->
// 4 elements per lane), everything re-read from L1/L2 between the reduction passes; butterfly reductions in a fixed
// order, the P partial losses summed by thread 0.  The backward follows autograd's rules for the same expression:
// full-reduction min()/max() split their gradient evenly over ties, nan_to_num passes it where 1/x is finite,
// d(1/x) = -g (1/x)^2, and nothing flows where d <= 0 (the constant branch of the where()).
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float nan_to_num(float v) {
  if (v != v) return 0.f;
  if (v == INFINITY) return 3.402823466e+38f;
  if (v == -INFINITY) return -3.402823466e+38f;
  return v;
}

// one patch by one wave64: returns (all lanes) the patch's share of the loss, (float)(mean residual^2) / P / 2; writes d_depth[n]
// (the gradient of that share times g_scale) when asked
__device__ __forceinline__ float patch_wave(const float* __restrict__ d, const float* __restrict__ g, int P, int n, float g_scale,
                                            float* __restrict__ d_depth, int lane) {
  auto inv = [&](int i) { const float x = d[i] <= 0.f ? 1e-4f : d[i]; return 1.f / x; };
  // pass 1: ranges
  float gmin = 1e5f, gmax = -INFINITY, pmin = 1e5f, pmax = -INFINITY;
  for (int i = lane; i < n; i += 64) {
    const float gt = nan_to_num(g[i]), pr = nan_to_num(inv(i));
    const float m = gt > 0.f ? 1.f : 0.f;
    gmin = fminf(gmin, gt > 0.f ? gt : 1e5f);
    gmax = fmaxf(gmax, gt);
    pmin = fminf(pmin, m * pr > 0.f ? pr : 1e5f);
    pmax = fmaxf(pmax, m * pr);
  }
  gmin = wave_min(gmin); gmax = wave_max(gmax); pmin = wave_min(pmin); pmax = wave_max(pmax);
  const float rg = gmax - gmin + 1e-4f, r = pmax - pmin + 1e-4f;
  auto gtn = [&](int i) { const float gt = nan_to_num(g[i]); return (gt > 0.f ? 1.f : 0.f) * (gt - gmin) / rg; };
  auto prq = [&](int i) { const float gt = nan_to_num(g[i]); return (gt > 0.f ? 1.f : 0.f) * (nan_to_num(inv(i)) - pmin); };
  // pass 2: shift
  double sd = 0.0;
  for (int i = lane; i < n; i += 64) sd += (double)(prq(i) / r - gtn(i));
  const float alpha = (float)(wave_sum(sd) / n);
  // pass 3: residuals
  double se2 = 0.0, se = 0.0;
  for (int i = lane; i < n; i += 64) {
    const float e = gtn(i) - prq(i) / r + alpha;
    se2 += (double)(e * e); se += (double)e;
  }
  se2 = wave_sum(se2); se = wave_sum(se);
  const float share = (float)(se2 / n) / P / 2;
  if (!d_depth) return share;
  // pass 4: gradient sums.  dL/dprn_i = (mean(e) - e_i) / (n P)
  const float ebar = (float)(se / n), w = g_scale / ((float)n * (float)P);
  double s_mg = 0.0, s_gq = 0.0;
  int cmin = 0, cmax = 0;
  for (int i = lane; i < n; i += 64) {
    const float gt = nan_to_num(g[i]), pr = nan_to_num(inv(i));
    const float m = gt > 0.f ? 1.f : 0.f, q = m * (pr - pmin);
    const float gi = w * (ebar - (gtn(i) - q / r + alpha));
    s_mg += (double)(m * gi); s_gq += (double)(gi * q);
    cmin += ((m * pr > 0.f ? pr : 1e5f) == pmin);
    cmax += (m * pr == pmax);
  }
  s_mg = wave_sum(s_mg); s_gq = wave_sum(s_gq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cmin += __shfl_xor(cmin, o, 64); cmax += __shfl_xor(cmax, o, 64); }
  const float d_r = (float)(-s_gq / ((double)r * (double)r));          // dL/dr
  const float d_pmin = (float)(-s_mg / (double)r) - d_r, d_pmax = d_r;    // r = pmax - pmin + 1e-4
  for (int i = lane; i < n; i += 64) {
    const float gt = nan_to_num(g[i]), c = inv(i), pr = nan_to_num(c);
    const float m = gt > 0.f ? 1.f : 0.f, q = m * (pr - pmin);
    const float gi = w * (ebar - (gtn(i) - q / r + alpha));
    float dpr = m * gi / r;
    if (m * pr > 0.f && pr == pmin) dpr += d_pmin / (float)cmin;
    if (m * pr == pmax) dpr += m * d_pmax / (float)cmax;
    const float dc = (c == c && fabsf(c) != INFINITY) ? dpr : 0.f;     // nan_to_num backward
    const float dx = -dc * c * c;                                      // reciprocal backward
    d_depth[i] = d[i] <= 0.f ? 0.f : dx;
  }
  return share;
}

__global__ void patch_depth_loss_k(const float* __restrict__ depth, const float* __restrict__ mono, int P, int n,
                                   float g_scale, float* __restrict__ loss, float* __restrict__ d_depth) {
  __shared__ float part[16];
  const int p = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float share = patch_wave(depth + (int64_t)p * n, mono + (int64_t)p * n, P, n, g_scale,
                                 d_depth ? d_depth + (int64_t)p * n : nullptr, lane);
  if (lane == 0) part[p] = share;
  __syncthreads();
  if (threadIdx.x == 0) {
    float l = 0.f;
    for (int k = 0; k < P; ++k) l += part[k];
    loss[0] = l;
  }
}

// ---- the loss tail of a ConsistentNeRF step whose masked losses rode in the compositing launches (composite.hip ClossFwd) -------
// ONE workgroup: sums each level's five per-workgroup fp64 partials in index order (thread t takes entries t, t + T, ...; then the
// fixed-order block sum — the value does not depend on the grid's scheduling), normalises with the local or the caller's (global,
// sharded batch) counts with the stand-alone kernels' own lt_normalise (loss_terms.hpp), evaluates the monocular patch term of both levels (one wave per patch: waves
// [0, P) the last level, [P, 2P) the coarse one), assembles the step's loss in the reference's order of accumulation (V:1672-1865:
// loss += w_rgb img_loss; loss += w_patch mono_mse; loss += w_depth depth_loss; then the same three of the coarse level) and leaves
// the per-level seed weights (w1, w0, wd) for cnerf_composite_bwd_closs.
struct ClossTail {
  const double* part[2];     // [5][nparts] per level; level 0 = the last (fine) level, level 1 = coarse or nullptr
  int nparts;
  const float* counts;       // (n1, n0) or nullptr
  float coef, far, rgb_w, depth_w, patch_w;
  int has_depth;
  const float* depth[2];     // depth maps of the levels (patch term), or nullptr
  const float* mono;
  int P, n;
  float* patch_d[2];         // [P * n] per level or nullptr
  float* terms;              // [8]: loss, img_loss, depth_loss, patch_loss, img_loss0, depth_loss0, patch_loss0, -
  float* stats;              // [2][4]: w1, w0, wd, - per level
  int ss;                    // 1: the in-loop consistency step's primary terms (VT:941-969), per-term coins below;
                             // 2: the WHOLE step as one render (cnerf_closs_finish_ss2): partials [0, nparts1) = the primary rays,
                             //    [nparts1, nparts) = the warped rays of the second render (VT:927-938) + padding
  int coin[4];               // rgb, depth, rgb0, depth0: 1 = the term over the selected rays (mask == 1), 0 = the reference's other branch
  int nparts1;               // ss == 2: workgroups of the first segment
  const float* counts3;      // ss == 2: GLOBAL (selected primary rays, primary rays, warped rays) of a batch sharded over ranks, or nullptr
  // V's patch SSIM term (cnerf_closs_finish_ssim; sP = 0: none): waves [0, sP) the last level, [sP, 2 sP) the coarse one, after the
  // depth patch term; terms[8 + level] = ssim_level = (sum_p ssim_p) / 4, loss -= ssim_w ssim_level after the level's patch term
  int sP;
  float ssim_w;
  const float* rgb[2];       // colour maps of the levels [B, 3]
  const float* tgt;          // [B, 3]
  float* ssim_d[2];          // [sP * 768] d ssim_level / d rgb per level, or nullptr
  // V's patch LPIPS term (cnerf_closs_finish_lpips; lP = 0: none): lpips_v[level * lP + p] = the LPIPS value of patch p of the level
  // (one batched cnerf_lpips_fwd over cnerf_lpips_pack_patches' images); terms[10 + level] = lpips_level = (sum_p v_p) / 4,
  // loss += lpips_w lpips_level after the level's SSIM term (V:1726-1728)
  int lP;
  float lpips_w;
  const float* lpips_v;
  // the FORMS tail only (cnerf_lossform_finish): a form per kind of term and level, CNERF_LOSSFORM_SLOTS partials per workgroup
  int rgb_form[2], depth_form[2];
  const float* temp_rgb[2];
  const float* temp_depth[2];
  float* d_temp;             // [2][2]: per level (rgb_w dL_rgb / dt, depth_w dL_depth / dt)
  double B;                  // rays of the batch: the denominator of the norm / plain depth means without global counts
};

// VT:941-969 — the primary render's terms under `--ss_loss`, mask = the rays `[mask_bound][mask]` selects (cnerf_ss_ref_rays'
// `sel`), each term behind its own random.randint(0, 1) coin:
//   img_loss  = coin ? img2mse(rgb[sel], target[sel])      : img2mse(rgb, target)                       (:942)
//   depth     = coin ? img2mse(depth[sel], prior[sel])      : 0                     (un-normalised: far = 1)   (:950-952)
//   img_loss0 = coin ? img2mse(rgb0[sel], target[sel])      : img2mse(rgb, target)  (the FINE rgb: the reference's line :959)
//   depth0    = coin ? img2mse(depth0[sel], prior[sel])     : 0                                          (:966-968)
// accumulated in that order onto `loss` (loss += each), which is returned.  The fallback of :959 sends its gradient to the fine
// level's colours.  fine / coarse = the five sums of the levels' primary rays (coarse = nullptr: one level); N1 / N1c = the
// selected rays the fine / coarse means divide by, Nall = all primary rays; anysel = false: nothing selected, every term takes its
// un-masked branch; the coarse level's seed weights go to stats[st_coarse ..].  Writes terms[1..6] and the primary seed weights.
__device__ __forceinline__ float ss_primary_terms(const ClossTail& a, const double* fine, const double* coarse, double N1, double Nall,
                                                  double N1c, bool anysel, int st_coarse, float loss) {
  const double s1 = fine[LT_S1], s0 = fine[LT_S0];
  const float plain = lt_mean3(s1 + s0, Nall);
  const bool c0 = a.coin[0] && anysel, c2 = a.coin[2] && anysel;
  const float wall = lt_seed_w3(Nall), wsel = anysel ? lt_seed_w3(N1) : 0.f;
  const float il = c0 ? lt_mean3(s1, N1) : plain;
  float w1 = c0 ? wsel : wall, w0 = c0 ? 0.f : wall;
  loss = loss + il;
  float dl = 0.f;
  const bool dep = a.has_depth && a.coin[1] && anysel;
  if (dep) { dl = lt_mean(fine[LT_SD], N1); loss = loss + dl; }
  a.terms[1] = il; a.terms[2] = dl; a.terms[3] = 0.f;
  a.stats[2] = dep ? lt_seed_w(N1) / a.far : 0.f;
  a.stats[3] = 0.f;
  a.terms[4] = a.terms[5] = a.terms[6] = 0.f;
  if (coarse) {
    const float il0 = c2 ? lt_mean3(coarse[LT_S1], N1c) : plain;
    loss = loss + il0;
    float dl0 = 0.f;
    const bool dep0 = a.has_depth && a.coin[3] && anysel;
    if (dep0) { dl0 = lt_mean(coarse[LT_SD], N1c); loss = loss + dl0; }
    a.terms[4] = il0; a.terms[5] = dl0;
    float* st = a.stats + st_coarse;
    st[0] = c2 ? lt_seed_w3(N1c) : 0.f;
    st[1] = 0.f;
    st[2] = dep0 ? lt_seed_w(N1c) / a.far : 0.f;
    st[3] = 0.f;
    if (!c2) { w1 += wall; w0 += wall; }
  }
  a.stats[0] = w1; a.stats[1] = w0;
  return loss;
}

template <bool FORMS>
__global__ __launch_bounds__(T) void closs_tail_k(ClossTail a) {
  constexpr int NS = FORMS ? CNERF_LOSSFORM_SLOTS : LT_MASKED_SLOTS;
  __shared__ double sh[T / 64];
  __shared__ float pshare[2][8];
  __shared__ double tot[2][NS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int levels = a.part[1] ? 2 : 1;
  for (int lv = 0; lv < levels; ++lv)
    for (int k = 0; k < NS; ++k) {
      double s = 0.0;
      for (int i = threadIdx.x; i < a.nparts; i += T) s += a.part[lv][(int64_t)k * a.nparts + i];
      s = block_sum(s, sh);
      if (threadIdx.x == 0) tot[lv][k] = s;
    }
  if (a.P > 0 && wv < levels * a.P) {
    const int lv = wv / a.P, p = wv - lv * a.P;
    const float share = patch_wave(a.depth[lv] + (int64_t)p * a.n, a.mono + (int64_t)p * a.n, a.P, a.n, 1.f,
                                   a.patch_d[lv] ? a.patch_d[lv] + (int64_t)p * a.n : nullptr, lane);
    if (lane == 0) pshare[lv][p] = share;
  }
  __shared__ float sshare[2][8];
  if (a.sP > 0 && wv < levels * a.sP) {
    const int lv = wv / a.sP, p = wv - lv * a.sP;
    const int64_t off = (int64_t)p * CN_PATCH_SSIM_RAYS * 3;
    const float share = cn_patch_ssim_wave(a.rgb[lv] + off, a.tgt + off, CN_PATCH_SSIM_SCALE, a.ssim_d[lv] ? a.ssim_d[lv] + off : nullptr,
                                           lane);
    if (lane == 0) sshare[lv][p] = share;
  }
  if (!FORMS && a.ss == 2) {
    // The one-render form of the whole `--ss_loss` step (VT:899-969): rays [0, 8 nparts1) are the primary batch (mask = sel, prior =
    // depth_cas_s), rays from there on the second render's warped rays (mask = 1 on the live rows, 0 on the padding; target / prior =
    // the reference view's colours / depth prior at the snapped pixels).  Segment sums in index order, like the sums above.
    __shared__ double seg[2][2][LT_MASKED_SLOTS];
    for (int lv = 0; lv < levels; ++lv)
      for (int sg = 0; sg < 2; ++sg)
        for (int k = 0; k < LT_MASKED_SLOTS; ++k) {
          const int lo = sg ? a.nparts1 : 0, hi = sg ? a.nparts : a.nparts1;
          double s = 0.0;
          for (int i = lo + (int)threadIdx.x; i < hi; i += T) s += a.part[lv][(int64_t)k * a.nparts + i];
          s = block_sum(s, sh);
          if (threadIdx.x == 0) seg[lv][sg][k] = s;
        }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // second render first, as the reference accumulates (VT:930-938): img2mse(rgb_ref, target_ref) [+ img2mse(depth_ref, prior_ref)]
    // then the coarse level's two; then the primary render's four coin-gated terms (VT:941-969, ss_primary_terms)
    const double M = a.counts3 ? (double)a.counts3[2] : seg[0][1][LT_N1];
    float loss = 0.f;
    float ref_t[4] = {0.f, 0.f, 0.f, 0.f};
    // M == 0 (no point of the batch projects into the reference view; the reference's `while mask.sum() == 0` never ends there, and the
    // two-render route raises): the second render has no rays — its terms and seed weights are 0 instead of 0 / 0, terms[7] = 0 tells
    // the caller, and with no in-bounds ray `sel` is empty too: the primary terms below fall to their un-masked branch.
    const bool have2 = M > 0.0;
    for (int lv = 0; lv < levels; ++lv) {          // level 0 = the last (fine) level: its terms come first in the reference
      const float il = have2 ? lt_mean3(seg[lv][1][LT_S1], M) : 0.f;
      loss = loss + il;
      ref_t[2 * lv] = il;
      float dl = 0.f;
      if (a.has_depth && have2) { dl = lt_mean(seg[lv][1][LT_SD], M); loss = loss + dl; }
      ref_t[2 * lv + 1] = dl;
      float* st = a.stats + 8 * lv + 4;            // segment 2 of this level: live rows weigh 2 / (3 M) and 2 / M, padding rows 0
      st[0] = have2 ? lt_seed_w3(M) : 0.f; st[1] = 0.f;
      st[2] = (a.has_depth && have2) ? lt_seed_w(M) / a.far : 0.f; st[3] = 0.f;
    }
    // the primary segment's own counts or the global ones; the coarse level's means divide by the same N1.  N1 == 0 only with
    // M == 0 (see above): the coins then have nothing to select
    const double N1 = a.counts3 ? (double)a.counts3[0] : seg[0][0][LT_N1];
    const double Nall = a.counts3 ? (double)a.counts3[1] : seg[0][0][LT_N1] + seg[0][0][LT_N0];
    a.terms[0] = ss_primary_terms(a, seg[0][0], levels == 2 ? seg[1][0] : nullptr, N1, Nall, N1, N1 > 0.0, 8, loss);
    a.terms[7] = (float)M;
    a.terms[8] = ref_t[0]; a.terms[9] = ref_t[1]; a.terms[10] = ref_t[2]; a.terms[11] = ref_t[3];
    return;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!FORMS && a.ss) {
    // the primary terms alone (the second render has launches of its own): each level's own count of selected rays, and no guard
    // for an empty selection
    a.terms[0] = ss_primary_terms(a, tot[0], levels == 2 ? tot[1] : nullptr, tot[0][LT_N1], tot[0][LT_N1] + tot[0][LT_N0],
                                  levels == 2 ? tot[1][LT_N1] : 0.0, true, 4, 0.f);
    a.terms[7] = 0.f;
    return;
  }
  float loss = 0.f;
  for (int lv = 0; lv < levels; ++lv) {
    // the v6 terms and seed weights (g_scale = 1: the upstream gradient joins in the compositing backward); the forms override
    const LtNorm nm = lt_normalise(tot[lv], a.counts, a.coef, a.far, a.has_depth != 0, 1.f, true);
    const double sd = tot[lv][LT_SD], N1 = nm.N1, N0 = nm.N0;
    float il = nm.img, dl = nm.dep;
    float wd = nm.wd, wd0 = 0.f, inv_rgb = 0.f;
    if constexpr (FORMS) {
      float dt_rgb = 0.f, dt_depth = 0.f;
      if (a.rgb_form[lv] != CNERF_RGB_HARDMASK) {
        const double Dn = tot[lv][LT_C_W], N = tot[lv][LT_C_WD2];
        il = (float)(N / Dn);
        inv_rgb = (float)(1.0 / Dn);
        if (a.rgb_form[lv] == CNERF_RGB_SOFTMASK)
          dt_rgb = a.rgb_w * (float)lt_softmask_dtemp(tot[lv][LT_C_WD4], Dn, N, (double)a.temp_rgb[lv][0]);
      }
      if (a.has_depth && a.depth_form[lv] != CNERF_DEPTH_HARDMASK) {
        const int df = a.depth_form[lv];
        if (df == CNERF_DEPTH_HARDMASK_COEF) {
          if (N0 > 0) { dl += a.coef * (float)(tot[lv][LT_D_W] / N0); wd0 = (float)(2.0 / N0); }
          wd = (float)(2.0 / N1);
        } else if (df == CNERF_DEPTH_NORM || df == CNERF_DEPTH_PLAIN) {
          const double Nall = a.counts ? (double)a.counts[0] + (double)a.counts[1] : a.B;
          dl = (float)(sd / Nall);
          wd = (float)(2.0 / Nall);
        } else {
          const double Dn = tot[lv][LT_D_W], N = tot[lv][LT_D_WD2];
          dl = (float)(N / Dn);
          wd = (float)(1.0 / Dn);
          if (df == CNERF_DEPTH_SOFTMASK) dt_depth = a.depth_w * (float)lt_softmask_dtemp(sd, Dn, N, (double)a.temp_depth[lv][0]);
        }
      }
      a.d_temp[2 * lv + 0] = dt_rgb; a.d_temp[2 * lv + 1] = dt_depth;
    }
    float pl = 0.f;
    for (int k = 0; k < a.P; ++k) pl += pshare[lv][k];
    loss += a.rgb_w * il;
    if (a.P > 0) loss += a.patch_w * pl;
    if (a.sP > 0) {
      float sl = 0.f;
      for (int k = 0; k < a.sP; ++k) sl += sshare[lv][k];
      sl = sl / 4.f;
      loss = loss - a.ssim_w * sl;
      a.terms[8 + lv] = sl;
    }
    if (!FORMS && a.lP > 0) {
      float ll = 0.f;
      for (int k = 0; k < a.lP; ++k) ll += a.lpips_v[lv * a.lP + k];
      ll = ll / 4.f;
      loss = loss + a.lpips_w * ll;
      a.terms[10 + lv] = ll;
    }
    if (a.has_depth) loss = loss + a.depth_w * dl;
    a.terms[1 + 3 * lv] = il; a.terms[2 + 3 * lv] = dl; a.terms[3 + 3 * lv] = pl;
    float* st = a.stats + (FORMS ? 8 : 4) * lv;
    st[0] = nm.w1;
    st[1] = nm.w0;
    st[2] = wd;
    st[3] = wd0;
    if constexpr (FORMS) { st[4] = inv_rgb; st[5] = st[6] = st[7] = 0.f; }
  }
  if (FORMS && levels == 1) {
    for (int k = 8; k < 16; ++k) a.stats[k] = 0.f;
    a.d_temp[2] = a.d_temp[3] = 0.f;
  }
  if (FORMS && a.sP == 0) a.terms[8] = a.terms[9] = 0.f;
  if (levels == 1) { a.terms[4] = a.terms[5] = a.terms[6] = 0.f; }
  if (a.sP > 0 && levels == 1) a.terms[9] = 0.f;
  if (!FORMS && a.lP > 0) {
    if (a.sP == 0) a.terms[8] = a.terms[9] = 0.f;
    if (levels == 1) a.terms[11] = 0.f;
  }
  a.terms[0] = loss;
  a.terms[7] = 0.f;
}

}  // namespace

// img2mse (H:9): loss = mean((x - y)^2) over n elements + the gradient seed 2 (x - y) / n, one launch (replaces ATen's
// sub, pow, mean and their three backward kernels).  One workgroup, fixed order, fp64 accumulation.
namespace {
__global__ __launch_bounds__(T) void mse_k(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                           float* __restrict__ loss, float* __restrict__ d_x) {
  __shared__ double sh[T / 64];
  double s = 0;
  const float w = (float)(2.0 / (double)n);
  for (int64_t i = threadIdx.x; i < n; i += T) {
    const float d = x[i] - y[i];
    s += (double)(d * d);
    if (d_x) d_x[i] = w * d;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}
}  // namespace

extern "C" int cnerf_mse(const float* x, const float* y, int64_t n, float* loss, float* d_x, void* stream) {
  if (!x || !y || !loss || n <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(mse_k, dim3(1), dim3(T), 0, cn_stream(stream), x, y, n, loss, d_x);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// img2mse_softLpmask (V:58; the `--softLpmask` branch of the loss, V:1663-1664 / V:1760-1761): every squared residual weighted by
// w = |d|^coef + 1, normalised by the DETACHED sum of the weights:  loss = sum(w d^2) / sum(w).  Gradient w.r.t. x (the denominator
// carries none): (dw/dd d^2 + 2 w d) / sum(w) with dw/dd = coef |d|^(coef - 1) sign(d)  ->  d (coef |d|^coef + 2 w) / sum(w).
// One workgroup, two sweeps (sums in fp64, fixed order), value + gradient seed in one launch like mse_k.
namespace {
__global__ __launch_bounds__(T) void soft_lp_k(const float* __restrict__ x, const float* __restrict__ y, int64_t n, float coef,
                                               float* __restrict__ loss, float* __restrict__ d_x) {
  __shared__ double sh[T / 64];
  __shared__ double tot[2];
  double num = 0, den = 0;
  double unused = 0;
  for (int64_t i = threadIdx.x; i < n; i += T) lt_soft_sums(false, x[i] - y[i], coef, 1.f, den, num, unused);
  num = block_sum(num, sh);
  den = block_sum(den, sh);
  if (threadIdx.x == 0) { tot[0] = num; tot[1] = den; loss[0] = (float)(num / den); }
  __syncthreads();
  if (!d_x) return;
  const float inv = (float)(1.0 / tot[1]);
  for (int64_t i = threadIdx.x; i < n; i += T) d_x[i] = lt_soft_seed(false, x[i] - y[i], coef, 1.f, inv);
}
}  // namespace

extern "C" int cnerf_soft_lp_loss(const float* x, const float* y, int64_t n, float coef, float* loss, float* d_x, void* stream) {
  if (!x || !y || !loss || n <= 0 || !(coef > 0.f)) return CNERF_E_ARG;
  hipLaunchKernelGGL(soft_lp_k, dim3(1), dim3(T), 0, cn_stream(stream), x, y, n, coef, loss, d_x);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// Large inputs (whole images: img2mse of a rendered 756 x 1008 frame is 2.3 M elements): one workgroup per MSE_CHUNK elements writes
// its fp64 partial, a second single-workgroup stage sums the partials in index order — the value does not depend on the grid the
// first stage ran on or on the order its workgroups finished in.
namespace {
constexpr int64_t MSE_CHUNK = 16384;
__global__ __launch_bounds__(T) void mse_part_k(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                double* __restrict__ part, float* __restrict__ d_x) {
  __shared__ double sh[T / 64];
  const int64_t lo = (int64_t)blockIdx.x * MSE_CHUNK, hi = lo + MSE_CHUNK < n ? lo + MSE_CHUNK : n;
  const float w = (float)(2.0 / (double)n);
  double s = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += T) {
    const float d = x[i] - y[i];
    s += (double)(d * d);
    if (d_x) d_x[i] = w * d;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(T) void mse_fin_k(const double* __restrict__ part, int64_t nparts, int64_t n, float* __restrict__ loss) {
  __shared__ double sh[T / 64];
  double s = 0;
  for (int64_t i = threadIdx.x; i < nparts; i += T) s += part[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}
}  // namespace

extern "C" int64_t cnerf_mse_ws_floats(int64_t n) { return n <= 0 ? 0 : 2 * ((n + MSE_CHUNK - 1) / MSE_CHUNK); }

extern "C" int cnerf_mse_ws(const float* x, const float* y, int64_t n, float* loss, float* d_x, float* workspace, void* stream) {
  if (!x || !y || !loss || n <= 0) return CNERF_E_ARG;
  if (!workspace || n <= MSE_CHUNK) return cnerf_mse(x, y, n, loss, d_x, stream);
  if (((uintptr_t)workspace & 7) != 0) return CNERF_E_ARG;      // fp64 partials
  const int64_t nparts = (n + MSE_CHUNK - 1) / MSE_CHUNK;
  hipLaunchKernelGGL(mse_part_k, dim3((unsigned)nparts), dim3(T), 0, cn_stream(stream), x, y, n, reinterpret_cast<double*>(workspace),
                     d_x);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mse_fin_k, dim3(1), dim3(T), 0, cn_stream(stream), reinterpret_cast<const double*>(workspace), nparts, n, loss);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// Large batches (whole images through the masked losses: evaluation, or a caller that does not shard): stage 1 — one workgroup per
// ML_CHUNK rays leaves its five fp64 partials; stage 2 — the same grid: every workgroup sums ALL partials in index order (a few
// hundred doubles: cheaper than a third launch), workgroup 0 writes the loss, each writes the gradient seeds of its own chunk.
// Fixed order at both stages: the value does not depend on scheduling.
namespace {
constexpr int64_t ML_CHUNK = 16384;
constexpr int64_t ML_MAX_PARTS = 1024;
__global__ __launch_bounds__(T) void masked_part_k(const float* __restrict__ rgb, const float* __restrict__ tgt,
                                                   const float* __restrict__ depth, const float* __restrict__ prior,
                                                   const float* __restrict__ mask, int64_t B, float far, double* __restrict__ part) {
  __shared__ double sh[T / 64];
  const int64_t lo = (int64_t)blockIdx.x * ML_CHUNK, hi = lo + ML_CHUNK < B ? lo + ML_CHUNK : B;
  double t[LT_MASKED_SLOTS] = {0, 0, 0, 0, 0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += T) masked_accum(t, rgb, tgt, depth, prior, mask, i, far);
  t[LT_N1] = block_sum(t[LT_N1], sh); t[LT_N0] = block_sum(t[LT_N0], sh);
  t[LT_S1] = block_sum(t[LT_S1], sh); t[LT_S0] = block_sum(t[LT_S0], sh); t[LT_SD] = block_sum(t[LT_SD], sh);
  if (threadIdx.x == 0) {
    double* o = part + LT_MASKED_SLOTS * (int64_t)blockIdx.x;
    for (int k = 0; k < LT_MASKED_SLOTS; ++k) o[k] = t[k];
  }
}
__global__ __launch_bounds__(T) void masked_fin_k(const float* __restrict__ rgb, const float* __restrict__ tgt,
                                                  const float* __restrict__ depth, const float* __restrict__ prior,
                                                  const float* __restrict__ mask, int64_t B, float far, float coef,
                                                  const float* __restrict__ counts, float g_scale, const double* __restrict__ part,
                                                  float* __restrict__ loss, float* __restrict__ d_rgb, float* __restrict__ d_depth) {
  double t[LT_MASKED_SLOTS] = {0, 0, 0, 0, 0};
  for (unsigned p = 0; p < gridDim.x; ++p)
    for (int k = 0; k < LT_MASKED_SLOTS; ++k) t[k] += part[LT_MASKED_SLOTS * (int64_t)p + k];
  const bool writes = blockIdx.x == 0 && threadIdx.x == 0;
  const LtNorm nm = lt_normalise(t, counts, coef, far, depth != nullptr, g_scale, writes);
  if (writes) { loss[0] = nm.img; loss[1] = nm.dep; }
  const int64_t lo = (int64_t)blockIdx.x * ML_CHUNK, hi = lo + ML_CHUNK < B ? lo + ML_CHUNK : B;
  for (int64_t i = lo + threadIdx.x; i < hi; i += T) masked_seeds(nm, rgb, tgt, depth, prior, mask, i, far, d_rgb, d_depth);
}
}  // namespace

extern "C" int64_t cnerf_loss_ws_floats(void) { return 2 * LT_MASKED_SLOTS * ML_MAX_PARTS; }

extern "C" int cnerf_masked_loss(const float* rgb, const float* target, const float* depth, const float* prior,
                                 const float* mask, int64_t B, float far, float coef, const float* counts,
                                 float g_scale, float* loss, float* d_rgb, float* d_depth, float* workspace,
                                 void* stream) {
  if (!rgb || !target || !loss || B <= 0 || (depth && !prior) || !(far > 0.f) || ((uintptr_t)workspace & 7) != 0) return CNERF_E_ARG;
  const int64_t nparts = (B + ML_CHUNK - 1) / ML_CHUNK;
  if (workspace && nparts > 1 && nparts <= ML_MAX_PARTS) {
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(masked_part_k, dim3((unsigned)nparts), dim3(T), 0, cn_stream(stream), rgb, target, depth, prior, mask, B, far,
                       part);
    CN_CHECK_LAUNCH();
    hipLaunchKernelGGL(masked_fin_k, dim3((unsigned)nparts), dim3(T), 0, cn_stream(stream), rgb, target, depth, prior, mask, B, far,
                       coef, counts, g_scale, part, loss, d_rgb, d_depth);
    CN_CHECK_LAUNCH();
    return CNERF_OK;
  }
  hipLaunchKernelGGL(masked_loss_k, dim3(1), dim3(T), 0, cn_stream(stream), rgb, target, depth, prior, mask, B, far,
                     coef, counts, g_scale, loss, d_rgb, d_depth);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_patch_depth_loss(const float* depth_pred, const float* mono, int P, int n, float g_scale,
                                      float* loss, float* d_depth, void* stream) {
  if (!depth_pred || !mono || !loss || P <= 0 || P > 16 || n <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(patch_depth_loss_k, dim3(1), dim3(64 * P), 0, cn_stream(stream), depth_pred, mono, P, n, g_scale,
                     loss, d_depth);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

// ---- the host path of the loss tail: each of the six entry points fills a Finish and goes through finish() ----------------------
namespace {
struct Finish {
  const cnerf_closs_sum* t;
  float *terms, *stats, *patch_d;
  struct Ssim {       // V's patch SSIM term: P patches of 16 x 16 rays = the batch's first P * 256 rays (P = 0: none)
    int P; float w; const float *rgb_last, *rgb_coarse, *target; float* d; bool required;
  } ssim;
  // V's patch LPIPS term next to it: v = the [levels P] per-image values of the one batched LPIPS forward over the levels' patches
  struct Lpips { bool on; int P; float w; const float* v; } lpips;      // (cnerf_lpips_pack_patches' order: the last level's first)
  struct Forms { bool on; const cnerf_lossform* F[2]; float* d_temp; } forms;      // cnerf_lossform_finish: a form per level
  int ss;             // the in-loop consistency step: 1 = its primary terms (coins), 2 = the whole step as one render (+ seg_row, counts3)
  const int32_t* coins;
  int64_t seg_row;
  const float* counts3;
};

// Every argument rule of the tail, once; all of them are CNERF_E_ARG.
bool validate(const Finish& f) {
  const cnerf_closs_sum* t = f.t;
  if (!t || !f.terms || !f.stats || !t->ws_last || t->B <= 0 || ((uintptr_t)t->ws_last & 7) != 0 || ((uintptr_t)t->ws_coarse & 7) != 0 ||
      (t->has_depth && !(t->far > 0.f)))
    return false;
  // the depth patch term: P patches of n rays inside the batch, with the monocular depths and every level's depth map
  if (t->P < 0 || t->P > 8 || (int64_t)t->P * t->n > t->B) return false;
  if (t->P > 0 && (t->n <= 0 || !t->mono || !t->depth_last || (t->ws_coarse && !t->depth_coarse))) return false;
  const Finish::Ssim& s = f.ssim;
  if (s.P < 0 || s.P > 8 || (s.required && s.P == 0)) return false;
  if (s.P > 0 && (!s.rgb_last || !s.target || (int64_t)s.P * CN_PATCH_SSIM_RAYS > t->B || (t->ws_coarse && !s.rgb_coarse))) return false;
  const Finish::Lpips& l = f.lpips;
  if (l.on && (!l.v || l.P <= 0 || l.P > 8 || (int64_t)l.P * CN_PATCH_SSIM_RAYS > t->B)) return false;
  if (f.forms.on) {
    // (no in-loop consistency segments here; a softlp / softmask normaliser is a sum of weights, which no caller all-reduces: no
    // global counts with those forms)
    if (f.ss || f.seg_row != 0 || !f.forms.d_temp) return false;
    for (int lv = 0; lv < (t->ws_coarse ? 2 : 1); ++lv) {
      const cnerf_lossform* F = f.forms.F[lv];
      if (!cn_lossform_ok(F, t->has_depth != 0)) return false;
      const bool soft = F->rgb_form != CNERF_RGB_HARDMASK || (t->has_depth && F->depth_form >= CNERF_DEPTH_SOFTLP);
      if (soft && t->counts) return false;
    }
  }
  // ss: the reference's block has neither a patch term nor sharded (n1, n0).  ss == 2: ONE batch of t->B rays = [primary | warped +
  // padding] cut at seg_row, a multiple of the 8 rays of a compositing workgroup, so that every partial belongs to one segment
  if (f.ss && (!f.coins || t->P != 0 || t->counts)) return false;
  return f.ss != 2 || (f.seg_row > 0 && f.seg_row < t->B && f.seg_row % CN_CLOSS_RAYS_PER_WG == 0);
}

// The kernel's arguments of a validated call: the partials' count and cut, the coarse level's slices of patch_d and ssim_d, and
// far = 1 without a depth term.  What a term that is off would read stays null / 0.
void fill(const Finish& f, ClossTail& a) {
  const cnerf_closs_sum& t = *f.t;
  const Finish::Ssim& s = f.ssim;
  a.part[0] = reinterpret_cast<const double*>(t.ws_last);
  a.part[1] = reinterpret_cast<const double*>(t.ws_coarse);
  a.nparts = (int)cn_div_up(t.B, (int64_t)CN_CLOSS_RAYS_PER_WG);
  a.nparts1 = (int)(f.seg_row / CN_CLOSS_RAYS_PER_WG);
  a.counts = t.counts; a.counts3 = f.counts3; a.coef = t.coef; a.far = t.has_depth ? t.far : 1.f; a.has_depth = t.has_depth;
  a.rgb_w = t.rgb_w; a.depth_w = t.depth_w; a.patch_w = t.patch_w;
  a.depth[0] = t.depth_last; a.depth[1] = t.depth_coarse; a.mono = t.mono; a.P = t.P; a.n = t.n;
  a.patch_d[0] = (f.patch_d && t.P > 0) ? f.patch_d : nullptr;
  a.patch_d[1] = (a.patch_d[0] && t.ws_coarse) ? f.patch_d + (int64_t)t.P * t.n : nullptr;
  a.terms = f.terms; a.stats = f.stats; a.ss = f.ss;
  for (int k = 0; k < 4; ++k) a.coin[k] = f.ss ? (f.coins[k] != 0) : 0;
  if (s.P > 0) {
    a.sP = s.P; a.ssim_w = s.w; a.rgb[0] = s.rgb_last; a.rgb[1] = t.ws_coarse ? s.rgb_coarse : nullptr; a.tgt = s.target;
    a.ssim_d[0] = s.d;
    a.ssim_d[1] = (s.d && t.ws_coarse) ? s.d + (int64_t)s.P * CN_PATCH_SSIM_RAYS * 3 : nullptr;
  }
  a.lP = f.lpips.P; a.lpips_w = f.lpips.w; a.lpips_v = f.lpips.v;
  for (int lv = 0; f.forms.on && lv < (t.ws_coarse ? 2 : 1); ++lv) {
    const cnerf_lossform& F = *f.forms.F[lv];
    a.rgb_form[lv] = F.rgb_form; a.depth_form[lv] = F.depth_form; a.temp_rgb[lv] = F.temp_rgb; a.temp_depth[lv] = F.temp_depth;
  }
  a.d_temp = f.forms.d_temp; a.B = (double)t.B;
}

int finish(const Finish& f, void* stream) {
  if (!validate(f)) return CNERF_E_ARG;
  ClossTail a{};
  fill(f, a);
  hipLaunchKernelGGL(f.forms.on ? closs_tail_k<true> : closs_tail_k<false>, dim3(1), dim3(T), 0, cn_stream(stream), a);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
}  // namespace

extern "C" int cnerf_closs_finish(const cnerf_closs_sum* t, float* terms, float* stats, float* patch_d, void* stream) {
  return finish({t, terms, stats, patch_d}, stream);
}

extern "C" int cnerf_closs_finish_ss(const cnerf_closs_sum* t, const int32_t* coins4, float* terms, float* stats, void* stream) {
  return finish({t, terms, stats, nullptr, {}, {}, {}, 1, coins4}, stream);
}

extern "C" int cnerf_closs_finish_ss2(const cnerf_closs_sum* t, const int32_t* coins4, int64_t seg_row, const float* counts3,
                                      float* terms12, float* stats16, void* stream) {
  return finish({t, terms12, stats16, nullptr, {}, {}, {}, 2, coins4, seg_row, counts3}, stream);
}

extern "C" int cnerf_closs_finish_ssim(const cnerf_closs_sum* t, int ssim_P, float ssim_w, const float* rgb_last, const float* rgb_coarse,
                                       const float* target, float* terms10, float* stats, float* patch_d, float* ssim_d, void* stream) {
  return finish({t, terms10, stats, patch_d, {ssim_P, ssim_w, rgb_last, rgb_coarse, target, ssim_d, true}}, stream);
}

extern "C" int cnerf_closs_finish_lpips(const cnerf_closs_sum* t, int ssim_P, float ssim_w, const float* rgb_last, const float* rgb_coarse,
                                        const float* target, int lpips_P, float lpips_w, const float* lpips_v, float* terms12, float* stats,
                                        float* patch_d, float* ssim_d, void* stream) {
  return finish({t, terms12, stats, patch_d, {ssim_P, ssim_w, rgb_last, rgb_coarse, target, ssim_d}, {true, lpips_P, lpips_w, lpips_v}},
                stream);
}

extern "C" int cnerf_lossform_finish(const cnerf_closs_sum* t, const cnerf_lossform* F_last, const cnerf_lossform* F_coarse, int ssim_P,
                                     float ssim_w, const float* rgb_last, const float* rgb_coarse, const float* target, float* terms10,
                                     float* stats16, float* patch_d, float* ssim_d, float* d_temp4, void* stream) {
  return finish({t, terms10, stats16, patch_d, {ssim_P, ssim_w, rgb_last, rgb_coarse, target, ssim_d}, {},
                 {true, {F_last, F_coarse}, d_temp4}}, stream);
}

// img2mse_softmask / img2mse_depth_softmask (V:50 / V:55; the `--softmask` branch of the loss, VC:1526-1528 / VC:1564-1572): every
// squared residual weighted by w = exp(d^2 / t), normalised by the sum of the weights, which is detached in d but NOT in the
// temperature:  L = N / Dn, N = sum(w d^2), Dn = sum(w);  dL / dd = w (2 d + 2 d^3 / t) / Dn;  dL / dt = -(sum(w d^4) / Dn - L^2) / t^2.
// One workgroup, two sweeps (sums in fp64, fixed order), like soft_lp_k.
namespace {
__global__ __launch_bounds__(T) void softmask_k(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                const float* __restrict__ temp, float* __restrict__ loss, float* __restrict__ d_x,
                                                float* __restrict__ d_temp) {
  __shared__ double sh[T / 64];
  __shared__ double tot[1];
  const float t = temp[0];
  double num = 0, den = 0, s4 = 0;
  for (int64_t i = threadIdx.x; i < n; i += T) lt_soft_sums(true, x[i] - y[i], 0.f, t, den, num, s4);
  num = block_sum(num, sh);
  den = block_sum(den, sh);
  s4 = block_sum(s4, sh);
  if (threadIdx.x == 0) {
    const double L = num / den;
    tot[0] = den;
    loss[0] = (float)L;
    if (d_temp) d_temp[0] = (float)lt_softmask_dtemp(s4, den, num, (double)t);
  }
  __syncthreads();
  if (!d_x) return;
  const float inv = (float)(1.0 / tot[0]);
  for (int64_t i = threadIdx.x; i < n; i += T) d_x[i] = lt_soft_seed(true, x[i] - y[i], 0.f, t, inv);
}
}  // namespace

extern "C" int cnerf_softmask_loss(const float* x, const float* y, int64_t n, const float* temp, float* loss, float* d_x, float* d_temp,
                                   void* stream) {
  if (!x || !y || !temp || !loss || n <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(softmask_k, dim3(1), dim3(T), 0, cn_stream(stream), x, y, n, temp, loss, d_x, d_temp);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
