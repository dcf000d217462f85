// cnerf_render_fwd / cnerf_render_bwd: render_rays (R:311-421, V:441-551) and its autograd as ONE call each — the
// launch sequence the Python surface drives (run_nerf.py::render_rays), for callers that bind the C ABI directly:
//   coarse_z -> [gamma + MLP](coarse) -> composite -> (Nf > 0:) resample -> [gamma + MLP](fine) -> composite
// and backwards  composite_bwd -> dgrad -> wgrad  per level (no gradient through the resampling, R:397).
// Host code only: every launch goes through the public entry points of this library, on the caller's stream, inside
// the caller's workspace; nothing is allocated and nothing synchronises.
#include "raygen.hpp"

namespace {

struct Layout {            // float offsets into the workspace
  int64_t z0, raw0, w0;    // coarse level: z[B,Nc], raw[B,Nc,C0], weights[B,Nc]
  int64_t z1, raw1, w1;    // fine level (Nf > 0): z[B,S1], raw[B,S1,C1], weights[B,S1]
  int64_t stash0, stash1;  // training stashes
  int64_t d_raw, bwd;      // backward scratch: d_raw of the coarse level, cnerf_mlp_bwd workspace of the coarse level
  int64_t d_raw1, bwd1;    // ... of the fine level (both levels are in flight together: cnerf_mlp_bwd_pair)
  int64_t total;
  int C0, C1, S1;
};

int raw_channels(const cnerf_net* n) { return n->use_viewdirs ? 4 : n->output_ch; }

int make_layout(const cnerf_net* coarse, const cnerf_net* fine, const cnerf_render_cfg* cfg, int64_t B, Layout* L) {
  if (!coarse || !cfg || B < 0 || cfg->Nc <= 0 || cfg->Nf < 0 || (cfg->ray_stride != 8 && cfg->ray_stride != 11))
    return CNERF_E_ARG;
  const cnerf_net* n1 = fine ? fine : coarse;      // R:402: the coarse network serves both levels when there is no fine one
  if ((coarse->use_viewdirs || n1->use_viewdirs) && cfg->ray_stride != 11) return CNERF_E_ARG;
  const int64_t Nc = cfg->Nc, S1 = cfg->Nc + cfg->Nf;
  L->C0 = raw_channels(coarse); L->C1 = raw_channels(n1); L->S1 = (int)S1;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t at = o; o += cn_round_up(n, 64); return at; };
  L->z0 = take(B * Nc); L->raw0 = take(B * Nc * L->C0); L->w0 = take(B * Nc);
  L->z1 = L->raw1 = L->w1 = L->stash0 = L->stash1 = -1;
  if (cfg->Nf > 0) { L->z1 = take(B * S1); L->raw1 = take(B * S1 * L->C1); L->w1 = take(B * S1); }
  L->d_raw = L->bwd = L->d_raw1 = L->bwd1 = -1;
  if (cfg->train) {
    L->stash0 = take(cnerf_mlp_stash_floats(coarse, B * Nc));
    if (cfg->Nf > 0) L->stash1 = take(cnerf_mlp_stash_floats(n1, B * S1));
    L->d_raw = take(B * Nc * L->C0);
    L->bwd = take(cnerf_mlp_bwd_ws_floats(coarse, B * Nc));
    if (cfg->Nf > 0) {
      L->d_raw1 = take(B * S1 * L->C1);
      L->bwd1 = take(cnerf_mlp_bwd_ws_floats(n1, B * S1));
    }
  }
  L->total = o;
  return CNERF_OK;
}

// One level as the launches take it: its network and its slices of the workspace
struct Level {
  const cnerf_net* net;
  const float* packed;
  int S, C;
  float *z, *raw, *w, *stash, *d_raw, *bwd;   // (stash / d_raw / bwd: training layouts only)
  const float* noise;
};
float* at(float* ws, int64_t off) { return off < 0 ? nullptr : ws + off; }   // (-1: not in this layout)
Level level0(const Layout& L, const cnerf_net* net, const float* packed, int Nc, const float* noise, float* ws) {
  return {net, packed, Nc, L.C0, at(ws, L.z0), at(ws, L.raw0), at(ws, L.w0), at(ws, L.stash0), at(ws, L.d_raw), at(ws, L.bwd), noise};
}
Level level1(const Layout& L, const cnerf_net* net, const float* packed, const float* noise, float* ws) {
  return {net, packed, L.S1, L.C1, at(ws, L.z1), at(ws, L.raw1), at(ws, L.w1), at(ws, L.stash1), at(ws, L.d_raw1), at(ws, L.bwd1), noise};
}

// The two ray sources of the forward: what differs between them is how coarse_z, the MLP and compositing are called.
struct RowRays {   // ray rows in memory
  const float* rays;
  int rs;
  int coarse_z(int64_t B, int Nc, const float* t_vals, const float* t_rand, int lindisp, float* z, void* stream) const {
    return cnerf_coarse_z(rays, rs, B, Nc, t_vals, t_rand, lindisp, z, stream);
  }
  int mlp(const Level& l, int64_t B, void* stream) const {
    return cnerf_mlp_fwd(l.net, l.packed, nullptr, rays, rs, nullptr, l.z, B, l.S, l.raw, l.stash, stream);
  }
  int composite(const Level& l, int64_t B, int white, float* rgb, float* disp, float* acc, float* depth, void* stream) const {
    return cnerf_composite_fwd(l.raw, l.C, l.z, rays, rs, l.noise, B, l.S, white, rgb, disp, acc, depth, l.w, stream);
  }
};
struct CamRays {   // the rays of a camera, generated in the kernels (inference: no stash)
  RayGenDev cam;
  int coarse_z(int64_t B, int Nc, const float* t_vals, const float* t_rand, int lindisp, float* z, void* stream) const {
    return cn_coarse_z_cam(cam, B, Nc, t_vals, t_rand, lindisp, z, cn_stream(stream));
  }
  int mlp(const Level& l, int64_t B, void* stream) const {
    return cn_mlp_fwd_cam(l.net, l.packed, cam, l.z, B, l.S, l.raw, cn_stream(stream));
  }
  int composite(const Level& l, int64_t B, int white, float* rgb, float* disp, float* acc, float* depth, void* stream) const {
    return cn_composite_fwd_cam(l.raw, l.C, l.z, cam, l.noise, B, l.S, white, rgb, disp, acc, depth, l.w, cn_stream(stream));
  }
};

// The forward of both entry points, after their own checks (B > 0)
template <class Rays>
int forward(const Rays& r, const cnerf_net* coarse, const float* packed_coarse, const cnerf_net* fine, const float* packed_fine,
            int64_t B, const cnerf_render_cfg& cfg, const Layout& L, const float* t_vals, const float* t_rand, const float* u,
            int64_t u_row_stride, const float* noise0, const float* noise1, const cnerf_render_out* out, float* ws, void* stream) {
  int rc;
  const bool two = cfg.Nf > 0;
  // coarse level (R:355-393)
  const Level l0 = level0(L, coarse, packed_coarse, cfg.Nc, noise0, ws);
  if ((rc = r.coarse_z(B, cfg.Nc, t_vals, t_rand, cfg.lindisp, l0.z, stream))) return rc;
  if ((rc = r.mlp(l0, B, stream))) return rc;
  if ((rc = r.composite(l0, B, cfg.white_bkgd, two ? out->rgb0 : out->rgb_map, two ? out->disp0 : out->disp_map,
                        two ? out->acc0 : out->acc_map, two ? out->depth0 : out->depth_map, stream)))
    return rc;
  // fine level (R:395-404); R:402: the coarse network serves both levels when there is no fine one
  const Level l1 = level1(L, fine ? fine : coarse, fine ? packed_fine : packed_coarse, noise1, ws);
  if (two) {
    if ((rc = cnerf_resample(l0.z, l0.w, u, u_row_stride, B, cfg.Nc, cfg.Nf, l1.z, out->z_std, nullptr, nullptr, stream))) return rc;
    if ((rc = r.mlp(l1, B, stream))) return rc;
    if ((rc = r.composite(l1, B, cfg.white_bkgd, out->rgb_map, out->disp_map, out->acc_map, out->depth_map, stream))) return rc;
  }
  // optional copies of the last level's per-sample tensors (retraw, R:412)
  const Level& last = two ? l1 : l0;
  const size_t n = (size_t)B * last.S * 4;
  hipStream_t st = cn_stream(stream);
  if (out->raw && hipMemcpyAsync(out->raw, last.raw, n * last.C, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
  if (out->z_vals && hipMemcpyAsync(out->z_vals, last.z, n, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
  if (out->weights && hipMemcpyAsync(out->weights, last.w, n, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
  return CNERF_OK;
}

}  // namespace

extern "C" int64_t cnerf_render_ws_floats(const cnerf_net* coarse, const cnerf_net* fine, const cnerf_render_cfg* cfg,
                                          int64_t B) {
  Layout L;
  return make_layout(coarse, fine, cfg, B, &L) == CNERF_OK ? L.total : -1;
}

extern "C" int cnerf_render_fwd(const cnerf_net* coarse, const float* packed_coarse, const cnerf_net* fine,
                                const float* packed_fine, const float* rays, int64_t B, const cnerf_render_cfg* cfg,
                                const float* t_vals, const float* t_rand, const float* u, int64_t u_row_stride,
                                const float* noise0, const float* noise1, const cnerf_render_out* out,
                                float* workspace, void* stream) {
  Layout L;
  int rc = make_layout(coarse, fine, cfg, B, &L);
  if (rc) return rc;
  if (!packed_coarse || !rays || !t_vals || !out || !workspace || (fine && !packed_fine) || (cfg->Nf > 0 && !u))
    return CNERF_E_ARG;
  if (B == 0) return CNERF_OK;
  return forward(RowRays{rays, cfg->ray_stride}, coarse, packed_coarse, fine, packed_fine, B, *cfg, L, t_vals, t_rand, u,
                 u_row_stride, noise0, noise1, out, workspace, stream);
}

extern "C" int cnerf_render_fwd_cam(const cnerf_net* coarse, const float* packed_coarse, const cnerf_net* fine,
                                    const float* packed_fine, const cnerf_raygen* cam_in, int64_t B,
                                    const cnerf_render_cfg* cfg_in, const float* t_vals, const float* t_rand, const float* u,
                                    int64_t u_row_stride, const float* noise0, const float* noise1,
                                    const cnerf_render_out* out, float* workspace, void* stream) {
  if (!cfg_in || cfg_in->train) return CNERF_E_ARG;
  cnerf_render_cfg cfg = *cfg_in;
  cfg.ray_stride = 11;
  CamRays r;
  int rc = cn_make_raygen(cam_in, &r.cam);
  if (rc) return rc;
  if (r.cam.first + B > (int64_t)cam_in->H * cam_in->W) return CNERF_E_ARG;
  Layout L;
  if ((rc = make_layout(coarse, fine, &cfg, B, &L))) return rc;
  if (!packed_coarse || !t_vals || !out || !workspace || (fine && !packed_fine) || (cfg.Nf > 0 && !u)) return CNERF_E_ARG;
  if (B == 0) return CNERF_OK;
  return forward(r, coarse, packed_coarse, fine, packed_fine, B, cfg, L, t_vals, t_rand, u, u_row_stride, noise0, noise1, out,
                 workspace, stream);
}

extern "C" int cnerf_render_bwd(const cnerf_net* coarse, const float* packed_coarse, const cnerf_net* fine,
                                const float* packed_fine, const float* rays, int64_t B, const cnerf_render_cfg* cfg,
                                const float* noise0, const float* noise1, const cnerf_render_grads* g, float* workspace,
                                const cnerf_ptrs* grads_coarse, const cnerf_ptrs* grads_fine, int accumulate,
                                void* stream) {
  Layout L;
  int rc = make_layout(coarse, fine, cfg, B, &L);
  if (rc) return rc;
  if (!cfg->train || !packed_coarse || !rays || !g || !workspace || !grads_coarse || (fine && (!packed_fine || !grads_fine)))
    return CNERF_E_ARG;
  if (B == 0) return CNERF_OK;
  const bool two = cfg->Nf > 0;
  const Level l0 = level0(L, coarse, packed_coarse, cfg->Nc, noise0, workspace);
  const Level l1 = level1(L, fine ? fine : coarse, fine ? packed_fine : packed_coarse, noise1, workspace);
  // a level's compositing backward: the seeds of the final maps (`last`) or of the coarse maps of a two-level render -> its d_raw
  auto composite_bwd = [&](const Level& l, bool last) {
    return cnerf_composite_bwd(l.raw, l.C, l.z, rays, cfg->ray_stride, l.noise, B, l.S, cfg->white_bkgd,
                               last ? g->g_rgb_map : g->g_rgb0, last ? g->g_disp_map : g->g_disp0, last ? g->g_acc_map : g->g_acc0,
                               last ? g->g_depth_map : g->g_depth0, l.d_raw, stream);
  };
  auto mlp_bwd = [&](const Level& l, int acc) {
    return cnerf_mlp_bwd(l.net, l.packed, l.d_raw, B, l.S, l.stash, l.bwd, grads_coarse, acc, stream);
  };
  if (!two) return (rc = composite_bwd(l0, true)) ? rc : mlp_bwd(l0, accumulate);
  if ((rc = composite_bwd(l1, true))) return rc;   // fine level first (the order autograd runs it)
  if (fine) {
    // two networks: their backward passes are independent (the fine depths are detached, R:397) -> both compositing
    // backwards, then ONE dgrad grid + ONE wgrad grid for both (fine level first: the larger blocks lead the grid)
    if ((rc = composite_bwd(l0, false))) return rc;
    return cnerf_mlp_bwd_pair(fine, packed_fine, l1.d_raw, B, l1.S, l1.stash, l1.bwd, grads_fine, coarse, packed_coarse, l0.d_raw, B,
                              l0.S, l0.stash, l0.bwd, grads_coarse, accumulate, stream);
  }
  // one network serving both levels (R:402); the coarse pass adds to what the fine pass wrote
  if ((rc = mlp_bwd(l1, accumulate))) return rc;
  return (rc = composite_bwd(l0, false)) ? rc : mlp_bwd(l0, 1);
}
