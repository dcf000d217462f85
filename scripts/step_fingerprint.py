#!/usr/bin/env python3
"""A fingerprint of the host path between a caller and the C ABI: for every route below, the ordered list of C entry points it calls
(recorded by wrapping _lib.check), the philox offset of the device's torch generator after it, and the sha256 of every tensor it
returns and of every parameter gradient it leaves.  A change of host code only (run_nerf.py, run_nerf_view.py, ops.py) must leave
the file this writes identical: run it on the commit before and on the commit after, and compare.  It uses nothing but API that
predates it.  Shapes: 64 x 64 views, D = 2 / W = 64 networks with view directions, 32 + 32 samples, 512 rays (two 16 x 16 patches),
chunk 4096.  The plane forwards (ops.mlp_forward_bf*) run on a D = 2 / W = 128 network: W = 64 is outside their envelope.

usage: python scripts/step_fingerprint.py OUT.json                  (every route)
       python scripts/step_fingerprint.py --sequences OUT.json      (tests/golden/entry_sequences.json: the entry-point lists of the
                                                                     routes tests/test_gpu_entry_sequence.py replays)"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import _inputs as I  # noqa: E402
import _lpips_ref  # noqa: E402

H = W = 64
NEAR, FAR, CHUNK, SEED = 1.2, 12.0, 4096, 20260
NC = NF = 32
SEQUENCE_ROUTES = ("render_loss.two_levels", "view.ssim_lpips", "view.softmask", "ss.one_render.1100")


@contextlib.contextmanager
def recording():
    """The names _lib.check is handed, in call order (every launch of ops.py reports through it)."""
    from consistentnerf_amd import _lib
    names, check = [], _lib.check

    def spy(rc, what):
        names.append(what)
        return check(rc, what)
    _lib.check = spy
    try:
        yield names
    finally:
        _lib.check = check


def digest(x, out, path):
    """sha256 of every tensor in a nest of tuples / lists / dicts (shape and dtype hashed along); other leaves by repr."""
    if torch.is_tensor(x):
        t = x.detach().cpu().contiguous()
        h = hashlib.sha256(repr((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.numpy().tobytes())
        out[path] = h.hexdigest()
    elif isinstance(x, dict):
        for k in x:
            digest(x[k], out, f"{path}.{k}")
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            digest(v, out, f"{path}[{i}]")
    elif isinstance(x, np.ndarray):
        digest(torch.from_numpy(np.ascontiguousarray(x)), out, path)
    elif x is None or isinstance(x, (bool, int, float, str)):
        out[path] = repr(x)
    # (anything else — modules, PackedRays — is no result of the route)


def model(seed, dev, width=64):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = I.nerf_state_dict(2, width, 10, 4, 5, True, seed)
    m = NeRF(D=2, W=width, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev)


def scene(dev):
    from consistentnerf_amd.lpips import LPIPS
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder, get_rays_np
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    K = I.intrinsics(H, W, 52.0)
    poses = [I.camera_pose(th, -10.0, 4.0) for th in (0.0, 6.0)]
    views = [I.analytic_scene(H, W, K, p) for p in poses]
    depths = [np.minimum(v[0], FAR).astype(np.float32) for v in views]
    images = [v[1].astype(np.float32) for v in views]
    pix = np.concatenate([((r0 + np.arange(16))[:, None] * W + c0 + np.arange(16)[None]).reshape(-1) for r0, c0 in ((8, 8), (36, 28))])
    ro, rd = get_rays_np(H, W, K, poses[0])
    rs = np.random.RandomState(5)
    coarse, fine = model(71, dev), model(72, dev)
    e, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    q = lambda inputs, viewdirs, fn: run_network(inputs, viewdirs, fn, embed_fn=e, embeddirs_fn=ed)  # noqa: E731
    q._cnerf_stock = True
    kw = dict(network_query_fn=q, perturb=1.0, N_importance=NF, network_fine=fine, N_samples=NC, network_fn=coarse, white_bkgd=False,
              raw_noise_std=1.0, lindisp=False, use_viewdirs=True, ndc=False, near=NEAR, far=FAR)
    return dict(dev=dev, K=K, poses=poses, img=[t(x) for x in images], dep=[t(x) for x in depths],
                rays=torch.stack([t(ro.reshape(-1, 3)[pix]), t(rd.reshape(-1, 3)[pix])], 0), target=t(images[0].reshape(-1, 3)[pix]),
                prior=t(depths[0].reshape(-1)[pix]), mask=t(rs.uniform(size=pix.size) < 0.55), mono=t(1.0 / depths[0].reshape(-1)[pix]),
                coarse=coarse, fine=fine, wide=model(73, dev, 128), kw=kw, kw1=dict(kw, N_importance=0, network_fine=None),
                lp=LPIPS(net="vgg", weights=_lpips_ref.package_state_dict(_lpips_ref.make_weights(0))).to(dev))


def routes(sc):
    """name -> callable returning (the loss to differentiate or None, the results to hash)."""
    import torch.nn.functional as F
    from consistentnerf_amd import distributed as D, ops, run_nerf as R, run_nerf_view as V
    from consistentnerf_amd.run_nerf_helpers import ndc_coefficients
    dev, K, kw, kw1, rays, target = sc["dev"], sc["K"], sc["kw"], sc["kw1"], sc["rays"], sc["target"]
    coarse, fine = sc["coarse"], sc["fine"]
    r = {}

    def render(kwargs, **extra):
        def run():
            with torch.no_grad():
                return None, R.render(H, W, K, chunk=CHUNK, rays=rays, **dict(kwargs, **extra))
        return run

    def host_rng(**extra):
        def run():
            ops.IN_KERNEL_RNG = False
            try:
                return render(kw, **extra)()
            finally:
                ops.IN_KERNEL_RNG = True
        return run
    r["render.two_levels"] = render(kw, retraw=True)
    r["render.one_level"] = render(kw1, retraw=True)
    r["render.perturb0"] = render(kw, perturb=0.0, raw_noise_std=0.0)
    r["render.pytest"] = render(kw, pytest=True)
    r["render.global_rows"] = render(kw, _global_rows=(128, 1024))
    r["render.global_rows_pytest"] = render(kw, _global_rows=(128, 1024), pytest=True)
    r["render.host_rng"] = host_rng()
    r["render.host_rng_global_rows"] = host_rng(_global_rows=(128, 1024))
    r["render.host_rng_global_rows_perturb_negative"] = host_rng(_global_rows=(128, 1024), perturb=-1.0)
    r["render.host_rng_noise_only"] = host_rng(perturb=0.0)
    r["render.noise_only"] = render(kw, perturb=0.0)

    def lines():
        rgb, disp, acc, extras = R.render(H, W, K, chunk=CHUNK, rays=rays, retraw=True, **kw)
        return R.img2mse(rgb, target) + R.img2mse(extras["rgb0"], target), (rgb, disp, acc, extras)
    r["render.img2mse_lines"] = lines

    def mse_fold(kwargs):
        def run():
            out = R.render_loss(H, W, K, target, chunk=CHUNK, rays=rays, retraw=True, **kwargs)
            return out[0], out
        return run
    r["render_loss.two_levels"] = mse_fold(kw)
    r["render_loss.one_level"] = mse_fold(kw1)

    def empty(kwargs):
        def run():
            rows = torch.cat([rays[0], rays[1], torch.zeros(512, 5, device=dev)], 1)[:0]
            k = {a: b for a, b in kwargs.items() if a not in ("use_viewdirs", "ndc", "near", "far")}
            return None, [R.render_rays(rows, retraw=rt, _with_depth=wd, **k) for rt, wd in ((True, True), (False, False))]
        return run
    r["empty.two_levels"] = empty(kw)
    r["empty.one_level"] = empty(kw1)

    full = dict(mask=sc["mask"], depth_prior=sc["prior"], mono=sc["mono"], patch_num=2, patch_size=16, hardmask_coef=0.2, depth_w=0.1,
                patch_w=0.001)

    def view(**extra):
        def run():
            out = V.render_loss(H, W, K, target, chunk=CHUNK, rays=rays, retraw=True, **dict(full, **extra), **kw)
            return out[0], out
        return run
    temps = lambda: dict(temp_rgb=(F.softplus(fine.temp_rgb[0]), F.softplus(coarse.temp_rgb[0])),  # noqa: E731
                         temp_depth=(F.softplus(fine.temp_depth[0]), F.softplus(coarse.temp_depth[0])))
    r["view.full"] = view()
    r["view.one_level"] = lambda: _with(kw1)
    r["view.ssim"] = view(ssim_w=0.005)
    r["view.lpips"] = view(lpips_w=0.005, lpips_fn=sc["lp"])
    r["view.ssim_lpips"] = view(ssim_w=0.005, lpips_w=0.005, lpips_fn=sc["lp"])
    r["view.softmask"] = lambda: view(rgb_form="softmask", depth_form="softmask", **temps())()
    r["view.softlp_norm"] = view(rgb_form="softlp", depth_form="norm", lp_coef=1.5)
    r["view.counts"] = lambda: view(counts=D.global_mask_counts(sc["mask"]))()
    r["view.lines"] = lambda: _lines(ssim_w=0.005, ssim_patches=2, lpips_w=0.005, lpips_fn=sc["lp"])

    def _with(kwargs):
        out = V.render_loss(H, W, K, target, chunk=CHUNK, rays=rays, retraw=True, **full, **kwargs)
        return out[0], out

    def _lines(**extra):
        out = V._render_loss_lines(H, W, K, target, sc["mask"], sc["prior"], CHUNK, rays, 0.2, FAR, 1.0, 0.1, sc["mono"], 2, 16, 0.001,
                                   None, dict(kw, retraw=True), **extra)
        return out[0], out

    def ss(route, n, coins):
        def run():
            loss, info = V.ss_step_loss(H, W, K, rays[:, :n], target[:n], sc["prior"][:n], sc["poses"][1], sc["img"][1], sc["dep"][1], kw,
                                        chunk=CHUNK, occlusion_threshold=0.1, with_depth_loss=True, coins=coins, route=route)
            return loss, (loss, V.ss_host_view(info))
        return run
    for coins in ((1, 1, 1, 1), (1, 1, 0, 0)):
        tag = "".join(map(str, coins))
        r["ss.two_renders." + tag] = ss("two_renders", 512, coins)
        r["ss.one_render." + tag] = ss("one_render", 256, coins)

    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, :4] = sc["poses"][1]
    w2c = np.linalg.inv(c2w).astype(np.float32)
    coef = ndc_coefficients(H, W, K[0][0])
    rows = lambda: ops.pack_rays(rays[0], rays[1], NEAR, FAR, True, False)  # noqa: E731

    def render_fwd_bwd():
        out, st = ops.render_forward(coarse.spec(), R._packed(coarse), fine.spec(), R._packed(fine), rows(), NC, NF, train=True,
                                     u=torch.linspace(0., 1., NF, device=dev)[None], retraw=True)
        gin = {k: torch.full_like(out[k], 0.25) for k in ("rgb_map", "disp_map", "acc_map", "depth_map", "rgb0", "disp0", "acc0", "depth0")}
        gc, gf = ([torch.empty_like(p) for p in m.kernel_tensors()] for m in (coarse, fine))
        ops.render_backward(st, gin, gc, gf)
        return None, (out, gc, gf)
    r["ops.render_forward_backward"] = render_fwd_bwd

    def render_fwd_cam():
        return None, [ops.render_forward_cam(coarse.spec(), R._packed(coarse), fs, pf, H, W, K, torch.from_numpy(c2w).to(dev), NEAR, FAR, True,
                                             ndc, coef if ndc else (0., 0.), 640, 512, NC, nf, retraw=True,
                                             u=torch.linspace(0., 1., nf, device=dev)[None] if nf else None)
                      for fs, pf, nf, ndc in ((fine.spec(), R._packed(fine), NF, False), (None, None, 0, True))]
    r["ops.render_forward_cam"] = render_fwd_cam

    def warp(*mid, pose=(w2c, c2w)):
        return (rays[0], rays[1], sc["prior"], *mid, *pose, K, H, W, sc["img"][1], sc["dep"][1], 0.1, NEAR, FAR, True)
    as_tensors = (torch.from_numpy(w2c), torch.from_numpy(c2w))
    r["ops.ss_ref_rays"] = lambda: (None, [ops.ss_ref_rays(*warp(), False, (0., 0.)), ops.ss_ref_rays(*warp(), True, coef),
                                           ops.ss_ref_rays(*warp(pose=as_tensors), False, want_rows=False)])
    r["ops.ss_batch"] = lambda: (None, [ops.ss_batch(*warp(target), False, (0., 0.)), ops.ss_batch(*warp(target, pose=as_tensors), True, coef)])

    def resample():
        z = ops.coarse_z(rows(), NC, None, False)
        w = torch.rand(512, NC, device=dev)
        u = torch.rand(512, NF, device=dev)
        rng = ops.rng_draw(dev)
        return None, [ops.resample(z, w, u), ops.resample(z, w, u, want_samples=True), ops.resample(z, w, u[:1]),
                      ops.resample(z, w, None, rng=rng, Nf=NF), ops.resample(z, w, None, want_samples=True, rng=rng, Nf=NF)]
    r["ops.resample"] = resample

    # ---- the forward entry points one by one (ops.mlp_forward*, coarse_z, sample_pdf)
    def points():
        r11 = rows()
        z = ops.coarse_z(r11, NC, None, False)
        return r11, z, (r11[:, None, :3] + r11[:, None, 3:6] * z[..., None]).reshape(-1, 3), r11[:, 8:].repeat_interleave(NC, 0).contiguous()

    def mlp_forward():
        r11, z, pts, dirs = points()
        spec, pk = coarse.spec(), R._packed(coarse)
        return None, [ops.mlp_forward(spec, pk, 512 * NC, 1, pts=pts, dirs=dirs),
                      ops.mlp_forward(spec, pk, 512, NC, rays=r11[:, :8].contiguous(), z=z, dirs=r11[:, 8:].contiguous()),
                      ops.mlp_forward(spec, pk, 512, NC, rays=r11, z=z),
                      ops.mlp_forward(spec, pk, 512, NC, rays=r11, z=z, want_stash=True),
                      ops.mlp_forward(spec, pk, 512 * NC, 1, pts=pts, dirs=dirs, want_stash=True)]
    r["ops.mlp_forward"] = mlp_forward

    def mlp_forward_embedded():
        _, _, pts, dirs = points()
        x = torch.cat([ops.embed(pts, 10), ops.embed(dirs, 4)], -1)
        return None, [ops.mlp_forward_embedded(coarse.spec(), R._packed(coarse), x, want_stash=ws) for ws in (False, True)]
    r["ops.mlp_forward_embedded"] = mlp_forward_embedded

    def planes(perwave):
        def run():
            r11, z, pts, dirs = points()
            spec, params = sc["wide"].spec(), [p.detach() for p in sc["wide"].kernel_tensors()]
            if perwave:
                os.environ["CNERF_BF_PERWAVE"] = "1"
            try:
                out = []
                for n in (1, 2, 3, ops.PLANES_FP16X2):
                    pk = ops.pack_weights_bf(spec, params, n)
                    out += [ops.mlp_forward_bf(spec, pk, n, 512, NC, rays=r11, z=z), ops.mlp_forward_bf(spec, pk, n, 512 * NC, 1, pts=pts, dirs=dirs)]
                pk = ops.pack_weights_bf(spec, params, 3)
                return None, out + [ops.mlp_forward_bf_train(spec, pk, 512, NC, rays=r11, z=z)]
            finally:
                os.environ.pop("CNERF_BF_PERWAVE", None)
        return run
    r["ops.mlp_forward_bf.shared_panel"] = planes(False)
    r["ops.mlp_forward_bf.per_wave"] = planes(True)

    def coarse_z():
        t = torch.rand(512, NC, device=dev)
        return None, [ops.coarse_z(rows(), NC, t, False), ops.coarse_z(rows(), NC, None, False), ops.coarse_z(rows(), NC, t, True),
                      ops.coarse_z(rows(), NC, None, False, rng=ops.rng_draw(dev))]
    r["ops.coarse_z"] = coarse_z

    def sample_pdf():
        bins = torch.sort(torch.rand(512, NC, device=dev), -1)[0]
        w, u = torch.rand(512, NC - 1, device=dev), torch.rand(512, NF, device=dev)
        return None, [ops.sample_pdf(bins, w, u), ops.sample_pdf(bins, w, u, want_inds=True), ops.sample_pdf(bins, w, u[:1])]
    r["ops.sample_pdf"] = sample_pdf
    return r


def run_route(sc, fn):
    """One route from the fixed seed and empty gradients -> dict(entries, offset, results, grads)."""
    from consistentnerf_amd import run_nerf as R
    params = [(f"{n}.{k}", p) for n, m in (("coarse", sc["coarse"]), ("fine", sc["fine"])) for k, p in m.named_parameters()]
    for _, p in params:
        p.grad = None
    torch.manual_seed(SEED)
    with recording() as names:
        loss, results = fn()
        if loss is not None:
            R.backward(loss)
        torch.cuda.synchronize()
    out = dict(entries=list(names), offset=int(torch.cuda.default_generators[sc["dev"].index].get_offset()), results={}, grads={})
    digest(results, out["results"], "out")
    for n, p in params:
        if p.grad is not None:
            digest(p.grad, out["grads"], n)
    return out


def main():
    seq = sys.argv[1] == "--sequences"
    dev = torch.device("cuda:0")
    sc = scene(dev)
    table = routes(sc)
    out, misuse = {}, []
    for name in (SEQUENCE_ROUTES if seq else table):
        try:
            res = run_route(sc, table[name])
        except (TypeError, ValueError, KeyError, AttributeError, IndexError) as e:    # a route written against the wrong signature
            misuse.append(name)
            print(f"{name}: {type(e).__name__}: {e}", flush=True)
            continue
        out[name] = res["entries"] if seq else res
        print(f"{name}: {len(res['entries'])} entry points, {len(res['results'])} results, {len(res['grads'])} gradients", flush=True)
    with open(sys.argv[-1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    if misuse:
        sys.exit(f"routes that did not run: {misuse}")


if __name__ == "__main__":
    main()
