"""GPU tests of the loss forms other than `--hardmask` folded into the compositing launches (run_nerf_view.render_loss(rgb_form=,
depth_form=); cnerf_composite_fwd_lossform / cnerf_lossform_finish / cnerf_composite_bwd_lossform) and of the stand-alone
`--softmask` launch (cnerf_softmask_loss), against the reference's lines on ATen (`_render_loss_lines`, whose restatement
tests/test_lossforms_host.py pins on the reference's own outputs).  Shapes: B = 264 rays (33 workgroups of 8) and B = 13 (a partial
last workgroup), S = 32; through render_loss: netdepth 4, netwidth 64, 32 + 32 samples, viewdirs, perturb 0."""
import argparse
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _inputs as I

pytestmark = pytest.mark.gpu

B, S, FAR, NEAR = 264, 32, 6.0, 1.2
H = W = 64
MSE_FORMS = ("norm", "plain", "hardmask_coef")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def scene(dev):
    """Networks of create_nerf + one 264-ray batch, shared (and left unchanged) by every render_loss test of this file."""
    from consistentnerf_amd import run_nerf_view as V
    torch.manual_seed(11)
    with tempfile.TemporaryDirectory() as tmp:
        args = argparse.Namespace(
            multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=32, netdepth=4, netwidth=64, netdepth_fine=4,
            netwidth_fine=64, netchunk=1024 * 64, lrate=5e-4, basedir=tmp, expname="lf", ft_path=None, no_reload=True, perturb=0.0,
            N_samples=32, white_bkgd=False, raw_noise_std=0.0, dataset_type="dtu", no_ndc=True, lindisp=False)
        kw, _, _, grad_vars, _opt = V.create_nerf(args)
    for name, seed in (("network_fn", 93), ("network_fine", 94)):     # seeded weights with live densities, as the other GPU tests use
        kw[name].load_state_dict({k: T(v, dev) for k, v in I.nerf_state_dict(4, 64, 10, 4, 5, True, seed).items()}, strict=True)
    kw = dict(kw, near=NEAR, far=FAR)
    rs = np.random.RandomState(5)
    rays = T(I.ray_batch(B, seed=5, near=NEAR, far=FAR), dev)
    s = dict(kw=kw, params=grad_vars, rays=rays, target=T(rs.uniform(size=(B, 3)).astype(np.float32), dev),
             prior=T(rs.uniform(NEAR, FAR, size=(B,)).astype(np.float32), dev),
             mask=T((rs.uniform(size=(B,)) < 0.55).astype(np.float32), dev),
             mono=T(rs.uniform(0.05, 1.0, size=(256,)).astype(np.float32), dev), K=I.intrinsics(H, W, 50.0))
    assert 0 < int(s["mask"].sum()) < B
    with torch.no_grad():
        acc = V.render(H, W, s["K"], chunk=4096, rays=(rays[:, 0:3], rays[:, 3:6]), **kw)[2]
    assert float(acc.max()) > 0.5, "the scene must not be empty"
    return s


def temps_of(scene):
    """What VC passes: the fine level reads network_fine's scalars, the coarse level network_fn's."""
    f, c = scene["kw"]["network_fine"], scene["kw"]["network_fn"]
    return (F.softplus(f.temp_rgb), F.softplus(c.temp_rgb)), (F.softplus(f.temp_depth), F.softplus(c.temp_depth))


def step(scene, fused, sl=slice(0, B), mask="mixed", target=None, counts=None, mono=False, ssim_w=0.0, no_backward=False, vc_temps=(),
         **forms):
    """One loss + backward through render_loss (fused) or the reference's lines -> (loss, terms, flat gradient, per-parameter grads).
    vc_temps: which of ("temp_rgb", "temp_depth") to pass as VC does (a fresh softplus graph per call)."""
    from consistentnerf_amd import run_nerf_view as V
    forms.update({k: v for k, v in zip(("temp_rgb", "temp_depth"), temps_of(scene)) if k in vc_temps})
    for p in scene["params"]:
        p.grad = None                      # (detaches FusedAdam's views: autograd leaves a tensor of its own, or None)
    m = {"mixed": scene["mask"], "ones": torch.ones_like(scene["mask"]), None: None}[mask]
    m = None if m is None else m[sl]
    tgt = (scene["target"] if target is None else target)[sl]
    rays = (scene["rays"][sl, 0:3], scene["rays"][sl, 3:6])
    if fused:
        out = V.render_loss(H, W, scene["K"], tgt, mask=m, depth_prior=scene["prior"][sl], chunk=4096, rays=rays, hardmask_coef=0.2,
                            depth_w=0.1, mono=scene["mono"] if mono else None, patch_num=1, counts=counts, ssim_w=ssim_w, **forms,
                            **scene["kw"])
    else:
        f = dict(forms)
        temps = V._temps4(f.pop("temp_rgb", None), f.pop("temp_depth", None))
        out = V._render_loss_lines(H, W, scene["K"], tgt, m, scene["prior"][sl], 4096, rays, 0.2, FAR, 1.0, 0.1,
                                   scene["mono"] if mono else None, 1 if mono else 0, 16, 0.001, counts, scene["kw"], ssim_w=ssim_w,
                                   ssim_patches=1, temps=temps, **f)
    if no_backward:
        return out[0], out[1], out
    loss, terms = out[0], {k: v.item() for k, v in out[1].items()}
    loss.backward()
    grads = {id(p): p.grad for p in scene["params"]}
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in scene["params"]])
    return loss.detach(), terms, flat, grads


def scalar_grads(scene, grads):
    return {(n, k): grads[id(getattr(scene["kw"][n], k))] for n in ("network_fine", "network_fn") for k in ("temp_rgb", "temp_depth")}


@pytest.mark.parametrize("form,mask", [("norm", "mixed"), ("plain", "mixed"), ("hardmask_coef", "mixed"), ("hardmask_coef", "ones"),
                                       ("norm", None)])
def test_mse_type_depth_forms_equal_the_lines_bit_for_bit(scene, form, mask):
    """render_loss(depth_form=...) — a TypeError before the forms existed — against `_render_loss_lines` with the same form: every
    term to fp64-association round-off (2e-7, the bound of the hardmask form's test), and after backward() every parameter
    gradient BIT FOR BIT (the seeds are the literal lines' fp32 operations in their order, x / far as ATen's x * (1 / far))."""
    lf, tf, gf, _ = step(scene, True, mask=mask, depth_form=form)
    lr, tr, gr, _ = step(scene, False, mask=mask, depth_form=form)
    for k, v in tr.items():
        print(form, mask, k, tf[k], v)
        assert abs(tf[k] - v) <= 2e-7 * abs(v) + 1e-12, (k, tf[k], v)
    assert abs(lf.item() - lr.item()) <= 3e-7 * abs(lr.item())
    print(form, mask, "max|grad|", float(gr.abs().max()), "max|d grad|", float((gf - gr).abs().max()))
    assert float(gr.abs().max()) > 0 and torch.equal(gf, gr)


def test_softlp_folded(scene):
    """rgb_form = depth_form = "softlp" (V:58 on colours and on depths / far) with coef 0.5 and three EXACT-zero colour residuals:
    loss 1e-6 relative, gradients 2e-6 of their largest element against the lines (the bounds of the stand-alone launch: powf vs
    ATen's pow), everything finite (the kernel's limit 0 where the reference's autograd forms inf * 0)."""
    from consistentnerf_amd import run_nerf_view as V
    with torch.no_grad():
        out = step(scene, True, no_backward=True)[2]
    target = scene["target"].clone()
    target[:3] = out[2][:3]                  # rgb of the fine level: exact zeros of its residual
    forms = dict(rgb_form="softlp", depth_form="softlp", lp_coef=0.5)
    lf, tf, gf, _ = step(scene, True, target=target, **forms)
    lr, tr, gr, _ = step(scene, False, target=target, **forms)
    for k, v in tr.items():
        print("softlp", k, tf[k], v)
        assert abs(tf[k] - v) <= 1e-6 * abs(v), (k, tf[k], v)
    scale = float(gr.abs().max())
    print("softlp max|grad|", scale, "max|d grad|", float((gf - gr).abs().max()))
    assert torch.isfinite(gf).all() and scale > 0 and float((gf - gr).abs().max()) <= 2e-6 * scale
    assert V.img2mse_softLpmask is not None


def aten_softmask(x, y, t):
    """V:50 / V:55, literally."""
    return torch.sum((torch.exp((x - y) ** 2 / t)) * (x - y) ** 2) / torch.sum(torch.exp((x - y).detach() ** 2 / t))


def _dist(a, ref):
    return float((a.double() - ref.double()).abs().max())


def kernel_batch(dev, b, mask_kind, s=S):
    g = torch.Generator(device="cpu").manual_seed(100 + b)
    raw = (torch.randn(b, s, 4, generator=g) * 3).to(dev)
    z = torch.sort(torch.rand(b, s, generator=g) * (FAR - NEAR) + NEAR, -1).values.to(dev)
    rays = T(I.ray_batch(b, seed=b, near=NEAR, far=FAR), dev)
    tgt = torch.rand(b, 3, generator=g).to(dev)
    prior = (torch.rand(b, generator=g) * (FAR - NEAR) + NEAR).to(dev)
    mask = (torch.rand(b, generator=g) < 0.55).float().to(dev) if mask_kind == "mixed" else torch.ones(b, device=dev)
    return raw, z, rays, tgt, prior, mask


def lines64(rgb, depth, tgt, prior, mask, rf, df, temps, coef=0.2, lp=0.5):
    """The forms on given maps in float64 (ATen) -> (img_loss, depth_loss, d img_loss / d rgb, d depth_loss / d depth, dt_rgb, dt_depth)."""
    c, d = rgb.double().requires_grad_(True), depth.double().requires_grad_(True)
    tr, td = (t.double().detach().requires_grad_(True) for t in temps)
    tg, pr, far = tgt.double(), prior.double(), FAR
    mse = lambda a, b: torch.mean((a - b) ** 2)  # noqa: E731
    softlp = lambda a, b: torch.sum(((a - b).abs() ** lp + 1) * (a - b) ** 2) / torch.sum((a - b).abs() ** lp + 1).detach()  # noqa: E731
    m1, m0 = mask == 1, mask == 0
    if rf == "hardmask":
        il = mse(c[m1], tg[m1]) + (coef * mse(c[m0], tg[m0]) if bool(m0.any()) else 0.0)
    else:
        il = softlp(c, tg) if rf == "softlp" else aten_softmask(c, tg, tr)
    p2 = torch.where(m0, torch.zeros_like(pr), pr)
    if df == "hardmask":
        dl = mse(d[m1] / far, pr[m1] / far)
    elif df == "hardmask_coef":
        dl = mse(d[m1] / far, pr[m1] / far) + (coef * mse(d[m0] / far, pr[m0] / far) if bool(m0.any()) else 0.0)
    elif df == "norm":
        dl = mse(d / far, p2 / far)
    elif df == "plain":
        dl = mse(d, p2)
    else:
        dl = softlp(d / far, pr / far) if df == "softlp" else aten_softmask(d / far, pr / far, td)
    (il + dl).backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    return il.detach(), dl.detach(), c.grad, d.grad, z(tr), z(td)


@pytest.mark.parametrize("b,mask_kind", [(264, "mixed"), (264, "ones"), (13, "mixed")])
@pytest.mark.parametrize("rf,df", [("hardmask", "norm"), ("hardmask", "plain"), ("hardmask", "hardmask_coef"), ("softlp", "softlp"),
                                   ("softmask", "softmask"), ("softlp", "hardmask")])
def test_lossform_kernels_vs_float64_lines(dev, b, mask_kind, rf, df):
    """The three launches through ops on raw = 3 N(0, 1): terms against the lines in float64 on the maps the forward returns, 1e-6
    relative (every fp32 product w d^2 is within 3 roundings, 2e-7, of its float64 value and the sums are fp64), the temperature
    gradients 1e-5 (a difference of two such sums, sum(w d^4) / Dn - L^2, which cancels to about a tenth of its terms), and d_raw
    against cnerf_composite_bwd fed with the float64 seeds, 2e-6 of its largest element (the softlp bound of the issue; each seed is
    <= 6 fp32 operations from its float64 value)."""
    _lossform_kernels_vs_float64_lines(dev, b, mask_kind, rf, df, S)


def test_lossform_kernels_vs_float64_lines_at_300_samples(dev):
    """The same at S = 300: the FORMS instantiations of 8 samples per lane (composite_fwd_k<8, MSE_WAVES, true>,
    composite_bwd_k<8, true>), lanes 38 ... 63 of every ray dead."""
    _lossform_kernels_vs_float64_lines(dev, 13, "mixed", "softmask", "softmask", 300)


def _lossform_kernels_vs_float64_lines(dev, b, mask_kind, rf, df, s):
    from consistentnerf_amd import ops
    raw, z, rays, tgt, prior, mask = kernel_batch(dev, b, mask_kind, s)
    temps = (torch.tensor([0.40318605], device=dev), torch.tensor([0.3], device=dev))
    L = ops.ClossSpec(tgt, mask, prior, FAR, 0.2, 1.0, 0.1, 0.0, rgb_form=ops.RGB_FORMS.index(rf), depth_form=ops.DEPTH_FORMS.index(df),
                      lp_coef=0.5, temps=temps + temps).checked(b)
    rgb, _disp, _acc, _w, depth, ws = ops.composite_forward_closs(raw, z, rays, None, False, L)
    assert ws.numel() == 10 * ((b + 7) // 8)
    terms, stats, _pd, _sd, d_temp = ops.lossform_finish(L, b, ws, None, depth, None, rgb, None)
    g_temp = torch.zeros(2, device=dev)
    g = torch.tensor([1.0], device=dev)
    d_raw = ops.composite_backward_closs(raw, z, rays, None, False, L, rgb, depth, stats[0:8], g, None, None, level=0,
                                         d_temp2=d_temp[0:2], g_temp2=g_temp)
    il, dl, g_rgb, g_dep, dt_r, dt_d = lines64(rgb, depth, tgt, prior, mask, rf, df, temps)
    want = ops.composite_backward(raw, z, rays, None, False, g_rgb.float(), None, None, (0.1 * g_dep).float())
    t = terms.cpu()
    print(rf, df, b, mask_kind, "img", float(t[1]), float(il), "depth", float(t[2]), float(dl), "d_temp", g_temp.tolist(), float(dt_r),
          0.1 * float(dt_d), "d_raw", _dist(d_raw, want), float(want.abs().max()))
    assert abs(float(t[1]) - float(il)) <= 1e-6 * abs(float(il)) and abs(float(t[2]) - float(dl)) <= 1e-6 * abs(float(dl))
    assert abs(float(t[0]) - (float(il) + 0.1 * float(dl))) <= 1e-6 * abs(float(t[0]))
    assert abs(float(g_temp[0]) - float(dt_r)) <= 1e-5 * abs(float(dt_r)) and abs(float(g_temp[1]) - 0.1 * float(dt_d)) <= 1e-6 * abs(float(dt_d))
    assert (float(dt_r) != 0) == (rf == "softmask") and (float(dt_d) != 0) == (df == "softmask")
    assert torch.isfinite(d_raw).all() and _dist(d_raw, want) <= 2e-6 * float(want.abs().max())


def test_softmask_folded_and_standalone_vs_aten_fp32(dev, scene):
    """No project number exists for exp-weighted sums: the literal lines in float64 on the same maps are the reference, the fp32 ATen
    lines' distance from it the yardstick, and the HIP path — stand-alone (img2mse_softmask on colours, img2mse_depth_softmask on
    depths / far) and folded (the three launches) — must be within 4x of it, per quantity: loss, gradient (d_x / d_raw), d / d temp.
    Through render_loss: net.temp_rgb.grad / net.temp_depth.grad of BOTH networks are None with the default forms and finite with
    the softmask forms (through F.softplus); one tensor for both levels receives the sum."""
    from consistentnerf_amd import ops, run_nerf_view as V
    raw, z, rays, tgt, prior, mask = kernel_batch(dev, B, "mixed")
    rgb, _d, _a, _w, depth = ops.composite_forward(raw, z, rays, None, False)
    tv = (0.40318605, 0.3)
    rows = []

    def lines(dtype):
        c, d = rgb.to(dtype).clone().requires_grad_(True), depth.to(dtype).clone().requires_grad_(True)
        tr, td = (torch.tensor([v], device=dev, dtype=dtype, requires_grad=True) for v in tv)
        il, dl = aten_softmask(c, tgt.to(dtype), tr), aten_softmask(d / FAR, prior.to(dtype) / FAR, td)
        (il + dl).backward()
        return il.detach(), dl.detach(), c.grad, d.grad, tr.grad, td.grad

    ref, a32 = lines(torch.float64), lines(torch.float32)
    # stand-alone
    c, d = rgb.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    tr, td = (torch.tensor([v], device=dev, requires_grad=True) for v in tv)
    il, dl = V.img2mse_softmask(c, tgt, tr), V.img2mse_depth_softmask(d / FAR, prior / FAR, td)
    (il + dl).backward()
    hip = (il.detach(), dl.detach(), c.grad, d.grad, tr.grad, td.grad)
    for k, name in enumerate(("img_loss", "depth_loss", "d_rgb", "d_depth", "d_temp_rgb", "d_temp_depth")):
        rows.append(("stand-alone " + name, _dist(hip[k], ref[k]), _dist(a32[k], ref[k]), float(ref[k].abs().max())))
    # folded
    temps = tuple(torch.tensor([v], device=dev) for v in tv)
    L = ops.ClossSpec(tgt, mask, prior, FAR, 0.2, 1.0, 1.0, 0.0, rgb_form=2, depth_form=5, temps=temps + temps).checked(B)
    rgb2, _d, _a, _w, depth2, ws = ops.composite_forward_closs(raw, z, rays, None, False, L)
    assert torch.equal(rgb2, rgb) and torch.equal(depth2, depth)
    terms, stats, _pd, _sd, d_temp = ops.lossform_finish(L, B, ws, None, depth, None, rgb, None)
    g_temp = torch.zeros(2, device=dev)
    d_raw = ops.composite_backward_closs(raw, z, rays, None, False, L, rgb, depth, stats[0:8], torch.ones(1, device=dev), None, None,
                                         level=0, d_temp2=d_temp[0:2], g_temp2=g_temp)
    through = lambda r: ops.composite_backward(raw, z, rays, None, False, r[2].float(), None, None, r[3].float())  # noqa: E731
    w64, w32 = through(ref), through(a32)
    rows += [("folded img_loss", _dist(terms[1], ref[0]), _dist(a32[0], ref[0]), float(ref[0])),
             ("folded depth_loss", _dist(terms[2], ref[1]), _dist(a32[1], ref[1]), float(ref[1])),
             ("folded d_raw", _dist(d_raw, w64), _dist(w32, w64), float(w64.abs().max())),
             ("folded d_temp_rgb", _dist(g_temp[0], ref[4][0]), _dist(a32[4], ref[4]), float(ref[4])),
             ("folded d_temp_depth", _dist(g_temp[1], ref[5][0]), _dist(a32[5], ref[5]), float(ref[5]))]
    for name, dh, da, scale in rows:
        print(f"softmask {name:28s} hip {dh:.3e}  aten-fp32 {da:.3e}  |ref| {scale:.3e}")
    for name, dh, da, scale in rows:
        assert dh <= 4.0 * da, (name, dh, da, scale)
    # through render_loss
    _, _, _, g0 = step(scene, True)
    assert all(v is None for v in scalar_grads(scene, g0).values())
    both = ("temp_rgb", "temp_depth")
    lf, tf, gf, g1 = step(scene, True, rgb_form="softmask", depth_form="softmask", vc_temps=both)
    lr, tr_, gr, g2 = step(scene, False, rgb_form="softmask", depth_form="softmask", vc_temps=both)
    s1, s2 = scalar_grads(scene, g1), scalar_grads(scene, g2)
    for k in s1:
        print("softmask render_loss", k, float(s1[k]), float(s2[k]))
        assert s1[k] is not None and torch.isfinite(s1[k]).all() and float(s1[k]) != 0
        assert abs(float(s1[k]) - float(s2[k])) <= 1e-5 * abs(float(s2[k]))
    assert abs(lf.item() - lr.item()) <= 1e-6 * abs(lr.item())
    assert float((gf - gr).abs().max()) <= 2e-6 * float(gr.abs().max())
    fine = scene["kw"]["network_fine"]
    one_r, one_d = F.softplus(fine.temp_rgb), F.softplus(fine.temp_depth)
    _, _, _, g3 = step(scene, True, rgb_form="softmask", depth_form="softmask", temp_rgb=one_r, temp_depth=one_d)
    s3 = scalar_grads(scene, g3)
    assert s3[("network_fn", "temp_rgb")] is None and float(s3[("network_fine", "temp_rgb")]) != float(s1[("network_fine", "temp_rgb")])


def test_forms_compose_and_shard(scene):
    """rgb_form "softmask" + depth_form "norm" + the monocular patch term + ssim_w = 0.005 in ONE call against the lines (loss 1e-6,
    gradients 2e-6 of their largest: the softmask form's rounding class); and "norm" under GLOBAL counts: three 88-ray shards add
    up to the one-batch call — values to fp32 round-off of three partial losses (1e-6), gradients to the sharded tests' 2e-5."""
    from consistentnerf_amd import distributed as D
    forms = dict(rgb_form="softmask", depth_form="norm", vc_temps=("temp_rgb",))
    lf, tf, gf, _ = step(scene, True, mono=True, ssim_w=0.005, **forms)
    lr, tr, gr, _ = step(scene, False, mono=True, ssim_w=0.005, **forms)
    assert set(tr) <= set(tf) and "ssim" in tf and "patch_loss0" in tf
    for k, v in tr.items():
        print("compose", k, tf[k], v)
        assert abs(tf[k] - v) <= 1e-6 * abs(v) + 1e-12, (k, tf[k], v)
    print("compose max|grad|", float(gr.abs().max()), "max|d grad|", float((gf - gr).abs().max()))
    assert float((gf - gr).abs().max()) <= 2e-6 * float(gr.abs().max())
    l_full, _, g_full, _ = step(scene, True, depth_form="norm")
    counts = D.global_mask_counts(scene["mask"])
    l_sum, g_sum = 0.0, torch.zeros_like(g_full)
    for lo in (0, 88, 176):
        l, _, g, _ = step(scene, True, sl=slice(lo, lo + 88), counts=counts, depth_form="norm")
        l_sum, g_sum = l_sum + l.item(), g_sum + g
    print("shards", l_sum, l_full.item(), float((g_sum - g_full).abs().max()), float(g_full.abs().max()))
    assert abs(l_sum - l_full.item()) <= 1e-6 * abs(l_full.item())
    assert float((g_sum - g_full).abs().max()) <= 2e-5 * float(g_full.abs().max())


def test_defaults_are_the_hardmask_form(scene):
    """render_loss with no new keyword = render_loss(rgb_form="hardmask", depth_form="hardmask"): same loss bits, same gradient bits."""
    l0, t0, g0, _ = step(scene, True)
    l1, t1, g1, _ = step(scene, True, rgb_form="hardmask", depth_form="hardmask")
    assert torch.equal(l0, l1) and t0 == t1 and torch.equal(g0, g1) and float(g0.abs().max()) > 0


@pytest.mark.parametrize("forms", [dict(depth_form="norm"), dict(depth_form="plain"), dict(depth_form="hardmask_coef"),
                                   dict(rgb_form="softlp", depth_form="softlp", lp_coef=0.5),
                                   dict(rgb_form="softmask", depth_form="softmask")])
def test_no_host_synchronisation(scene, forms):
    """A folded call of every new form, forward and backward, under torch.cuda.set_sync_debug_mode("error"): device-resident
    inputs, scalar near / far, the temperatures as device tensors."""
    from consistentnerf_amd import run_nerf as R
    f = dict(forms, vc_temps=("temp_rgb", "temp_depth") if "softmask" in forms.values() else ())
    step(scene, True, **f)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, _, out = step(scene, True, no_backward=True, **f)
        R.backward(loss)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
