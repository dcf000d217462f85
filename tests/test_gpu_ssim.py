"""GPU tests of SSIM (csrc/ssim.hip, consistentnerf_amd/ssim.py, io_formats.img2ssim) and of V's patch SSIM term in the C3 step
(run_nerf_view.render_loss(ssim_w=...)), against the float64 restatement of pytorch-msssim 0.2.1 in tests/_ssim_ref.py."""
import numpy as np
import pytest
import torch

import _inputs as I
import _ssim_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _pair(shape, seed, dev, noise=0.15):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(*shape, generator=g)
    Y = (X + noise * torch.randn(*shape, generator=g)).clamp(0, 1)
    return X.to(dev), Y.to(dev)


def _bound(got, ref64, ref32):
    """<= 1e-5 from float64 and no more than 2x the reference's own fp32 arithmetic + 1e-7."""
    d = (got.double() - ref64).abs().max().item()
    d32 = (ref32.double() - ref64).abs().max().item()
    assert d <= 1e-5 and d <= 2 * d32 + 1e-7, (d, d32)


@pytest.mark.parametrize("shape,dr", [((4, 3, 64, 80), 1.0), ((2, 3, 301, 401), 255.0), ((1, 16, 16, 3), 1.0), ((1, 3, 8, 8), 1.0)])
def test_ssim_against_the_float64_statement(dev, shape, dr):
    from consistentnerf_amd import ssim as S
    X, Y = _pair(shape, 1, dev)
    X, Y = X * dr, Y * dr
    for sa in (True, False):
        got = S.ssim(X, Y, data_range=dr, size_average=sa)
        ref64 = R.ssim(X.double(), Y.double(), data_range=dr, size_average=sa)
        ref32 = R.ssim(X, Y, data_range=dr, size_average=sa)
        _bound(got, ref64, ref32)
        assert torch.equal(got, S.ssim(X, Y, data_range=dr, size_average=sa))     # deterministic reductions
    # per-channel values and nonnegative_ssim through the same kernels
    got = S.ssim(X, 1 - Y if dr == 1.0 else dr - Y, data_range=dr, size_average=False, nonnegative_ssim=True)
    ref = R.ssim(X.double(), (1 - Y if dr == 1.0 else dr - Y).double(), data_range=dr, size_average=False, nonnegative_ssim=True)
    assert (got.double() - ref).abs().max().item() <= 1e-5


def test_ssim_other_windows(dev):
    from consistentnerf_amd import ssim as S
    X, Y = _pair((2, 2, 70, 90), 4, dev)
    for ws, sg in ((7, 1.0), (31, 3.0), (1, 1.5)):
        got = S.ssim(X, Y, data_range=1, win_size=ws, win_sigma=sg, size_average=False)
        _bound(got, R.ssim(X.double(), Y.double(), data_range=1, win_size=ws, win_sigma=sg, size_average=False),
               R.ssim(X, Y, data_range=1, win_size=ws, win_sigma=sg, size_average=False))


def test_ms_ssim_and_img2ssim(dev):
    from consistentnerf_amd import io_formats as F, ssim as S
    X, Y = _pair((4, 3, 756, 1008), 2, dev)
    got = S.ms_ssim(X, Y, data_range=1)
    _bound(got, R.ms_ssim(X.double(), Y.double(), data_range=1), R.ms_ssim(X, Y, data_range=1))
    assert torch.equal(got, S.ms_ssim(X, Y, data_range=1))
    got = S.ms_ssim(X[:2, :, :301, :401], Y[:2, :, :301, :401], data_range=1, size_average=False)
    _bound(got, R.ms_ssim(X[:2, :, :301, :401].double(), Y[:2, :, :301, :401].double(), data_range=1, size_average=False),
           R.ms_ssim(X[:2, :, :301, :401], Y[:2, :, :301, :401], data_range=1, size_average=False))
    # img2ssim at DTU-like 300 x 400, masked and not; numpy inputs as the metrics loop passes them
    x, y = _pair((2, 300, 400, 3), 3, dev)
    rs = np.random.RandomState(0)
    m = torch.from_numpy((rs.uniform(size=(2, 300, 400)) < 0.6).astype(np.float32)).to(dev)
    for mask in (None, m):
        s, ms = F.img2ssim(x.cpu().numpy(), y.cpu().numpy(), None if mask is None else mask.cpu().numpy())
        assert s.dim() == 0 and ms.dim() == 0 and s.is_cuda
        s64, ms64 = R.img2ssim(x.double(), y.double(), None if mask is None else mask.double())
        s32, ms32 = R.img2ssim(x, y, mask)
        _bound(s, s64, s32)
        _bound(ms, ms64, ms32)


@pytest.mark.parametrize("shape", [(2, 3, 64, 80), (1, 16, 16, 3), (1, 3, 8, 8), (1, 2, 37, 300)])
def test_ssim_gradients(dev, shape):
    from consistentnerf_amd import ssim as S
    X, Y = _pair(shape, 5, dev)
    g_out = torch.rand(shape[0], generator=torch.Generator().manual_seed(9)).to(dev)
    grads = []
    for dt in (None, torch.float64, torch.float32):
        x = (X if dt is None else X.to(dt)).clone().requires_grad_()
        y = (Y if dt is None else Y.to(dt)).clone().requires_grad_()
        v = S.ssim(x, y, data_range=1, size_average=False) if dt is None else R.ssim(x, y, data_range=1, size_average=False)
        gx, gy = torch.autograd.grad((v * g_out.to(v.dtype)).sum(), (x, y))
        grads.append((gx.double(), gy.double()))
    (kx, ky), (rx, ry), (fx, fy) = grads
    for k, r, f in ((kx, rx, fx), (ky, ry, fy)):
        scale = r.abs().max().item()
        d, d32 = (k - r).abs().max().item() / scale, (f - r).abs().max().item() / scale
        assert d <= 2 * d32 + 1e-6 and d <= 1e-3, (d, d32)
    # dX alone (Y constant) through the same backward
    x = X.clone().requires_grad_()
    gx1, = torch.autograd.grad(S.ssim(x, Y, data_range=1), (x,))
    gx2, = torch.autograd.grad(S.ssim(x, Y, data_range=1), (x,))
    assert torch.equal(gx1, gx2)


def test_patch_ssim_standalone(dev):
    from consistentnerf_amd import run_nerf_view as V
    rgb, tgt = _pair((2100, 3), 6, dev)
    for P in (1, 4, 8):
        r = rgb.clone().requires_grad_()
        v = V.patch_ssim(r, tgt, P)
        g, = torch.autograd.grad(v, (r,))
        r64 = rgb.double().requires_grad_()
        v64 = R.patch_level(r64, tgt.double(), P)
        g64, = torch.autograd.grad(v64, (r64,))
        assert abs(v.item() - v64.item()) <= 1e-5
        assert (g.double() - g64).abs().max().item() <= 1e-3 * g64.abs().max().item()
        assert float(g[P * 256:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the C3 step's patch SSIM term
def _model(D, W, seed, dev):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = I.nerf_state_dict(D, W, 10, 4, 5, True, seed)
    m = NeRF(D=D, W=W, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev)


def _kwargs(coarse, fine, Nc, Nf, far):
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    e, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    q = lambda inputs, viewdirs, fn: run_network(inputs, viewdirs, fn, embed_fn=e, embeddirs_fn=ed)  # noqa: E731
    return dict(network_query_fn=q, perturb=1.0, N_importance=Nf, network_fine=fine, N_samples=Nc, network_fn=coarse,
                white_bkgd=False, raw_noise_std=0.0, lindisp=False, use_viewdirs=True, ndc=False, near=1.2, far=far)


def _batch(dev, B, seed, far):
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return (t(I.ray_batch(B, seed=seed, near=1.2, far=far)), t(rs.uniform(size=(B, 3)).astype(np.float32)),
            t(rs.uniform(1.2, far, size=(B,)).astype(np.float32)), t((rs.uniform(size=(B,)) < 0.55).astype(np.float32)),
            t(rs.uniform(0.05, 1.0, size=(1024,)).astype(np.float32)))


def _run(dev, route, Nf, with_depth, with_patch, with_mask, owned, ssim_w, B=1500, seed=31):
    from consistentnerf_amd import run_nerf_view as V
    from consistentnerf_amd.optim import FusedAdam
    far = 12.0
    rays, target, prior, mask, mono = _batch(dev, B, seed, far)
    H = W = 64
    K = I.intrinsics(H, W, 50.0)
    coarse = _model(4, 128, 93, dev)
    fine = _model(4, 128, 94, dev) if Nf else None
    params = list(coarse.parameters()) + (list(fine.parameters()) if fine is not None else [])
    opt = FusedAdam(params, lr=5e-4) if owned else None
    kw = _kwargs(coarse, fine, 32, Nf, far)
    m, d, mo = mask if with_mask else None, prior if with_depth else None, mono if with_patch else None
    torch.manual_seed(7)
    if route == "fused":
        extra = {} if ssim_w is None else dict(ssim_w=ssim_w)
        out = V.render_loss(H, W, K, target, mask=m, depth_prior=d, chunk=4096, rays=(rays[:, 0:3], rays[:, 3:6]), hardmask_coef=0.2,
                            rgb_w=1.0, depth_w=0.1, mono=mo, patch_num=4, patch_size=16, patch_w=0.001, **extra, **kw)
    else:
        out = V._render_loss_lines(H, W, K, target, m, d, 4096, (rays[:, 0:3], rays[:, 3:6]), 0.2, far, 1.0, 0.1, mo,
                                   4 if with_patch else 0, 16, 0.001, None, kw, ssim_w=ssim_w or 0.0)
    loss, terms = out[0], out[1]
    if opt is not None:
        opt.zero_grad()
    loss.backward()
    grads = opt.flat_grad.clone() if opt is not None else torch.cat(
        [(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
    return loss.detach(), {k: v.item() for k, v in terms.items() if v is not None}, out[2], out[5], out[6], grads, target


@pytest.mark.parametrize("Nf,with_depth,with_patch,with_mask,owned", [(48, True, True, True, True), (48, True, True, True, False),
                                                                      (0, True, True, True, True), (48, False, False, False, True),
                                                                      (0, False, False, True, False)])
def test_render_loss_ssim_fused_equals_the_lines(dev, Nf, with_depth, with_patch, with_mask, owned):
    lf, tf, rgbf, depf, exf, gf, target = _run(dev, "fused", Nf, with_depth, with_patch, with_mask, owned, 0.005)
    lr, tr, rgbr, depr, exr, gr, _ = _run(dev, "lines", Nf, with_depth, with_patch, with_mask, owned, 0.005)
    assert torch.equal(rgbf, rgbr) and torch.equal(depf, depr)
    if Nf:
        assert torch.equal(exf["rgb0"], exr["rgb0"])
    assert "ssim" in tr and ("ssim0" in tr) == bool(Nf)
    for k, v in tr.items():
        assert abs(tf[k] - v) <= 2e-7 * abs(v) + 1e-12, (k, tf[k], v)
    assert abs(lf.item() - lr.item()) <= 3e-7 * abs(lr.item())
    assert float(gr.abs().max()) > 0 and torch.equal(gf, gr)
    # the level values against float64 on the returned maps (the quirk reshape), and the loss as the assembled sum
    levels = [("", rgbf)] + ([("0", exf["rgb0"])] if Nf else [])
    for sfx, rgb in levels:
        ref = R.patch_level(rgb.double(), target.double(), 4).item()
        assert abs(tf["ssim" + sfx] - ref) <= 1e-5     # (near 0 here: random targets against an untrained render)
    tot = 0.0
    for sfx, _ in levels:
        tot += 1.0 * tf["img_loss" + sfx] + 0.001 * tf.get("patch_loss" + sfx, 0.0) - 0.005 * tf["ssim" + sfx]
        tot += 0.1 * tf.get("depth_loss" + sfx, 0.0) if with_depth else 0.0
    assert abs(lf.item() - tot) <= 1e-6 * max(1.0, abs(tot))


def test_render_loss_ssim_off_is_todays_call(dev):
    a = _run(dev, "fused", 48, True, True, True, True, None)
    b = _run(dev, "fused", 48, True, True, True, True, 0.0)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[5], b[5]) and "ssim" not in b[1]
    c = _run(dev, "fused", 48, True, True, True, True, 0.005)
    assert not torch.equal(a[5], c[5])


def test_c3_step_with_ssim_same_launches_and_graph(dev):
    """The C3 step with ssim_w > 0 launches as many kernels as with ssim_w = 0, and its hipGraph replay equals the eager step."""
    from consistentnerf_amd import run_nerf as Rn, run_nerf_view as V
    from consistentnerf_amd.graph import GraphedStep
    from consistentnerf_amd.optim import FusedAdam
    far, H, W = 12.0, 64, 64
    K = I.intrinsics(H, W, 50.0)
    B = 1024

    def build(ssim_w):
        coarse, fine = _model(4, 128, 11, dev), _model(4, 128, 12, dev)
        opt = FusedAdam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)
        kw = _kwargs(coarse, fine, 32, 48, far)

        def step(ro, rd, tgt, msk, pr, mono):
            loss = V.render_loss(H, W, K, tgt, mask=msk, depth_prior=pr, chunk=4096, rays=(ro, rd), depth_w=0.1, mono=mono,
                                 ssim_w=ssim_w, **kw)[0]
            opt.zero_grad()
            Rn.backward(loss)
            opt.step()
            return loss
        return opt, step
    batches = []
    for i in range(4):
        rays, tgt, pr, msk, mono = _batch(dev, B, 50 + i, far)
        batches.append((rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), tgt, msk, pr, mono))
    counts = []
    for sw in (0.0, 0.005):
        opt, step = build(sw)
        step(*batches[0])
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step(*batches[1])
            torch.cuda.synchronize()
        counts.append(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
    assert counts[0] == counts[1] and counts[0] > 0, counts
    opt_e, step_e = build(0.005)
    opt_e.make_capturable()
    torch.manual_seed(2024)
    for _ in range(3):
        step_e(*batches[0])
    le = [step_e(*b).item() for b in batches]
    opt_g, step_g = build(0.005)
    torch.manual_seed(2024)
    gs = GraphedStep(step_g, opt_g, batches[0], warmup=3)
    lg = [float(gs(*b).detach().clone()) for b in batches]
    gs.release()
    assert le == lg, (le, lg)
    assert torch.equal(opt_e.flat_param, opt_g.flat_param)
