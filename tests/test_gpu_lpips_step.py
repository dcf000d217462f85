"""GPU tests of V's patch LPIPS term folded into the C3 step (run_nerf_view.render_loss(lpips_w=, lpips_fn=)): the patches of both
levels through ONE batched LPIPS pass inside the step's autograd node, against the lines route (_render_loss_lines: one patch_lpips
per level) and against the float64 restatement of tests/_lpips_ref.py.  The rig is test_gpu_ssim.py's; the LPIPS weights are the
seeded ones of _lpips_ref.make_weights(0)."""
import numpy as np
import pytest
import torch

import _inputs as I
import _lpips_ref as R

pytestmark = pytest.mark.gpu

FAR, H, W = 12.0, 64, 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lp(dev):
    from consistentnerf_amd.lpips import LPIPS
    return LPIPS(net="vgg", weights=R.package_state_dict(R.make_weights(0))).to(dev)


class _RefLpips(torch.nn.Module):
    """An lpips_fn that is NOT the HIP module: the restatement of _lpips_ref.py in float32 on the inputs' device (ATen autograd)."""

    def __init__(self):
        super().__init__()
        self.wts = R.make_weights(0)

    def forward(self, in0, in1):
        return R.lpips(in0, in1, self.wts)[0].reshape(-1, 1, 1, 1)


def _model(D, Wd, seed, dev):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = I.nerf_state_dict(D, Wd, 10, 4, 5, True, seed)
    m = NeRF(D=D, W=Wd, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
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
    """rays [B, 8+], targets [B, 3], depth priors [B], mask [B], mono [8 * 256] (cut to the patch count by the caller)"""
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return (t(I.ray_batch(B, seed=seed, near=1.2, far=far)), t(rs.uniform(size=(B, 3)).astype(np.float32)),
            t(rs.uniform(1.2, far, size=(B,)).astype(np.float32)), t((rs.uniform(size=(B,)) < 0.55).astype(np.float32)),
            t(rs.uniform(0.05, 1.0, size=(2048,)).astype(np.float32)))


_RUNS = {}


def _run(dev, route, B, P, Nf, owned, full, lpips_w, fn, chunk=4096, seed=31):
    """One step loss + backward -> (loss, terms, rgb, depth, extras, flat gradient, target); cached: every comparison below shares
    its runs.  full: mask, depth prior, mono and ssim_w = 0.005 next to the LPIPS term; else the LPIPS term alone.  lpips_w = None:
    the call without the two arguments."""
    key = (route, B, P, Nf, owned, full, lpips_w, None if fn is None else id(fn), chunk, seed)
    if key in _RUNS:
        return _RUNS[key]
    from consistentnerf_amd import run_nerf_view as V
    from consistentnerf_amd.optim import FusedAdam
    rays, target, prior, mask, mono = _batch(dev, B, seed, FAR)
    K = I.intrinsics(H, W, 50.0)
    coarse = _model(4, 128, 93, dev)
    fine = _model(4, 128, 94, dev) if Nf else None
    params = list(coarse.parameters()) + (list(fine.parameters()) if fine is not None else [])
    opt = FusedAdam(params, lr=5e-4) if owned else None
    kw = _kwargs(coarse, fine, 32, Nf, FAR)
    m, d, mo, sw = (mask, prior, mono[:P * 256], 0.005) if full else (None, None, None, 0.0)
    ro_rd = (rays[:, 0:3], rays[:, 3:6])
    torch.manual_seed(7)
    if route == "fused":
        extra = {} if lpips_w is None else dict(lpips_w=lpips_w, lpips_fn=fn)
        out = V.render_loss(H, W, K, target, mask=m, depth_prior=d, chunk=chunk, rays=ro_rd, hardmask_coef=0.2, rgb_w=1.0, depth_w=0.1,
                            mono=mo, patch_num=P, patch_size=16, patch_w=0.001, ssim_w=sw, **extra, **kw)
    else:
        out = V._render_loss_lines(H, W, K, target, m, d, chunk, ro_rd, 0.2, FAR, 1.0, 0.1, mo, P if full else 0, 16, 0.001, None, kw,
                                   ssim_w=sw, ssim_patches=P, lpips_w=lpips_w or 0.0, lpips_fn=fn)
    loss, terms = out[0], out[1]
    if opt is not None:
        opt.zero_grad()
    loss.backward()
    grads = opt.flat_grad.clone() if opt is not None else torch.cat(
        [(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
    _RUNS[key] = (loss.detach(), {k: v.item() for k, v in terms.items() if v is not None}, out[2], out[5], out[6], grads, target)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. the precondition
def test_lpips_batch_invariance(dev, lp):
    """An image pair gives the same value and the same input gradient alone in a batch of 4 as inside a batch of 8: what lets one pass
    serve both levels of the step."""
    x, y = R.images(8, 16, 16, 3)
    g = (torch.rand(8, generator=torch.Generator().manual_seed(9)) + 0.5).to(dev)

    def run(sl):
        a = x[sl].to(dev).requires_grad_()
        v = lp(a, y[sl].to(dev)).reshape(-1)
        (v * g[sl]).sum().backward()
        return v.detach(), a.grad
    v8, d8 = run(slice(0, 8))
    va, da = run(slice(0, 4))
    vb, db = run(slice(4, 8))
    assert torch.equal(v8, torch.cat([va, vb]))
    assert float(d8.abs().max()) > 0 and torch.equal(d8, torch.cat([da, db]))


# ------------------------------------------------------------------------------------------------ 2. folded == the lines
CASES = [(1500, 4, 48, True), (1500, 4, 0, True), (264, 1, 48, True), (2056, 8, 48, True)]


def _compare(dev, lp, B, P, Nf, owned, full):
    lf, tf, rgbf, depf, exf, gf, _ = _run(dev, "fused", B, P, Nf, owned, full, 0.005, lp)
    lr, tr, rgbr, depr, exr, gr, _ = _run(dev, "lines", B, P, Nf, owned, full, 0.005, lp)
    assert torch.equal(rgbf, rgbr) and torch.equal(depf, depr)
    if Nf:
        assert torch.equal(exf["rgb0"], exr["rgb0"])
    assert "lpips" in tr and ("lpips0" in tr) == bool(Nf) and ("ssim" in tr) == full
    assert set(tr) <= set(tf)
    for k, v in tr.items():
        print(f"B={B} P={P} Nf={Nf} owned={owned} full={full} {k}: folded {tf[k]!r} lines {v!r}")
        assert abs(tf[k] - v) <= 2e-7 * abs(v) + 1e-12, (k, tf[k], v)
    assert tf["lpips"] > 0 and (not Nf or tf["lpips0"] > 0)
    assert abs(lf.item() - lr.item()) <= 3e-7 * abs(lr.item()), (lf.item(), lr.item())
    print(f"  max|grad| {float(gr.abs().max()):.3e}   max|folded - lines| {float((gf - gr).abs().max()):.3e}")
    assert float(gr.abs().max()) > 0 and torch.equal(gf, gr)


@pytest.mark.parametrize("owned", [True, False])
@pytest.mark.parametrize("B,P,Nf,full", CASES)
def test_render_loss_lpips_folded_equals_the_lines(dev, lp, B, P, Nf, full, owned):
    """Full step (mask, depth, mono, SSIM, LPIPS): maps and flat parameter gradient bit for bit, terms and loss to summation order;
    FusedAdam-owned and plain-parameter gradient routes."""
    _compare(dev, lp, B, P, Nf, owned, full)


@pytest.mark.parametrize("owned", [True, False])
def test_render_loss_lpips_term_alone_equals_the_lines(dev, lp, owned):
    """Only the LPIPS term on: no mask, no depth, no mono, ssim_w = 0."""
    _compare(dev, lp, 1500, 4, 48, owned, False)


# ------------------------------------------------------------------------------------------------ 3. the term reaches the networks
def test_lpips_term_reaches_the_networks_and_off_is_todays_call(dev, lp):
    today = _run(dev, "fused", 1500, 4, 48, True, True, None, None)
    w0 = _run(dev, "fused", 1500, 4, 48, True, True, 0.0, lp)
    nofn = _run(dev, "fused", 1500, 4, 48, True, True, 0.0, None)
    for b in (w0, nofn):
        assert torch.equal(today[0], b[0]) and today[1] == b[1] and torch.equal(today[5], b[5])
        assert "lpips" not in b[1] and "lpips0" not in b[1]
    on = _run(dev, "fused", 1500, 4, 48, True, True, 0.005, lp)
    assert not torch.equal(today[5], on[5])
    assert torch.equal(today[2], on[2])                       # (the maps do not depend on the loss)
    # the loss moves by lpips_w times the two level values
    want = today[0].item() + 0.005 * (on[1]["lpips"] + on[1]["lpips0"])
    assert abs(on[0].item() - want) <= 1e-6 * max(1.0, abs(want))


# ------------------------------------------------------------------------------------------------ 4. the value, independently
@pytest.mark.parametrize("B,P,Nf", [(1500, 4, 48), (2056, 8, 48), (1500, 4, 0)])
def test_lpips_terms_against_float64(dev, lp, B, P, Nf):
    """terms['lpips'] / ['lpips0'] against the float64 restatement on the returned maps: patches as [1, 3, 16, 16], (x - 0.5) * 2, the
    sum over the patches, / 4; the project's LPIPS value bound, 5e-6 relative."""
    _, terms, rgb, _, ex, _, target = _run(dev, "fused", B, P, Nf, True, True, 0.005, lp)
    wts = R.make_weights(0)
    img = lambda t: ((t[:P * 256].cpu().double().reshape(-1, 16, 16, 3) - 0.5) * 2.).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    for key, m in [("lpips", rgb)] + ([("lpips0", ex["rgb0"])] if Nf else []):
        ref = (R.lpips(img(m), img(target), wts)[0].sum() / 4).item()
        print(f"B={B} P={P} {key}: {terms[key]!r} float64 {ref!r} rel {abs(terms[key] - ref) / abs(ref):.2e}")
        assert abs(terms[key] - ref) <= 5e-6 * abs(ref), (key, terms[key], ref)


# ------------------------------------------------------------------------------------------------ 5. / 6. launches, graph
def _step_rig(dev, lp):
    from consistentnerf_amd import run_nerf as Rn, run_nerf_view as V
    from consistentnerf_amd.optim import FusedAdam
    K = I.intrinsics(H, W, 50.0)

    def build(lpips_w, lines=False):
        coarse, fine = _model(4, 128, 11, dev), _model(4, 128, 12, dev)
        opt = FusedAdam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)
        kw = _kwargs(coarse, fine, 32, 48, FAR)

        def step(ro, rd, tgt, msk, pr, mono):
            if lines:
                loss = V._render_loss_lines(H, W, K, tgt, msk, pr, 4096, (ro, rd), 0.2, FAR, 1.0, 0.1, mono, 4, 16, 0.001, None, kw,
                                            ssim_w=0.005, ssim_patches=4, lpips_w=lpips_w, lpips_fn=lp)[0]
            else:
                loss = V.render_loss(H, W, K, tgt, mask=msk, depth_prior=pr, chunk=4096, rays=(ro, rd), depth_w=0.1, mono=mono,
                                     ssim_w=0.005, lpips_w=lpips_w, lpips_fn=lp, **kw)[0]
            opt.zero_grad()
            Rn.backward(loss)
            opt.step()
            return loss
        return opt, step
    batches = []
    for i in range(4):
        rays, tgt, pr, msk, mono = _batch(dev, 1024, 50 + i, FAR)
        batches.append((rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), tgt, msk, pr, mono[:1024].contiguous()))
    return build, batches


def _launches(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def test_lpips_step_launch_count(dev, lp):
    """The folded term costs ONE LPIPS forward + backward over the 8 image pairs of both levels, + the pack and the seed launch;
    the lines route (two passes and their ATen glue) needs strictly more."""
    from consistentnerf_amd import ops
    build, batches = _step_rig(dev, lp)
    x, y = R.images(8, 16, 16, 5)
    x, y, packed = x.to(dev), y.to(dev), lp.packed(dev)
    g = torch.ones(8, device=dev)

    def one_pass():
        _, _, ws, _ = ops.lpips_forward(x, y, packed, keep=True)
        ops.lpips_backward(packed, ws, g, x.shape)
    n_lpips = _launches(one_pass)
    counts = {}
    for name, lw, lines in (("off", 0.0, False), ("folded", 0.005, False), ("lines", 0.005, True)):
        _, step = build(lw, lines)
        counts[name] = _launches(lambda: step(*batches[1]))
    print(f"launches: one LPIPS forward + backward at [8, 3, 16, 16] {n_lpips}; step lpips_w = 0 {counts['off']}, folded "
          f"{counts['folded']}, lines {counts['lines']}")
    assert n_lpips > 0 and counts["off"] > 0
    assert counts["folded"] - counts["off"] <= n_lpips + 3, (counts, n_lpips)
    assert counts["lines"] > counts["folded"], counts


def test_lpips_step_graph_equals_eager(dev, lp):
    """GraphedStep of the full step (ssim_w = lpips_w = 0.005, mono, mask, depth) over 4 batches: every loss and the final flat_param
    equal the eager step's."""
    from consistentnerf_amd.graph import GraphedStep
    build, batches = _step_rig(dev, lp)
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


# ------------------------------------------------------------------------------------------------ 7. fallbacks
def test_lpips_fallbacks_keep_the_term(dev, lp):
    """A batch beyond `chunk`, and an lpips_fn that is not the HIP module, take the lines: the term's values are returned and the
    gradient equals calling _render_loss_lines directly."""
    ref = _RefLpips()
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False         # ATen's own im2col convolution for the restatement: no kernel search in a test
    try:
        for chunk, fn in ((1024, lp), (4096, ref)):
            a = _run(dev, "fused", 1500, 4, 48, True, True, 0.005, fn, chunk=chunk)
            b = _run(dev, "lines", 1500, 4, 48, True, True, 0.005, fn, chunk=chunk)
            assert a[1]["lpips"] > 0 and a[1]["lpips0"] > 0 and a[1] == b[1]
            assert torch.equal(a[0], b[0]) and float(b[5].abs().max()) > 0 and torch.equal(a[5], b[5])
            off = _run(dev, "fused", 1500, 4, 48, True, True, 0.0, None, chunk=chunk)
            assert not torch.equal(a[5], off[5])
    finally:
        torch.backends.cudnn.enabled = prev
    # the restatement in float32 and the HIP network state the same term
    hip = _run(dev, "fused", 1500, 4, 48, True, True, 0.005, lp)
    other = _run(dev, "fused", 1500, 4, 48, True, True, 0.005, ref)
    for k in ("lpips", "lpips0"):
        assert abs(hip[1][k] - other[1][k]) <= 1e-5 * abs(hip[1][k]), (k, hip[1][k], other[1][k])
