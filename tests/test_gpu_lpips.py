"""GPU tests of LPIPS (csrc/lpips.hip, consistentnerf_amd/lpips.py, io_formats.img2lpips, run_nerf_view.patch_lpips) against the torch
restatement tests/_lpips_ref.py in float64 (on the CPU), with seeded weights.  Each piece alone first (convolution, its input gradient,
pool, head), then end to end.  The end-to-end gradient is compared ON THE KERNEL'S BRANCH: the restatement is forced onto the ReLU
masks and pool choices read from the kernel's stored activations, because a single flipped branch moves a float32 gradient by 1e-3
(ATen's own float32 differs from its float64 by that much at [1, 3, 37, 50]) and says nothing about the arithmetic."""
import functools
import math
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lpips_ref as R

pytestmark = pytest.mark.gpu

CONV_SHAPES = ((2, 16, 16), (3, 2, 2), (2, 1, 1), (1, 37, 50))
E2E_SHAPES = ((8, 3, 16, 16), (2, 3, 16, 21), (1, 3, 37, 50), (1, 3, 61, 83))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _wts():
    return R.make_weights(0)


@functools.lru_cache(maxsize=None)
def _model():
    from consistentnerf_amd.lpips import LPIPS
    return LPIPS(net="vgg", weights=R.package_state_dict(_wts())).to("cuda:0")


def _conv_case(ci, co, shape, seed):
    g = torch.Generator().manual_seed(seed)
    N, H, W = shape
    x = torch.randn(N, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci))
    b = torch.randn(co, generator=g) * 0.05
    gout = torch.randn(N, co, H, W, generator=g)
    return x, w, b, gout


@pytest.mark.parametrize("ci,co", R.PAIRS)
def test_conv_forward_alone(dev, ci, co):
    """|got - ref64| <= 5e-7 (|x| (*) |w| + |b|) elementwise: the guide's measured 3.5e-7 sum|a b| of a K = 4096 fp32 MFMA chain,
    K <= 4608 here."""
    from consistentnerf_amd import ops
    for shape in CONV_SHAPES:
        x, w, b, _ = _conv_case(ci, co, shape, 7)
        panel = ops.conv3x3_pack(w.to(dev))
        got = ops.conv3x3_forward(x.to(dev), panel, b.to(dev), co, relu=False)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
        err = (got.cpu().double() - ref).abs()
        print(f"conv fwd {ci}->{co} {shape}: max err / bound = {(err / (5e-7 * mag)).max().item():.3f}")
        assert got.shape == ref.shape and (err <= 5e-7 * mag).all()
        again = ops.conv3x3_forward(x.to(dev), panel, b.to(dev), co, relu=False)
        assert torch.equal(got, again)
        assert torch.equal(ops.conv3x3_forward(x.to(dev), panel, b.to(dev), co, relu=True), torch.relu(got))
        assert torch.equal(ops.conv3x3_forward(x.to(dev), panel, None, co, relu=False) + b.to(dev).reshape(1, -1, 1, 1), got)


@pytest.mark.parametrize("ci,co", R.PAIRS)
def test_conv_input_gradient_alone(dev, ci, co):
    """The same bound with the transposed sum, and the ReLU gate: gating inside the kernel == gating the gradient beforehand."""
    from consistentnerf_amd import ops
    for shape in CONV_SHAPES:
        x, w, b, gout = _conv_case(ci, co, shape, 11)
        panel_t = ops.conv3x3_pack(w.to(dev), transposed=True)
        got = ops.conv3x3_dgrad(gout.to(dev), panel_t, ci)
        ref = F.conv_transpose2d(gout.double(), w.double(), padding=1)
        mag = F.conv_transpose2d(gout.double().abs(), w.double().abs(), padding=1)
        err = (got.cpu().double() - ref).abs()
        print(f"conv dgrad {ci}->{co} {shape}: max err / bound = {(err / (5e-7 * mag + 1e-300)).max().item():.3f}")
        assert got.shape == x.shape and (err <= 5e-7 * mag).all()
        act = torch.relu(torch.randn(gout.shape, generator=torch.Generator().manual_seed(5))).to(dev)      # a stored post-ReLU output
        act[0, 0] = 0
        gated = ops.conv3x3_dgrad(gout.to(dev), panel_t, ci, gate=act)
        assert torch.equal(gated, ops.conv3x3_dgrad(gout.to(dev) * (act > 0), panel_t, ci))
        assert not torch.equal(gated, got)


def test_pool_forward_backward_equal_aten(dev):
    """torch.equal with ATen on the same device tensors: odd sides (the dropped row / column gets zero gradient), windows with ties
    (the first maximum in row-major order takes the gradient) and all-zero windows (post-ReLU maps are full of them)."""
    from consistentnerf_amd import ops
    g = torch.Generator().manual_seed(3)
    cases = [torch.randn(2, 5, 16, 16, generator=g), torch.randn(1, 3, 37, 51, generator=g), torch.randn(3, 2, 2, 3, generator=g),
             torch.randint(0, 3, (2, 4, 9, 12), generator=g).float(),                     # ties everywhere
             torch.relu(torch.randn(2, 6, 8, 8, generator=g) - 1.0),                      # mostly zero windows
             torch.zeros(1, 2, 4, 6)]
    tie = torch.zeros(1, 1, 4, 4)
    tie[0, 0, 0, 1] = tie[0, 0, 1, 0] = 2.0           # window (0, 0): two maxima, the first (row 0, column 1) wins
    tie[0, 0, 2, 2] = tie[0, 0, 3, 3] = -0.0          # window (1, 1): all zero (signed): element 0 wins
    cases.append(tie)
    for x in cases:
        x = x.to(dev).requires_grad_()
        ref = F.max_pool2d(x, 2, 2)
        gout = torch.randn(ref.shape, generator=g).to(dev)
        dref, = torch.autograd.grad(ref, x, gout)
        got = ops.maxpool2_forward(x.detach())
        dgot = ops.maxpool2_backward(x.detach(), gout)
        assert torch.equal(got, ref.detach()) and torch.equal(dgot, dref)
        H, W = x.shape[2:]
        if H % 2:
            assert (dgot[:, :, -1] == 0).all()
        if W % 2:
            assert (dgot[:, :, :, -1] == 0).all()
        add = torch.randn(x.shape, generator=g).to(dev)
        assert torch.equal(ops.maxpool2_backward(x.detach(), gout, add=add), add + dref)
    d = ops.maxpool2_backward(tie.to(dev), torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], device=dev))
    assert d[0, 0, 0, 1] == 1 and d[0, 0, 1, 0] == 0 and d[0, 0, 2, 2] == 4 and d[0, 0, 3, 3] == 0 and d.sum() == 10


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_head_forward_backward(dev, C):
    """One tap's head against float64.  The kernel sums in fp64 and rounds once: value within 2e-7 relative, gradient within 1e-6 of
    its largest element.  One constructed all-zero feature column in F0: the value follows the formula, the gradient there is
    exactly 0 (autograd gives NaN)."""
    from consistentnerf_amd import ops
    g = torch.Generator().manual_seed(C)
    N, H, W = 2, 17, 19                                                  # 323 pixels: two blocks of partial sums
    f0, f1 = torch.relu(torch.randn(N, C, H, W, generator=g)), torch.relu(torch.randn(N, C, H, W, generator=g) + 0.2)
    f0[0, :, 1, 2] = 0
    f1[1, :, 3, 4] = 0
    lin = torch.rand(C, generator=g) * (4.0 / C)
    gv = torch.rand(N, generator=g) + 0.5
    a = f0.double().requires_grad_()
    ref = R.head(a, f1.double(), lin.double())
    dref, = torch.autograd.grad((ref * gv.double()).sum(), a)
    assert torch.isnan(dref[0, :, 1, 2]).all()                           # the deliberate difference
    got = ops.lpips_head_forward(f0.to(dev), f1.to(dev), lin.to(dev))
    rel = ((got.cpu().double() - ref.detach()).abs() / ref.detach().abs()).max().item()
    print(f"head C={C}: value rel err {rel:.2e}")
    assert rel <= 2e-7
    assert torch.equal(got, ops.lpips_head_forward(f0.to(dev), f1.to(dev), lin.to(dev)))
    d = ops.lpips_head_backward(f0.to(dev), f1.to(dev), lin.to(dev), gv.to(dev)).cpu()
    assert torch.isfinite(d).all() and (d[0, :, 1, 2] == 0).all()
    keep = torch.ones(N, 1, H, W, dtype=torch.bool)
    keep[0, 0, 1, 2] = False
    dref0 = torch.where(keep, dref, torch.zeros_like(dref))
    e = (d.double() - dref0).abs().max().item() / dref0.abs().max().item()
    print(f"head C={C}: gradient err / max {e:.2e}")
    assert e <= 1e-6


@functools.lru_cache(maxsize=None)
def _e2e(shape):
    """One kept forward of the kernels at `shape` with its activations, and the float64 / float32 restatement (computed once)."""
    from consistentnerf_amd import ops
    N, _, H, W = shape
    x0, x1 = R.images(N, H, W, seed=H * W)
    model = _model()
    packed = model.packed(torch.device("cuda:0"))
    value, taps, ws, acts = ops.lpips_forward(x0.cuda(), x1.cuda(), packed, keep=True, want_taps=True, want_acts=True)
    v64, t64, _ = R.lpips(x0.double(), x1.double(), _wts())
    v32, t32, _ = R.lpips(x0, x1, _wts())
    return dict(x0=x0, x1=x1, value=value, taps=taps, acts=[a.cpu() for a in acts], v64=v64, t64=t64, v32=v32, t32=t32, packed=packed)


@pytest.mark.parametrize("shape", E2E_SHAPES)
def test_end_to_end_value(dev, shape):
    """Total and per-tap relative error against float64 <= 5e-6 (13 chained layers at the guide's 3.5e-7); identical bits call after
    call."""
    from consistentnerf_amd import ops
    c = _e2e(shape)
    rel = lambda a, b: ((a.cpu().double() - b).abs() / b.abs()).max().item()  # noqa: E731
    ev, et = rel(c["value"], c["v64"]), rel(c["taps"], c["t64"])
    rv, rt = rel(c["v32"], c["v64"]), rel(c["t32"], c["t64"])
    print(f"lpips {shape}: rel err total {ev:.2e} per-tap {et:.2e}   (restatement in float32: total {rv:.2e} per-tap {rt:.2e})")
    assert ev <= 5e-6 and et <= 5e-6
    v2, t2, _, _ = ops.lpips_forward(c["x0"].cuda(), c["x1"].cuda(), c["packed"], keep=True, want_taps=True)
    assert torch.equal(v2, c["value"]) and torch.equal(t2, c["taps"])
    assert len(c["acts"]) == 13 and c["acts"][12].shape == (2 * shape[0], 512, shape[2] // 16, shape[3] // 16)


@pytest.mark.parametrize("shape", E2E_SHAPES)
def test_end_to_end_gradient_on_the_kernels_branch(dev, shape):
    """max|dX - dX64| <= 1e-5 max|dX64| (criterion a6) with the float64 restatement forced onto the kernel's ReLU masks and pool
    choices; w.r.t. in0, w.r.t. in1, and both at once."""
    c = _e2e(shape)
    model = _model()
    N = shape[0]
    gv = torch.rand(N, generator=torch.Generator().manual_seed(9)) + 0.5
    force = R.branches_of(c["acts"])
    a, b = c["x0"].double().requires_grad_(), c["x1"].double().requires_grad_()
    v64, _, _ = R.lpips(a, b, _wts(), force=force)
    da64, db64 = torch.autograd.grad((v64 * gv.double()).sum(), (a, b))
    a32, b32 = c["x0"].clone().requires_grad_(), c["x1"].clone().requires_grad_()
    v32, _, _ = R.lpips(a32, b32, _wts(), force=force)
    da32, = torch.autograd.grad((v32 * gv).sum(), a32)
    err = lambda g, r: (g.cpu().double() - r).abs().max().item() / r.abs().max().item()  # noqa: E731

    def run(req0, req1):
        x0, x1 = c["x0"].to(dev).requires_grad_(req0), c["x1"].to(dev).requires_grad_(req1)
        v = model(x0, x1)
        assert v.shape == (N, 1, 1, 1) and torch.equal(v.detach().reshape(-1), c["value"])
        (v.reshape(-1) * gv.to(dev)).sum().backward()
        return x0.grad, x1.grad
    d0, none = run(True, False)
    assert none is None
    e0 = err(d0, da64)
    none, d1 = run(False, True)
    assert none is None
    e1 = err(d1, db64)
    b0, b1 = run(True, True)
    print(f"lpips grad {shape}: in0 {e0:.2e} in1 {e1:.2e}   (ATen float32 on the same branch: {err(da32, da64):.2e})")
    assert torch.isfinite(d0).all() and torch.isfinite(d1).all()
    assert e0 <= 1e-5 and e1 <= 1e-5
    assert torch.equal(b0, d0) and torch.equal(b1, d1)


def test_public_surface(dev, tmp_path, monkeypatch):
    from consistentnerf_amd import io_formats, ops
    from consistentnerf_amd.run_nerf_view import patch_lpips
    import consistentnerf_amd.lpips as L
    model = _model()
    c = _e2e((2, 3, 16, 21))
    x0, x1 = c["x0"].to(dev), c["x1"].to(dev)
    # the no-grad path walks the batch image by image through two buffers: the same bits as the kept-activation path
    with torch.no_grad():
        v, taps = model(x0, x1, retPerLayer=True)
    assert v.shape == (2, 1, 1, 1) and torch.equal(v.reshape(-1), c["value"])
    assert len(taps) == 5 and all(t.shape == (2, 1, 1, 1) for t in taps) and torch.equal(torch.stack(taps).reshape(5, 2), c["taps"])
    vs, ts, ws, _ = ops.lpips_forward(x0, x1, c["packed"], keep=False, want_taps=True)
    assert ws is None and torch.equal(vs, c["value"]) and torch.equal(ts, c["taps"])
    # normalize=True: inputs in [0, 1]
    vn = model((x0 + 1) / 2, (x1 + 1) / 2, normalize=True)
    assert torch.allclose(vn.reshape(-1), c["value"], rtol=1e-4, atol=0)
    assert torch.equal(vn, model(2 * ((x0 + 1) / 2) - 1, 2 * ((x1 + 1) / 2) - 1))
    assert float(model(x0, x0).abs().max()) == 0.0
    # img2lpips, unmasked and masked (V:2055-2076)
    rs = np.random.RandomState(4)
    pred, gt = rs.uniform(size=(2, 24, 20, 3)).astype(np.float32), rs.uniform(size=(2, 24, 20, 3)).astype(np.float32)
    mask = rs.uniform(size=(2, 24, 20)) > 0.3
    w = _wts()
    to = lambda a: ((torch.from_numpy(a) - 0.5) * 2.).permute(0, 3, 1, 2).double()  # noqa: E731
    ref = R.lpips(to(gt), to(pred), w)[0].mean().item()
    got = io_formats.img2lpips(pred, gt, model)
    assert got.dim() == 0 and abs(got.item() - ref) <= 5e-6 * ref
    m = torch.from_numpy(mask).unsqueeze(1).double()
    refm = R.lpips(to(gt) * m + (1 - m), to(pred) * m + (1 - m), w)[0].mean().item()
    gotm = io_formats.img2lpips(torch.from_numpy(pred), torch.from_numpy(gt), model, mask=mask)
    assert abs(gotm.item() - refm) <= 5e-6 * refm and gotm.item() != got.item()
    # patch_lpips: V:1699-1706 + V:1721 on 4 patches of a 1100-ray batch, the gradient reaching rgb
    g = torch.Generator().manual_seed(6)
    tgt = torch.rand(1100, 3, generator=g)
    rgb = (tgt + 0.1 * torch.randn(1100, 3, generator=g)).clamp(0, 1)
    rgb_d = rgb.to(dev).requires_grad_()
    val = patch_lpips(rgb_d, tgt.to(dev), model)
    val[0].backward()
    tp = lambda t: ((t[:1024].reshape(4, 16, 16, 3) - 0.5) * 2.).permute(0, 3, 1, 2)  # noqa: E731
    r64 = R.lpips(tp(rgb.double()), tp(tgt.double()), w)[0].sum().item() / 4
    assert val.shape == (1,) and abs(val.item() - r64) <= 5e-6 * r64
    assert torch.isfinite(rgb_d.grad).all() and (rgb_d.grad[1024:] == 0).all() and float(rgb_d.grad[:1024].abs().max()) > 0
    # ... and it is the network's own input gradient (checked above) carried back through (x - 0.5) * 2, the permute and the / 4
    p = tp(rgb.to(dev)).contiguous().requires_grad_()
    model(p, tp(tgt.to(dev)).contiguous()).sum().backward()
    assert torch.allclose(rgb_d.grad[:1024], (p.grad.permute(0, 2, 3, 1).reshape(1024, 3) / 4) * 2., rtol=1e-6, atol=0)
    # the module stands in for the package, with a weights file named by the environment
    path = tmp_path / "vgg_lpips.pth"
    torch.save(R.package_state_dict(w, lins_prefix=True), path)
    monkeypatch.setenv("CNERF_LPIPS_WEIGHTS", str(path))
    monkeypatch.setitem(sys.modules, "lpips", L)
    import lpips
    lpips_fn = lpips.LPIPS(net="vgg").to(torch.device("cuda", torch.cuda.current_device()))
    with torch.no_grad():
        assert torch.equal(lpips_fn(x0, x1).reshape(-1), c["value"])
