"""Camera gradients on the folded training step, render_loss(rows=...).

Kernel level: cnerf_mlp_input_grad_pair, cnerf_rays_input_grad_pair and cnerf_composite_norm_grad_pair bit for bit against the
single kernels they pair up, repeated calls, NaN guard bands.  The whole chain: CameraPoses + CameraIntrinsics -> pose.camera_rows ->
run_nerf.render_loss(rows=) -> backward, rows.grad against the float64 oracle on the kernel's ReLU masks and fine depths, the camera
gradients bit for bit against the camera backward kernels, the parameter gradients and the loss bit for bit against the step on
detached rows, and the entry points the step calls."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _camera_ref as CR
import _inputs as I
from oracle import nerf_oracle as O
from test_gpu_camera_grads import WB, WH, WK, WW, _chain_camera
from test_gpu_input_grads import _check, _err
from test_gpu_parity import T, _kwargs, check_flips, dev, make_model, relu_masks  # noqa: F401  (dev: the device fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, NAN = 64, float("nan")
NC, NF = 16, 8
PAIR_OPS = ("mlp_input_grad_pair", "rays_input_grad_pair", "composite_norm_grad_pair")


# ------------------------------------------------------------------------------------------------ kernel level
# (coarse, fine) as (D, W, use_viewdirs, output_ch)
LEVEL_PAIRS = {"D4W128_D4W128": ((4, 128, True, 4), (4, 128, True, 4)),
               "D2W64_D8W256skip": ((2, 64, True, 4), (8, 256, True, 4)),
               "novd_D4W128_D4W128": ((4, 128, False, 5), (4, 128, False, 5))}
MLP_SHAPES = [(37, 16, 24), (1, 1, 1), (24, 16, 32)]     # both last tiles ragged (M = 592 / 888); one point each; whole tiles
S_PAIRS = [(1, 192), (63, 64), (64, 65), (65, 1), (192, 63), (64, 64)]     # {1, 63, 64, 65, 192} per level, mixed
B_SET = (1, 4, 5)


def _level(dev, net, seed, rays, S):
    """One level behind its dgrad: forward on the ray rows at random depths, a random d_raw, cnerf_mlp_dgrad into its own workspace."""
    from consistentnerf_amd import ops, run_nerf as R
    D, W, vd, och = net
    model, _ = make_model(D, W, vd, och, seed, dev)
    spec, packed, B = model.spec(), R._packed(model), rays.shape[0]
    rs = np.random.RandomState(seed)
    z = T(np.sort(rs.uniform(2.0, 6.0, size=(B, S)), -1).astype(np.float32), dev)
    raw, stash = ops.mlp_forward(spec, packed, B, S, rays=rays, z=z, want_stash=True)
    d_raw = T(rs.normal(size=tuple(raw.shape)).astype(np.float32), dev)
    ws = ops.mlp_bwd_workspace(spec, B, S, dev)
    ops.mlp_dgrad(spec, packed, d_raw, B, S, stash, ws)
    return dict(spec=spec, packed=packed, B=B, S=S, stash=stash, ws=ws, vd=vd, model=model)


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("B,S0,S1", MLP_SHAPES)
@pytest.mark.parametrize("pair", list(LEVEL_PAIRS))
def test_mlp_input_grad_pair_equals_two_single_calls(dev, pair, B, S0, S1):
    """One grid over both levels against cnerf_mlp_input_grad on each level's workspace: d_pts and d_dirs_pt of both, bit for bit,
    twice (the same bits)."""
    from consistentnerf_amd import ops
    n0, n1 = LEVEL_PAIRS[pair]
    rays = T(I.ray_batch(B, seed=3)[:, :11 if n0[2] else 8].copy(), dev)
    a, b = _level(dev, n0, 61, rays, S0), _level(dev, n1, 62, rays, S1)
    want = [ops.mlp_input_grad(l["spec"], l["packed"], B, l["S"], l["stash"], l["ws"], want_dirs=l["vd"]) for l in (a, b)]
    args = (a["spec"], a["packed"], B, S0, a["stash"], a["ws"], b["spec"], b["packed"], B, S1, b["stash"], b["ws"])
    for _ in range(2):
        got = ops.mlp_input_grad_pair(*args, want_dirs=a["vd"])
        for lv in (0, 1):
            assert got[lv][0].shape == (B * (S0, S1)[lv], 3) and torch.isfinite(got[lv][0]).all() and got[lv][0].any()
            assert torch.equal(got[lv][0], want[lv][0]), f"d_pts of level {lv}"
            assert _same(got[lv][1], want[lv][1]), f"d_dirs_pt of level {lv}"
            assert (got[lv][1] is not None) == a["vd"]
    if a["vd"]:     # without the view-direction outputs: the positions' bits do not move
        got = ops.mlp_input_grad_pair(*args, want_dirs=False)
        assert got[0][1] is None and got[1][1] is None and torch.equal(got[0][0], want[0][0]) and torch.equal(got[1][0], want[1][0])


def _ray_sums_inputs(dev, B, S, seed, dirs):
    rs = np.random.RandomState(seed)
    d_pts = T(rs.normal(size=(B * S, 3)).astype(np.float32), dev)
    d_dirs = T(rs.normal(size=(B * S, 3)).astype(np.float32), dev) if dirs else None
    z = T(np.sort(rs.uniform(0.0, 6.0, size=(B, S)), -1).astype(np.float32), dev)
    return d_pts, d_dirs, z


@pytest.mark.parametrize("stride", [8, 11])
def test_rays_input_grad_pair_equals_the_sum_of_two(dev, stride):
    """Every (S0, S1) of S_PAIRS x B in {1, 4, 5}: the pair's [B, stride] result equals rays_input_grad(level 0) + rays_input_grad(level 1)
    bit for bit (columns 6:8 zero, the view-direction sums in the last three columns at stride 11), twice."""
    from consistentnerf_amd import ops
    for S0, S1 in S_PAIRS:
        for B in B_SET:
            p0, v0, z0 = _ray_sums_inputs(dev, B, S0, 100 + S0 + B, stride == 11)
            p1, v1, z1 = _ray_sums_inputs(dev, B, S1, 200 + S1 + B, stride == 11)
            want = ops.rays_input_grad(p0, v0, z0, B, S0, ray_stride=stride) + ops.rays_input_grad(p1, v1, z1, B, S1, ray_stride=stride)
            got = ops.rays_input_grad_pair(p0, v0, z0, p1, v1, z1, stride)
            assert got.shape == (B, stride) and torch.equal(got, want), (S0, S1, B)
            assert not got[:, 6:8].any() and got[:, 0:6].abs().min() > 0 and (stride == 8 or got[:, 8:11].abs().min() > 0)
            assert torch.equal(ops.rays_input_grad_pair(p0, v0, z0, p1, v1, z1, stride), got)
    # rows of width 11 whose levels carry no view-direction gradient: zeros there
    got = ops.rays_input_grad_pair(p0, None, z0, p1, None, z1, 11)
    assert torch.equal(got[:, 0:6], want[:, 0:6]) and not got[:, 6:].any()


def _norm_inputs(dev, B, S, ch, seed, noise):
    rs = np.random.RandomState(seed)
    d_raw = T(rs.normal(size=(B, S, ch)).astype(np.float32), dev)
    raw = T(rs.normal(size=(B, S, ch)).astype(np.float32), dev)
    nz = T(rs.normal(size=(B, S)).astype(np.float32), dev) if noise else None
    return d_raw, raw, nz


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("stride", [8, 11])
def test_composite_norm_grad_pair_equals_the_sum_of_two(dev, stride, noise):
    """The same S / B sets, raw of 4 and of 5 channels: [B, stride] with columns 3:6 = composite_norm_grad(level 0) +
    composite_norm_grad(level 1) bit for bit and every other column zero, twice."""
    from consistentnerf_amd import ops
    for S0, S1 in S_PAIRS:
        for B in B_SET:
            rays = T(I.ray_batch(B, seed=S0 + B)[:, :stride].copy(), dev)
            a, b = _norm_inputs(dev, B, S0, 4, 300 + S0 + B, noise), _norm_inputs(dev, B, S1, 5, 400 + S1 + B, noise)
            want = ops.composite_norm_grad(*a, rays) + ops.composite_norm_grad(*b, rays)
            got = ops.composite_norm_grad_pair(*a, *b, rays)
            assert got.shape == (B, stride) and torch.equal(got, want), (S0, S1, B)
            assert got[:, 3:6].abs().min() > 0 and not got[:, 0:3].any() and not got[:, 6:].any()
            assert torch.equal(ops.composite_norm_grad_pair(*a, *b, rays), got)


def test_guarded_buffers(dev):
    """The three entry points on outputs of exactly their size inside NaN guard bands (64 floats each side), at the ragged shape and
    at S = 65 / 192: the guards stay NaN, every element between them is written and finite, and the results are the ops wrappers'."""
    from consistentnerf_amd import _lib, ops
    from consistentnerf_amd.ops import _p, _stream
    import ctypes as C
    lib = _lib.load()

    def guarded(n):
        buf = torch.full((GUARD + n + GUARD,), NAN, device=dev)
        return buf, buf[GUARD:GUARD + n]

    def intact(buf, n, what):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{what}: a write outside the buffer"
        assert torch.isfinite(buf[GUARD:GUARD + n]).all(), f"{what}: an element that was not written"

    B, S0, S1 = 37, 16, 24
    rays = T(I.ray_batch(B, seed=3), dev)
    a, b = _level(dev, (2, 64, True, 4), 61, rays, S0), _level(dev, (8, 256, True, 4), 62, rays, S1)
    outs = [guarded(B * S * 3) for S in (S0, S0, S1, S1)]
    n0, n1 = a["spec"].c(), b["spec"].c()
    _lib.check(lib.cnerf_mlp_input_grad_pair(C.byref(n0), _p(a["packed"]), B, S0, _p(a["stash"]), _p(a["ws"]), _p(outs[0][1]), _p(outs[1][1]),
                                             C.byref(n1), _p(b["packed"]), B, S1, _p(b["stash"]), _p(b["ws"]), _p(outs[2][1]), _p(outs[3][1]),
                                             _stream()), "cnerf_mlp_input_grad_pair")
    for (buf, _), S, what in zip(outs, (S0, S0, S1, S1), ("d_pts0", "d_dirs_pt0", "d_pts1", "d_dirs_pt1")):
        intact(buf, B * S * 3, what)
    want = ops.mlp_input_grad_pair(a["spec"], a["packed"], B, S0, a["stash"], a["ws"], b["spec"], b["packed"], B, S1, b["stash"], b["ws"], True)
    for (_, got), w in zip(outs, (want[0][0], want[0][1], want[1][0], want[1][1])):
        assert torch.equal(got.view(-1, 3), w)
    for B, S0, S1, stride in ((5, 65, 192, 11), (5, 192, 1, 8), (1, 63, 64, 11)):
        p0, v0, z0 = _ray_sums_inputs(dev, B, S0, 7, stride == 11)
        p1, v1, z1 = _ray_sums_inputs(dev, B, S1, 8, stride == 11)
        buf, out = guarded(B * stride)
        _lib.check(lib.cnerf_rays_input_grad_pair(_p(p0), _p(v0), _p(z0), S0, _p(p1), _p(v1), _p(z1), S1, B, _p(out), stride, _stream()),
                   "cnerf_rays_input_grad_pair")
        intact(buf, B * stride, "d_rays (ray sums)")
        assert torch.equal(out.view(B, stride), ops.rays_input_grad_pair(p0, v0, z0, p1, v1, z1, stride))
        rows = T(I.ray_batch(B, seed=2)[:, :stride].copy(), dev)
        x, y = _norm_inputs(dev, B, S0, 4, 9, True), _norm_inputs(dev, B, S1, 5, 10, False)
        buf, out = guarded(B * stride)
        _lib.check(lib.cnerf_composite_norm_grad_pair(_p(x[0]), _p(x[1]), 4, _p(x[2]), S0, _p(y[0]), _p(y[1]), 5, _p(y[2]), S1, _p(rows), stride, B,
                                                      _p(out), _stream()), "cnerf_composite_norm_grad_pair")
        intact(buf, B * stride, "d_rays (norm term)")
        assert torch.equal(out.view(B, stride), ops.composite_norm_grad_pair(*x, *y, rows))


# ------------------------------------------------------------------------------------------------ the whole chain
def _target():
    return np.random.RandomState(41).uniform(size=(WB, 3)).astype(np.float32)


def _nets(dev, vd, D=4, Wn=128, owned=True, frozen=False, prec=None, one_level=False):
    """Two networks (seeds 31 / 32, as the chain tests of the camera gradients), owned by a FusedAdam unless told otherwise."""
    from consistentnerf_amd.optim import FusedAdam
    (coarse, sdc), (fine, sdf) = make_model(D, Wn, vd, 5, 31, dev), make_model(D, Wn, vd, 5, 32, dev)
    if one_level:
        fine, sdf = None, None
    nets = [m for m in (coarse, fine) if m is not None]
    for m in nets:
        if prec is not None:
            m.training_precision = prec
        if frozen:
            for p in m.parameters():
                p.requires_grad_(False)
    opt = None
    if owned and not frozen:
        opt = FusedAdam([p for m in nets for p in m.parameters()], lr=5e-4)
        opt.zero_grad()
    return coarse, fine, sdc, sdf, opt


def _rows(dev, vd, grad=True):
    from consistentnerf_amd.pose import camera_rows
    poses, intr, coords, view = _chain_camera(dev)
    c2w, K = poses(), intr()
    assert CR.min_abs_dz(WH, WW, K.detach().cpu().tolist(), c2w.detach().cpu().numpy(), coords.cpu(), view.cpu()) >= 0.85
    K.retain_grad()
    rows = camera_rows(WH, WW, K, c2w, coords, view, near=0., far=1., use_viewdirs=vd, ndc=True)
    assert rows.shape == (WB, 11 if vd else 8) and rows.requires_grad
    if not grad:
        return rows.detach(), None
    rows.retain_grad()
    return rows, (poses, intr, coords, view, c2w, K)


def _render_loss(dev, rows, coarse, fine, vd, chunk=4096, nf=NF, perturb=0.0, noise=0.0, target=None):
    from consistentnerf_amd import run_nerf as R
    tgt = T(_target(), dev) if target is None else target
    return R.render_loss(WH, WW, WK, tgt, chunk, rows=rows, use_viewdirs=vd, ndc=True, near=0., far=1.,
                         **_kwargs(coarse, fine, NC, nf if fine is not None else 0, perturb, False, noise, False))


_REF = {}


def _reference(dev, vd, rows, D=4, Wn=128, nf=NF, prec=None):
    """(float64, float32) oracle gradients of img2mse(rgb_map, target) (+ img2mse(rgb0, target)) w.r.t. the rows, on the kernel's ReLU
    masks and fine depths — built the way test_gpu_camera_grads._chain_reference is; once per case."""
    key = (vd, D, Wn, nf, prec)
    if key in _REF:
        return _REF[key]
    from consistentnerf_amd import run_nerf_view as V
    coarse, fine, sdc, sdf, _ = _nets(dev, vd, D, Wn, owned=False, prec=prec, one_level=nf == 0)
    ret = V.render_rays(rows.detach().clone(), retraw=True, _debug=True, **_kwargs(coarse, fine, NC, nf, 0.0, False, 0.0, False))
    if nf:
        masks_c = relu_masks(ret["_raw_coarse"].grad_fn.stash, WB * NC, D, Wn, vd)
        masks_f = relu_masks(ret["raw"].grad_fn.stash, WB * (NC + nf), D, Wn, vd)
    else:
        masks_c, masks_f = relu_masks(ret["raw"].grad_fn.stash, WB * NC, D, Wn, vd), None
    z_fine = ret["_z_vals"].detach().cpu()
    rows_cpu, tgt = rows.detach().cpu(), _target()

    def run(dtype, flips):
        r = rows_cpu.to(dtype).clone().requires_grad_(True)
        out = O.render_rays(r, {k: T(v).to(dtype) for k, v in sdc.items()}, None if sdf is None else {k: T(v).to(dtype) for k, v in sdf.items()},
                            O.NetCfg(D, Wn, use_viewdirs=vd, output_ch=5), O.RenderCfg(NC, nf, 0.0, False, False, 0.0),
                            u=torch.linspace(0.0, 1.0, nf, dtype=dtype).expand(WB, nf) if nf else None,
                            z_fine=z_fine.to(dtype) if nf else None, masks_coarse=masks_c, masks_fine=masks_f, flips=flips)
        t = T(tgt).to(dtype)
        loss = ((out["rgb_map"] - t) ** 2).mean()
        if nf:
            loss = loss + ((out["rgb0"] - t) ** 2).mean()
        loss.backward()
        return r.grad.double()

    flips32, flips64 = [], []
    g64, g32 = run(torch.float64, flips64), run(torch.float32, flips32)
    # (the tolerances of test_gpu_camera_grads._chain_reference: the float32 oracle sees the kernel's positions, the float64 one the
    # unrounded o + d z, which layer 0 of the 2^9-frequency encoding amplifies)
    check_flips(flips32)
    xmax = float((rows_cpu[:, None, 0:3] + rows_cpu[:, None, 3:6] * z_fine[:, :, None]).abs().max())
    dx = 1.5 * 2.0 ** (np.floor(np.log2(xmax)) - 23)
    check_flips(flips64, tol=1e-5 + float(np.abs(sdc["pts_linears.0.weight"]).max()) * (6 * 1023 + 3) * dx)
    _REF[key] = (g64, g32)
    return _REF[key]


def _check_rows(tag, g, ref, vd):
    g64, g32 = ref
    assert g is not None and torch.isfinite(g).all() and g[:, 0:6].abs().max() > 0 and not g[:, 6:8].any()
    _check(f"{tag} rows.grad, origins", g[:, 0:3], g64[:, 0:3], g32[:, 0:3])
    _check(f"{tag} rows.grad, directions", g[:, 3:6], g64[:, 3:6], g32[:, 3:6])
    if vd:
        _check(f"{tag} rows.grad, view directions", g[:, 8:11], g64[:, 8:11], g32[:, 8:11])


def _spy(monkeypatch, names=PAIR_OPS):
    """Record what the named ops functions return (they still run)."""
    from consistentnerf_amd import ops
    seen = {n: [] for n in names}
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _n=n, _r=real, **k: (seen[_n].append(_r(*a, **k)), seen[_n][-1])[1])
    return seen


@pytest.mark.parametrize("vd", [True, False])
def test_pose_step_on_the_folded_route(dev, vd, monkeypatch):
    """CameraPoses (3 views) + CameraIntrinsics -> camera_rows(ndc=True) of 37 pixels -> run_nerf.render_loss(rows=) on two D4 / W128
    networks owned by a FusedAdam, 16 + 8 samples, a seeded target -> backward.  rows.grad against float64 (bound max(1e-5, 4 x the
    float32 oracle's error)); poses.rot.grad / poses.trans.grad / K.grad bit for bit the camera backward kernels on the retained
    rows.grad; rows.grad bit for bit the sum of what composite_norm_grad_pair and rays_input_grad_pair returned.  Without view
    directions, rows.grad[:, 3:6] minus the norm pair's part must MISS the bound (the analogous single-level case measured 3.1e-3).
    Measured on the MI355X: err 9.6e-6 / 6.4e-6 / 3.0e-6 (origins / directions / view directions; bounds 3.7e-5 / 2.6e-5 / 1.2e-5) with
    view directions, 1.2e-5 / 7.5e-6 (bounds 4.6e-5 / 2.9e-5) without, the float32 oracle within 4 % of the same figures; with the
    norm-pair term taken out 4.1e-3."""
    from consistentnerf_amd import ops, run_nerf as R
    coarse, fine, _, _, opt = _nets(dev, vd)
    rows, (poses, intr, coords, view, c2w, K) = _rows(dev, vd)
    seen = _spy(monkeypatch)
    loss = _render_loss(dev, rows, coarse, fine, vd)[0]
    R.backward(loss)
    g = rows.grad
    ref = _reference(dev, vd, rows)
    _check_rows("folded", g, ref, vd)
    assert [len(seen[n]) for n in PAIR_OPS] == [1, 1, 1]
    norm, sums = seen["composite_norm_grad_pair"][0], seen["rays_input_grad_pair"][0]
    assert torch.equal(g, norm + sums) and norm[:, 3:6].any()
    d_c2w, d_K = ops.camera_rows_bwd(g, WH, WW, K.detach(), c2w.detach().reshape(3, 12), coords, view, vd, True)
    want_rot, want_trans = ops.pose_compose_bwd(poses.c2w0, poses.rot.detach(), d_c2w)
    for name, got, want in (("rot", poses.rot.grad, want_rot), ("trans", poses.trans.grad, want_trans), ("K", K.grad, d_K)):
        assert got is not None and torch.isfinite(got).all() and got.any(), name
        assert torch.equal(got, want), name
    assert float(opt.flat_grad.abs().max()) > 0
    if not vd:      # must fail: the directions without the norm term
        g64, g32 = ref
        err, bound = _err(g[:, 3:6] - norm[:, 3:6], g64[:, 3:6]), max(1e-5, 4.0 * _err(g32[:, 3:6], g64[:, 3:6]))
        print(f"  rows.grad directions with the norm-pair term taken out: err {err:.3e} (bound {bound:.3e})")
        assert err > bound


def _recording():
    spec = importlib.util.spec_from_file_location("step_fingerprint", os.path.join(ROOT, "scripts", "step_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    return fp.recording


@pytest.mark.parametrize("vd", [True, False])
def test_parameter_gradients_and_launch_sequence(dev, vd, monkeypatch):
    """The pose step against the same step on rows.detach(): the flat gradient of the FusedAdam and the loss bit for bit; the entry
    points of the pose step are the detached step's plus exactly the three pair launches and the two camera launches, with one
    cnerf_mlp_dgrad_pair, one cnerf_mlp_wgrad_pair and none of the single input-gradient launches; the detached step calls none of the
    new ops functions."""
    from consistentnerf_amd import ops, run_nerf as R
    recording = _recording()
    out = {}
    for tag in ("pose", "detached"):
        coarse, fine, _, _, opt = _nets(dev, vd)
        rows, cams = _rows(dev, vd, grad=tag == "pose")
        calls = []
        if tag == "detached":
            for n in PAIR_OPS + ("mlp_input_grad", "rays_input_grad", "composite_norm_grad"):
                monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: calls.append(_n))
        with recording() as names:
            loss = _render_loss(dev, rows, coarse, fine, vd)[0]
            R.backward(loss)
        assert not calls, calls
        out[tag] = (loss.detach().clone(), opt.flat_grad.clone(), list(names))
    assert torch.equal(out["pose"][0], out["detached"][0]), "the loss depends on whether the rows require grad"
    assert float(out["detached"][1].abs().max()) > 0 and torch.equal(out["pose"][1], out["detached"][1]), \
        "parameter gradients depend on whether the rows require grad"
    pose, det = out["pose"][2], out["detached"][2]
    print("  pose step:", " ".join(pose))
    extra = list(pose)
    for n in det:
        extra.remove(n)
    assert sorted(extra) == sorted(["cnerf_composite_norm_grad_pair", "cnerf_mlp_input_grad_pair", "cnerf_rays_input_grad_pair",
                                    "cnerf_camera_rows_bwd", "cnerf_pose_compose_bwd"]), extra
    assert [n for n in pose if n not in extra] == det
    assert pose.count("cnerf_mlp_dgrad_pair") == 1 and pose.count("cnerf_mlp_wgrad_pair") == 1
    assert not {"cnerf_mlp_input_grad", "cnerf_rays_input_grad", "cnerf_composite_norm_grad", "cnerf_mlp_dgrad", "cnerf_mlp_wgrad"} & set(pose)
    at = [pose.index(n) for n in ("cnerf_composite_norm_grad_pair", "cnerf_mlp_dgrad_pair", "cnerf_mlp_wgrad_pair", "cnerf_mlp_input_grad_pair",
                                  "cnerf_rays_input_grad_pair", "cnerf_camera_rows_bwd")]
    assert at == sorted(at), pose


def test_no_host_synchronisation(dev):
    """The pose step, forward and backward, under torch.cuda.set_sync_debug_mode("error")."""
    from consistentnerf_amd import run_nerf as R
    coarse, fine, _, _, opt = _nets(dev, True)
    tgt = T(_target(), dev)
    rows, _ = _rows(dev, True)
    R.backward(_render_loss(dev, rows, coarse, fine, True, target=tgt)[0])      # (first use: packing, caches)
    opt.zero_grad()
    rows, _ = _rows(dev, True)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = _render_loss(dev, rows, coarse, fine, True, target=tgt)[0]
        R.backward(loss)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and torch.isfinite(rows.grad).all()


ROUTES = {"tensor_route": dict(owned=False), "frozen": dict(frozen=True), "one_level": dict(one_level=True), "chunk_16": dict(chunk=16),
          "bf16x3_D8W256": dict(D=8, Wn=256, prec="bf16x3")}


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_other_routes_through_render_loss(dev, route, monkeypatch):
    """render_loss(rows=) where the pair does not apply or runs behind other kernels, each against float64 at the same bound: plain
    nn.Parameters (the tensor route: the levels singly), frozen networks (the dgrad alone), N_importance = 0, chunk 16 (three slices
    through batchify_rays + the loss lines), training_precision = "bf16x3" on D8 / W256 (the pair behind cnerf_mlp_dgrad_bf_pair)."""
    from consistentnerf_amd import run_nerf as R
    cfg = dict(ROUTES[route])
    chunk, D, Wn, prec = cfg.pop("chunk", 4096), cfg.get("D", 4), cfg.get("Wn", 128), cfg.get("prec")
    one = cfg.get("one_level", False)
    coarse, fine, _, _, opt = _nets(dev, True, **cfg)
    rows, _ = _rows(dev, True)
    seen = _spy(monkeypatch)
    recording = _recording()
    with recording() as names:
        loss = _render_loss(dev, rows, coarse, fine, True, chunk=chunk)[0]
        R.backward(loss)
    _check_rows(route, rows.grad, _reference(dev, True, rows, D, Wn, 0 if one else NF, prec), True)
    paired = route == "bf16x3_D8W256"
    # (chunk 16: no folded node, but each of the three slices still pairs its two levels' backward and input-gradient launches)
    assert [len(seen[n]) for n in PAIR_OPS] == {"bf16x3_D8W256": [1, 1, 1], "one_level": [0, 0, 0], "chunk_16": [3, 3, 0]}.get(route, [0, 0, 1])
    if paired:
        assert names.count("cnerf_mlp_dgrad_bf_pair") == 1 and names.count("cnerf_mlp_wgrad_bf_pair") == 1
    if route == "frozen":
        assert all(p.grad is None for p in coarse.parameters()) and not any("wgrad" in n for n in names)
    elif route == "tensor_route":
        assert coarse.kernel_tensors()[0].grad is not None and names.count("cnerf_mlp_input_grad") == 2
    else:
        assert float(opt.flat_grad.abs().max()) > 0


def test_random_streams(dev, monkeypatch):
    """perturb = 1, raw_noise_std = 1, the generator re-seeded identically before each call: render_loss(rows=) against
    batchify_rays(rows) + img2mse(rgb) + img2mse(rgb0) with the levels NOT paired (run_nerf.MERGE_BWD off): the launch sequence the
    camera gradients had before — each level's own dgrad + wgrad, the single cnerf_mlp_input_grad / cnerf_rays_input_grad /
    cnerf_composite_norm_grad, ATen adds — so the reference shares none of the pair kernels (asserted).  The loss bit for bit;
    rows.grad within 1e-5 of max|g| (two fp32 evaluations of the same sums in different association); the flat gradient bit for bit.
    Measured on the MI355X: max|d rows.grad| 1.5e-8 = 3.4e-8 of max|g|."""
    from consistentnerf_amd import run_nerf as R
    from consistentnerf_amd.run_nerf_helpers import img2mse
    got = {}
    tgt = T(_target(), dev)
    seen = _spy(monkeypatch)
    for tag in ("folded", "lines"):
        coarse, fine, _, _, opt = _nets(dev, True)
        rows, _ = _rows(dev, True)
        torch.manual_seed(77)
        if tag == "folded":
            loss = _render_loss(dev, rows, coarse, fine, True, perturb=1.0, noise=1.0, target=tgt)[0]
            loss.backward()
            assert [len(seen[n]) for n in PAIR_OPS] == [1, 1, 1]
        else:
            monkeypatch.setattr(R, "MERGE_BWD", False)
            out = R.batchify_rays(rows, 4096, **_kwargs(coarse, fine, NC, NF, 1.0, False, 1.0, False))
            loss = img2mse(out["rgb_map"], tgt) + img2mse(out["rgb0"], tgt)
            loss.backward()
            assert [len(seen[n]) for n in PAIR_OPS] == [1, 1, 1], "the reference route ran a pair kernel"
        got[tag] = (loss.detach().clone(), rows.grad.clone(), opt.flat_grad.clone())
    assert torch.equal(got["folded"][0], got["lines"][0])
    scale = float(got["lines"][1].abs().max())
    diff = float((got["folded"][1] - got["lines"][1]).abs().max())
    print(f"  rows.grad folded vs unpaired lines under perturb / noise: max|d| {diff:.3e} = {diff / scale:.3e} of max|g| {scale:.3e}")
    assert scale > 0 and diff <= 1e-5 * scale
    assert torch.equal(got["folded"][2], got["lines"][2])


@pytest.mark.parametrize("form", ["default", "softlp"])
def test_the_consistentnerf_step(dev, form, monkeypatch):
    """run_nerf_view.render_loss(rows=, mask=, depth_prior=) on 37 rays with a mixed 0 / 1 mask, the default forms and rgb_form =
    "softlp", against the maps of batchify_rays(rows) + the docstring's loss lines written here in torch (hardmask_losses /
    img2mse_softLpmask per level, rgb_w * img + depth_w * depth, fine + coarse), the levels NOT paired (run_nerf.MERGE_BWD off), so
    the reference shares neither the folded node, nor the `rows=` entry, nor a pair kernel (asserted).  rows.grad within 1e-5 of
    max|g|; the loss and the parameter gradients as the folded tests of the forms hold them against their lines
    (tests/test_gpu_lossforms.py): loss 3e-7 relative and gradients bit for bit (default), loss 1e-6 and gradients 2e-6 of their
    largest (softlp: powf against ATen's pow).
    Measured on the MI355X: rows.grad 2.9e-8 (default) / 5.0e-8 (softlp) of max|g|; the losses equal to every digit printed."""
    from consistentnerf_amd import run_nerf as R, run_nerf_view as V
    rs = np.random.RandomState(43)
    tgt = T(_target(), dev)
    mask = T((rs.uniform(size=(WB,)) < 0.55).astype(np.float32), dev)
    prior = T(rs.uniform(0.1, 0.9, size=(WB,)).astype(np.float32), dev)
    assert 0 < int(mask.sum()) < WB
    forms = dict(rgb_form="softlp", lp_coef=0.5) if form == "softlp" else {}
    coef, far, rgb_w, depth_w = 0.2, 1.0, 1.0, 0.1
    got = {}
    seen = _spy(monkeypatch)
    for tag in ("folded", "lines"):
        coarse, fine, _, _, opt = _nets(dev, True)
        rows, _ = _rows(dev, True)
        kw = _kwargs(coarse, fine, NC, NF, 0.0, False, 0.0, False)
        if tag == "folded":
            loss = V.render_loss(WH, WW, WK, tgt, mask=mask, depth_prior=prior, chunk=4096, rows=rows, hardmask_coef=coef, depth_w=depth_w,
                                 use_viewdirs=True, ndc=True, near=0., far=far, **forms, **kw)[0]
        else:
            monkeypatch.setattr(R, "MERGE_BWD", False)
            maps = R.batchify_rays(rows, 4096, _with_depth=True, **kw)

            def level(c, d):
                il, dl = V.hardmask_losses(c, tgt, mask, coef, d, prior, far)                 # V:1645-1648, V:1737
                if form == "softlp":
                    il = V.img2mse_softLpmask(c, tgt, 0.5)                                    # V:1663-1664
                return rgb_w * il + depth_w * dl

            loss = level(maps["rgb_map"], maps["depth_map"]) + level(maps["rgb0"], maps["depth0"])
        loss.backward()
        assert [len(seen[n]) for n in PAIR_OPS] == [1, 1, 1], tag
        got[tag] = (loss.detach().clone(), rows.grad.clone(), opt.flat_grad.clone())
    lf, lr = float(got["folded"][0]), float(got["lines"][0])
    print(f"  {form}: loss folded {lf!r} lines {lr!r}")
    assert abs(lf - lr) <= (3e-7 if form == "default" else 1e-6) * abs(lr), (lf, lr)
    scale = float(got["lines"][1].abs().max())
    diff = float((got["folded"][1] - got["lines"][1]).abs().max())
    print(f"  {form}: rows.grad folded vs unpaired lines: max|d| {diff:.3e} = {diff / scale:.3e} of max|g| {scale:.3e}")
    assert scale > 0 and diff <= 1e-5 * scale
    gf, gr = got["folded"][2], got["lines"][2]
    assert float(gr.abs().max()) > 0
    if form == "default":
        assert torch.equal(gf, gr)
    else:
        assert float((gf - gr).abs().max()) <= 2e-6 * float(gr.abs().max())


def test_the_pinned_errors(dev):
    """render_loss(rays=(o, d)) with rays requiring grad still raises and names rows=; a `live` batch whose rows require grad raises;
    rows= together with rays= raises; rows of width 8 with use_viewdirs=True raise; z_vals and the target still take no gradient."""
    from consistentnerf_amd import ops, run_nerf as R, run_nerf_view as V
    coarse, fine, _, _, _ = _nets(dev, True, owned=False)
    kw = _kwargs(coarse, fine, NC, NF, 0.0, False, 0.0, False)
    rows = T(I.ray_batch(WB, seed=3), dev)
    o, d = rows[:, 0:3].clone().requires_grad_(True), rows[:, 3:6].clone()
    tgt = T(_target(), dev)
    for mod in (R, V):
        with pytest.raises(ops.CnerfError, match="render_loss") as e:
            mod.render_loss(4, 4, WK, tgt, rays=(o, d), ndc=False, near=2., far=6., use_viewdirs=True, **kw)
        assert "rows=" in str(e.value)
        with pytest.raises(ops.CnerfError, match="mutually exclusive"):
            mod.render_loss(4, 4, WK, tgt, rays=(o.detach(), d), rows=rows, use_viewdirs=True, **kw)
        with pytest.raises(ops.CnerfError, match="mutually exclusive"):
            mod.render_loss(4, 4, WK, tgt, rows=rows, c2w=torch.eye(4, device=dev)[:3], use_viewdirs=True, **kw)
        with pytest.raises(ops.CnerfError, match="use_viewdirs"):
            mod.render_loss(4, 4, WK, tgt, rows=rows[:, :8].contiguous(), use_viewdirs=True, **kw)
        with pytest.raises(ops.CnerfError, match="use_viewdirs"):
            mod.render_loss(4, 4, WK, tgt, rows=rows, use_viewdirs=False, **kw)
    live = torch.tensor([WB], device=dev, dtype=torch.int32)
    with pytest.raises(ops.CnerfError, match="live"):
        R.render_rays(rows.clone().requires_grad_(True), _live=live, **kw)
    with pytest.raises(ops.CnerfError, match="target"):
        R.render_loss(4, 4, WK, tgt.clone().requires_grad_(True), rows=rows, use_viewdirs=True, **kw)
