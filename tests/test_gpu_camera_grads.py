"""NDC and intrinsics gradients (csrc/camera_grad.hip): cnerf_camera_rows / cnerf_camera_rows_bwd / cnerf_ndc_rays_bwd, and the Python
routes pose.camera_rows (+ CameraPoses, CameraIntrinsics) -> batchify_rays -> backward, ndc_rays under autograd, and get_rays /
get_rays_at with a device K that requires grad.

Kernel level: against float64 autograd of tests/_camera_ref.py (which tests/test_camera_cpu.py holds to the reference's own get_rays
+ ndc_rays).  Error measure and bound are those of tests/test_gpu_input_grads.py: err = max|g - g64| / max|g64| per tensor, bound =
max(1e-5, 4 x err of the float32 CPU evaluation of the same restatement); both printed by every check.  The cameras are forward
facing ([Exp(w) | t], w ~ U(-0.15, 0.15)^3, t ~ U(-0.3, 0.3)^3), so that the warp's divisions by d_z stay tame: every test asserts
min |d_z| >= 0.85 on its own inputs.  The pixel cases are those of test_gpu_pose_grads.
Wiring: the row gradients of a whole batchify_rays + backward are held to float64 through the oracle's render_rays fed the NDC rows
(on the kernel's ReLU branch and fine depths, as test_gpu_input_grads does for the rays form), and the pose / intrinsics gradients
are compared, bit for bit, with the backward kernels applied to the row gradients autograd kept.
"""
import numpy as np
import pytest
import torch

import _camera_ref as CR
import _pose_ref as P
from oracle import nerf_oracle as O
from test_gpu_input_grads import KCAM, _check, _err, _loss
from test_gpu_parity import T, _kwargs, check_flips, dev, make_model, relu_masks  # noqa: F401  (dev: the device fixture)
from test_gpu_pose_grads import CASES, _case, _dev_args

pytestmark = pytest.mark.gpu

K1 = CR.K1
GUARD, NAN = 64, float("nan")
MODES = [(ndc, vd) for ndc in (True, False) for vd in (True, False)]


def _cpu_pixels(H, W, coords, view, first, B):
    cc = P.pixel_coords(H, W, first, B) if coords is None else T(coords.astype(np.int64))
    return cc, (None if view is None else T(view.astype(np.int64)))


def _setup(name, dev):
    H, W, n_views, coords, view, first, B = _case(name)
    c2w = CR.forward_poses(n_views, 5)
    cc, cv = _cpu_pixels(H, W, coords, view, first, B)
    dz = CR.min_abs_dz(H, W, K1, c2w, cc, cv)
    assert dz >= 0.85, f"{name}: min |d_z| = {dz:.3f}"
    dc, dv = _dev_args(dev, coords, view)
    return H, W, n_views, first, B, c2w, cc, cv, dc, dv


def _upstream(B, cols, seed=9):
    G = np.random.RandomState(seed).normal(size=(B, cols)).astype(np.float32)
    G[:, 6:8] = 0      # (the near / far columns carry nothing)
    return G


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", CASES)
def test_rows_forward_host_K_equals_gen_rays(dev, name):
    """cnerf_camera_rows with host intrinsics against cnerf_gen_rays of the same pose (host floats) and pixel, bit for bit, over
    {ndc} x {use_viewdirs}: near / far columns included."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.run_nerf_helpers import ndc_coefficients
    H, W, n_views, first, B, c2w, _, _, dc, dv = _setup(name, dev)
    coef = ndc_coefficients(H, W, K1[0][0])
    flat = torch.arange(first, first + B, device=dev) if dc is None else dc[:, 0] * W + dc[:, 1]
    vsel = dv if dv is not None else torch.zeros(B, dtype=torch.int64, device=dev)
    for ndc, vd in MODES:
        full = torch.stack([ops.gen_rays(H, W, K1, c2w[n], 0.25, 1.5, vd, ndc, dev, coef if ndc else (0., 0.)) for n in range(n_views)])
        rows = ops.camera_rows(H, W, K1, T(c2w.reshape(n_views, 12), dev), dc, dv, 0.25, 1.5, vd, ndc, coef if ndc else (0., 0.), first, B)
        assert rows.shape == (B, 11 if vd else 8)
        assert torch.equal(rows, full[vsel, flat]), (ndc, vd)


@pytest.mark.parametrize("name", CASES)
def test_rows_forward_device_K(dev, name):
    """K as a float32 [3,3] tensor on the GPU.  ndc=False: the same bits as with the host K.  ndc=True: the coefficients are formed
    in fp32 from K[0][0] in the kernel (the host route forms them in double), so the rows are held to the float32 restatement —
    the reference's tensor arithmetic — within 1e-6 of the largest row entry.  Measured on the MI355X: 3.0e-8 .. 1.3e-7."""
    from consistentnerf_amd import ops
    H, W, n_views, first, B, c2w, cc, cv, dc, dv = _setup(name, dev)
    d12, Kd = T(c2w.reshape(n_views, 12), dev), T(np.asarray(K1, np.float32), dev)
    for vd in (True, False):
        assert torch.equal(ops.camera_rows(H, W, Kd, d12, dc, dv, 0.25, 1.5, vd, False, (0., 0.), first, B),
                           ops.camera_rows(H, W, K1, d12, dc, dv, 0.25, 1.5, vd, False, (0., 0.), first, B))
        got = ops.camera_rows(H, W, Kd, d12, dc, dv, 0., 1., vd, True, (7., 7.), first, B)      # (ndc_coef is ignored with a device K)
        want = CR.rows(H, W, T(np.asarray(K1, np.float32)), T(c2w), cc, cv, 0., 1., vd, True)
        err = float((got.cpu() - want).abs().max() / want.abs().max())
        print(f"  rows, device K, ndc ({name}, viewdirs {vd}): max |diff| / max |row| = {err:.3e}")
        assert err <= 1e-6


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", CASES)
def test_rows_backward_against_float64(dev, name):
    """cnerf_camera_rows_bwd (device K) of a random upstream row gradient against float64 autograd of the restatement, over {ndc} x
    {use_viewdirs}: d_c2w and d_K within the bound; only the four entries of K the kernel reads are non-zero; the gradient rows of
    a view without a ray are exactly zero; the call repeated, and with 1, 2, 3 and 7 workgroups in the first launch, gives the
    same bits; leaving out d_K or d_c2w leaves the other's bits unchanged; with a host K (ndc=False) d_c2w has the same bits.
    Measured on the MI355X (profiles/camera_gpu_tests.txt): d_c2w err 3.2e-9 .. 4.7e-8, d_K err 3.5e-9 .. 4.8e-8 over the 28
    combinations, the float32 restatement 5.0e-9 .. 6.6e-7 and 3.0e-8 .. 4.5e-7; every bound is the 1e-5 floor."""
    from consistentnerf_amd import ops
    H, W, n_views, first, B, c2w, cc, cv, dc, dv = _setup(name, dev)
    d12, Kd = T(c2w.reshape(n_views, 12), dev), T(np.asarray(K1, np.float32), dev)
    for ndc, vd in MODES:
        G = _upstream(B, 11 if vd else 8)
        _, c64, k64 = CR.grads(H, W, K1, c2w, cc, cv, G, vd, ndc, torch.float64)
        _, c32, k32 = CR.grads(H, W, K1, c2w, cc, cv, G, vd, ndc, torch.float32)
        run = lambda grid=0, **kw: ops.camera_rows_bwd(T(G, dev), H, W, Kd, d12, dc, dv, vd, ndc, (0., 0.), first, grid=grid, **kw)  # noqa: E731
        d_c2w, d_K = run()
        assert d_c2w.shape == (n_views, 12) and d_K.shape == (3, 3)
        tag = f"{name}, ndc {ndc}, viewdirs {vd}"
        _check(f"d_c2w ({tag})", d_c2w, c64, c32)
        _check(f"d_K ({tag})", d_K, k64, k32)
        mask = torch.zeros(3, 3, dtype=torch.bool)
        mask[0, 0] = mask[1, 1] = mask[0, 2] = mask[1, 2] = True
        assert not d_K.cpu()[~mask].any() and not k64[~mask].any()
        if name == "views_3_one_empty":
            assert not d_c2w[1].any() and not c64[1].any() and d_c2w[0].any() and d_c2w[2].any()
        again = run()
        assert torch.equal(d_c2w, again[0]) and torch.equal(d_K, again[1])
        for grid in (1, 2, 3, 7):
            a, b = run(grid)
            assert torch.equal(d_c2w, a) and torch.equal(d_K, b), f"grid {grid} changed the bits"
        only_c, none_k = run(want_K=False)
        none_c, only_k = run(want_c2w=False)
        assert none_k is None and none_c is None and torch.equal(only_c, d_c2w) and torch.equal(only_k, d_K)
        if not ndc:
            host = ops.camera_rows_bwd(T(G, dev), H, W, K1, d12, dc, dv, vd, False, (0., 0.), first)
            assert torch.equal(host[0], d_c2w) and torch.equal(host[1], d_K)


@pytest.mark.parametrize("name", ["image_19x29", "views_3_one_empty"])
def test_rows_backward_needs_the_coefficient_paths(dev, name):
    """With ndc K[0][0] also reaches the rows through the two coefficients of H:193-199.  Against a float64 side that drops those
    paths (the graph from K[0][0] to the coefficients cut, every value the same) the check of d_K[0][0] must FAIL — while d_c2w,
    which does not see them, still passes: the float64 test above can see that term.  Measured on the MI355X: err 0.56 (551 rays)
    and 0.20 (300 rays over three views) against the bound 1e-5."""
    from consistentnerf_amd import ops
    H, W, n_views, first, B, c2w, cc, cv, dc, dv = _setup(name, dev)
    G = _upstream(B, 11)
    _, c64, k64 = CR.grads(H, W, K1, c2w, cc, cv, G, True, True, torch.float64)
    _, c32, k32 = CR.grads(H, W, K1, c2w, cc, cv, G, True, True, torch.float32)
    _, ccut, kcut = CR.grads(H, W, K1, c2w, cc, cv, G, True, True, torch.float64, coef_paths=False)
    d_c2w, d_K = ops.camera_rows_bwd(T(G, dev), H, W, T(np.asarray(K1, np.float32), dev), T(c2w.reshape(n_views, 12), dev), dc, dv, True, True,
                                     (0., 0.), first)
    _check("d_c2w (coefficient paths dropped on the float64 side)", d_c2w, ccut, c32)
    bound = max(1e-5, 4.0 * _err(k32, k64))
    err = abs(float(d_K[0, 0]) - float(kcut[0, 0])) / float(kcut.abs().max())
    print(f"  d_K[0][0] against float64 without the coefficient paths: err {err:.3e} (bound {bound:.3e})")
    assert err > 10 * bound


@pytest.mark.parametrize("name", ["one_ray", "image_19x29", "views_3_one_empty"])
def test_guarded_buffers(dev, name):
    """The C entry points on outputs of exactly their size inside NaN guard bands (64 floats each side): the guards stay NaN, every
    element between them is written (the rows, d_c2w, d_K, the workspace, d_rays_o / d_rays_d), and the results equal the ops
    wrappers'."""
    from consistentnerf_amd import _lib, ops
    from consistentnerf_amd.ops import _p, _stream
    H, W, n_views, first, B, c2w, _, _, dc, dv = _setup(name, dev)
    d12, Kd = T(c2w.reshape(n_views, 12), dev), T(np.asarray(K1, np.float32), dev)
    lib = _lib.load()
    nws = lib.cnerf_camera_rows_bwd_ws_floats(B, n_views)
    assert nws == 2 * (12 * n_views + 4) * ((B + 63) // 64)

    def guarded(n):
        buf = torch.full((GUARD + n + GUARD,), NAN, device=dev)
        return buf, buf[GUARD:GUARD + n]

    def intact(buf, n, what):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{what}: a write outside the buffer"

    G = T(_upstream(B, 11), dev)
    rows_b, rows = guarded(B * 11)
    _lib.check(lib.cnerf_camera_rows(H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, _p(Kd), _p(d12), n_views, _p(dc), _p(dv), first, B, 0.0, 1.0, 1, 1,
                                     _p(rows), _stream()), "cnerf_camera_rows")
    intact(rows_b, B * 11, "rows")
    assert not torch.isnan(rows).any()
    assert torch.equal(rows.view(B, 11), ops.camera_rows(H, W, Kd, d12, dc, dv, 0., 1., True, True, (0., 0.), first, B))
    (ws_b, ws), (c_b, d_c2w), (k_b, d_K) = guarded(nws), guarded(n_views * 12), guarded(9)
    _lib.check(lib.cnerf_camera_rows_bwd(H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, _p(Kd), _p(d12), n_views, _p(dc), _p(dv), first, B, 1, 1, _p(G),
                                         _p(d_c2w), _p(d_K), _p(ws), 0, _stream()), "cnerf_camera_rows_bwd")
    intact(ws_b, nws, "workspace"), intact(c_b, n_views * 12, "d_c2w"), intact(k_b, 9, "d_K")
    assert not torch.isnan(ws.view(torch.float64)).any(), "a record that was not written"
    assert not torch.isnan(d_c2w).any() and not torch.isnan(d_K).any()
    want = ops.camera_rows_bwd(G, H, W, Kd, d12, dc, dv, True, True, (0., 0.), first)
    assert torch.equal(d_c2w.view(n_views, 12), want[0]) and torch.equal(d_K.view(3, 3), want[1])
    # cnerf_ndc_rays_bwd on the pre-NDC rays of the same pixels
    o, d = ops.gen_rays_at(H, W, K1, d12, dc, dv, first, B)
    (o_b, d_o), (d_b, d_d) = guarded(B * 3), guarded(B * 3)
    g_o, g_d = G[:, 0:3].contiguous(), G[:, 3:6].contiguous()
    _lib.check(lib.cnerf_ndc_rays_bwd(_p(g_o), _p(g_d), _p(o), _p(d), B, -1.5, -1.25, _p(d_o), _p(d_d), _stream()), "cnerf_ndc_rays_bwd")
    intact(o_b, B * 3, "d_rays_o"), intact(d_b, B * 3, "d_rays_d")
    want = ops.ndc_rays_bwd(g_o, g_d, o, d, (-1.5, -1.25))
    assert torch.equal(d_o.view(B, 3), want[0]) and torch.equal(d_d.view(B, 3), want[1])


# ------------------------------------------------------------------------------------------------ ndc_rays under autograd
def _ndc_inputs(dev):
    from consistentnerf_amd import ops
    H, W = CR.H1, CR.W1
    c2w = CR.forward_poses(1, 17)
    o, d = ops.gen_rays_at(H, W, K1, T(c2w.reshape(1, 12), dev), None, None, 0, H * W)
    assert float(d[:, 2].abs().min()) >= 0.85
    rs = np.random.RandomState(12)
    return H, W, o.reshape(H, W, 3), d.reshape(H, W, 3), rs.normal(size=(H, W, 3)).astype(np.float32), rs.normal(size=(H, W, 3)).astype(np.float32)


def test_ndc_rays_keeps_the_graph(dev):
    """run_nerf_helpers.ndc_rays on [H, W, 3] rays requiring grad: the outputs carry a graph and equal the no-grad call bit for bit;
    d_rays_o / d_rays_d of a random linear functional against float64 autograd of the restatement; only one of the two requiring
    grad works as well.  run_nerf / run_nerf_view export the same function.  Measured on the MI355X: err 6.0e-8 / 9.0e-8 (float32
    restatement 1.5e-7 / 1.9e-7)."""
    from consistentnerf_amd import run_nerf as R, run_nerf_view as V
    from consistentnerf_amd.run_nerf_helpers import ndc_rays
    assert R.ndc_rays is ndc_rays and V.ndc_rays is ndc_rays
    H, W, o, d, G_o, G_d = _ndc_inputs(dev)
    focal = K1[0][0]
    o0, d0 = ndc_rays(H, W, focal, 1., o, d)
    assert not o0.requires_grad and not d0.requires_grad
    to, td = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    on, dn = ndc_rays(H, W, focal, 1., to, td)
    assert on.shape == (H, W, 3) and dn.shape == (H, W, 3) and on.requires_grad and dn.requires_grad
    assert torch.equal(on, o0) and torch.equal(dn, d0)
    with torch.no_grad():
        assert not ndc_rays(H, W, focal, 1., to, td)[0].requires_grad
    ((on * T(G_o, dev)).sum() + (dn * T(G_d, dev)).sum()).backward()

    def ref(dtype):
        ro, rd = o.cpu().to(dtype).reshape(-1, 3).requires_grad_(True), d.cpu().to(dtype).reshape(-1, 3).requires_grad_(True)
        a, b = CR.ndc_warp(ro, rd, *CR.ndc_coefs(H, W, focal))
        ((a * T(G_o).to(dtype).reshape(-1, 3)).sum() + (b * T(G_d).to(dtype).reshape(-1, 3)).sum()).backward()
        return ro.grad.double(), rd.grad.double()
    (o64, d64), (o32, d32) = ref(torch.float64), ref(torch.float32)
    assert to.grad.shape == (H, W, 3) and td.grad.shape == (H, W, 3)
    _check("d_rays_o (ndc_rays)", to.grad.reshape(-1, 3), o64, o32)
    _check("d_rays_d (ndc_rays)", td.grad.reshape(-1, 3), d64, d32)
    td2 = d.clone().requires_grad_(True)
    on2, dn2 = ndc_rays(H, W, focal, 1., o, td2)
    ((on2 * T(G_o, dev)).sum() + (dn2 * T(G_d, dev)).sum()).backward()
    assert torch.equal(td2.grad, td.grad)


def test_ndc_rays_without_grad_runs_what_it_ran(dev, monkeypatch):
    """Rays that do not require grad: one ops.pack_rays call with the arguments of before and none of the new ops functions; a
    focal tensor requiring grad raises CnerfError naming camera_rows (it used to lose its graph silently)."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.run_nerf_helpers import ndc_coefficients, ndc_rays
    H, W, o, d, _, _ = _ndc_inputs(dev)
    calls, pack = [], ops.pack_rays
    monkeypatch.setattr(ops, "pack_rays", lambda *a, **k: calls.append(("pack_rays", a, k)) or pack(*a, **k))
    for name in ("ndc_rays_bwd", "camera_rows", "camera_rows_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    on, dn = ndc_rays(H, W, K1[0][0], 1., o, d)
    assert len(calls) == 1 and calls[0][0] == "pack_rays" and not calls[0][2]
    a = calls[0][1]
    assert a[0] is o and a[1] is d and a[2:] == (0., 1., False, True, ndc_coefficients(H, W, K1[0][0]))
    want = pack(o, d, 0., 1., False, True, ndc_coefficients(H, W, K1[0][0]))
    assert torch.equal(on.reshape(-1, 3), want[:, 0:3]) and torch.equal(dn.reshape(-1, 3), want[:, 3:6])
    focal = torch.tensor(K1[0][0], device=dev, requires_grad=True)
    with pytest.raises(ops.CnerfError, match="camera_rows"):
        ndc_rays(H, W, focal, 1., o, d)
    with torch.no_grad():      # (nothing to lose without grad mode)
        assert ndc_rays(H, W, focal, 1., o, d)[0].shape == on.shape


# ------------------------------------------------------------------------------------------------ get_rays with a learnable K
@pytest.mark.parametrize("pose_grad", [True, False])
def test_get_rays_keeps_the_graph_of_K(dev, pose_grad):
    """get_rays(H, W, K, pose) on a 6 x 8 image with K a float32 [3,3] tensor on the GPU requiring grad (the pose a device tensor
    requiring grad, or a host array): the rays carry a graph and equal the host-K call bit for bit; K.grad (and pose.grad) of
    (rays_o * Go + rays_d * Gd).sum() pass the float64 check.  get_rays_at likewise, on a few pixels."""
    from consistentnerf_amd.run_nerf_helpers import get_rays, get_rays_at
    H, W = 6, 8
    c2w = CR.forward_poses(1, 31)[0]
    G = _upstream(H * W, 8, seed=4)
    K = T(np.asarray(K1, np.float32), dev).requires_grad_(True)
    pose = T(c2w, dev).requires_grad_(True) if pose_grad else c2w
    o, d = get_rays(H, W, K, pose)
    assert o.shape == (H, W, 3) and d.shape == (H, W, 3) and o.requires_grad and d.requires_grad
    o0, d0 = get_rays(H, W, K1, c2w)
    assert not d0.requires_grad and torch.equal(o, o0) and torch.equal(d, d0)
    ((o.reshape(-1, 3) * T(G[:, 0:3], dev)).sum() + (d.reshape(-1, 3) * T(G[:, 3:6], dev)).sum()).backward()
    cc = P.pixel_coords(H, W)
    _, c64, k64 = CR.grads(H, W, K1, c2w, cc, None, G, False, False, torch.float64)
    _, c32, k32 = CR.grads(H, W, K1, c2w, cc, None, G, False, False, torch.float32)
    assert K.grad is not None and K.grad.shape == (3, 3)
    _check("K.grad (get_rays)", K.grad, k64, k32)
    if pose_grad:
        _check("pose.grad (get_rays)", pose.grad.reshape(1, 12), c64, c32)
    # get_rays_at: chosen pixels index the same rays, and K.grad is that of the subset
    sel = torch.tensor([[5, 7], [0, 0], [2, 3], [5, 7], [1, 5]])
    K2 = T(np.asarray(K1, np.float32), dev).requires_grad_(True)
    oa, da = get_rays_at(H, W, K2, T(c2w, dev), sel.to(dev))
    flat = (sel[:, 0] * W + sel[:, 1]).to(dev)
    assert torch.equal(oa, o0.reshape(-1, 3)[flat]) and torch.equal(da, d0.reshape(-1, 3)[flat])
    ((oa * T(G[:5, 0:3], dev)).sum() + (da * T(G[:5, 3:6], dev)).sum()).backward()
    _, _, s64 = CR.grads(H, W, K1, c2w, sel, None, G[:5], False, False, torch.float64)
    _, _, s32 = CR.grads(H, W, K1, c2w, sel, None, G[:5], False, False, torch.float32)
    _check("K.grad (get_rays_at)", K2.grad, s64, s32)


def test_get_rays_without_K_grad_takes_none_of_the_new_paths(dev, monkeypatch):
    """A host K, or a device K tensor that does not require grad: none of the new ops functions is called by get_rays / get_rays_at
    (with or without a pose requiring grad)."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.run_nerf_helpers import get_rays, get_rays_at
    calls = []
    for name in ("camera_rows", "camera_rows_bwd", "ndc_rays_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    c2w = CR.forward_poses(1, 31)[0]
    want = ops.gen_rays(6, 8, K1, c2w, 0.0, 1.0, False, False, dev)
    pose = T(c2w, dev).requires_grad_(True)
    o, d = get_rays(6, 8, K1, pose)
    (o.sum() + d.sum()).backward()
    assert torch.equal(o.reshape(-1, 3), want[:, 0:3]) and torch.equal(d.reshape(-1, 3), want[:, 3:6]) and pose.grad is not None
    o, d = get_rays(6, 8, K1, c2w)
    assert torch.equal(d.reshape(-1, 3), want[:, 3:6])
    oa, da = get_rays_at(6, 8, K1, pose, torch.tensor([[1, 2]], device=dev))
    assert torch.equal(da[0], want[1 * 8 + 2, 3:6])
    with torch.no_grad():
        get_rays(6, 8, K1, pose)
    assert not calls, calls


# ------------------------------------------------------------------------------------------------ the whole chain
WH, WW, WB, WNC, WNF = 9, 11, 37, 16, 16
WK = [[24.0, 0.0, 5.25], [0.0, 22.0, 4.75], [0.0, 0.0, 1.0]]


def _chain_camera(dev):
    """Three forward-facing cameras moved off their initial poses (rot ~ 0.03 rad, trans ~ 0.05), intrinsics moved off K0 (focal
    lengths by a few per cent, untied; the centre by a fraction of a pixel), 37 pixels over the three views."""
    from consistentnerf_amd.pose import CameraIntrinsics, CameraPoses
    rs = np.random.RandomState(23)
    poses = CameraPoses(T(CR.forward_poses(3, 29), dev))
    intr = CameraIntrinsics(T(np.asarray(WK, np.float32), dev), learn_focal=True, learn_center=True, tie_focal=False)
    with torch.no_grad():
        poses.rot.copy_(T((0.03 * rs.normal(size=(3, 3))).astype(np.float32), dev))
        poses.trans.copy_(T((0.05 * rs.normal(size=(3, 3))).astype(np.float32), dev))
        intr.log_focal.copy_(T((0.03 * rs.normal(size=2)).astype(np.float32), dev))
        intr.center.copy_(T((0.3 * rs.normal(size=2)).astype(np.float32), dev))
    coords = T(np.stack([rs.randint(0, WH, size=WB), rs.randint(0, WW, size=WB)], -1).astype(np.int64), dev)
    view = T(rs.randint(0, 3, size=WB).astype(np.int64), dev)
    return poses, intr, coords, view


def _chain_G():
    rs = np.random.RandomState(7)
    return {k: rs.normal(size=(WB, 3) if k.startswith("rgb") else (WB,)).astype(np.float32)
            for k in ("rgb_map", "depth_map", "acc_map", "rgb0", "depth0")}


_CHAIN_REF = {}


def _chain_reference(dev, vd, rows):
    """(float64, float32) oracle gradients w.r.t. the rows, on the kernel's ReLU masks and fine depths; once per vd."""
    if vd in _CHAIN_REF:
        return _CHAIN_REF[vd]
    from consistentnerf_amd import run_nerf_view as V
    D, Wn = 4, 128
    (coarse, sdc), (fine, sdf) = make_model(D, Wn, vd, 5, 31, dev), make_model(D, Wn, vd, 5, 32, dev)
    ret = V.render_rays(rows.detach().clone(), retraw=True, _debug=True, **_kwargs(coarse, fine, WNC, WNF, 0.0, False, 0.0, False))
    masks_c = relu_masks(ret["_raw_coarse"].grad_fn.stash, WB * WNC, D, Wn, vd)
    masks_f = relu_masks(ret["raw"].grad_fn.stash, WB * (WNC + WNF), D, Wn, vd)
    z_fine = ret["_z_vals"].detach().cpu()
    rows_cpu, G = rows.detach().cpu(), _chain_G()

    def run(dtype, flips):
        r = rows_cpu.to(dtype).clone().requires_grad_(True)
        out = O.render_rays(r, {k: T(v).to(dtype) for k, v in sdc.items()}, {k: T(v).to(dtype) for k, v in sdf.items()},
                            O.NetCfg(D, Wn, use_viewdirs=vd, output_ch=5), O.RenderCfg(WNC, WNF, 0.0, False, False, 0.0),
                            u=torch.linspace(0.0, 1.0, WNF, dtype=dtype).expand(WB, WNF), z_fine=z_fine.to(dtype),
                            masks_coarse=masks_c, masks_fine=masks_f, flips=flips)
        _loss(out, G, lambda g: T(g).to(dtype)).backward()
        return r.grad.double()

    flips32, flips64 = [], []
    g64, g32 = run(torch.float64, flips64), run(torch.float32, flips32)
    # (the tolerances of test_gpu_input_grads._rays_reference: the float32 oracle sees the kernel's positions, the float64 one the
    # unrounded o + d z, which layer 0 of the 2^9-frequency encoding amplifies)
    check_flips(flips32)
    xmax = float((rows_cpu[:, None, 0:3] + rows_cpu[:, None, 3:6] * z_fine[:, :, None]).abs().max())
    dx = 1.5 * 2.0 ** (np.floor(np.log2(xmax)) - 23)
    check_flips(flips64, tol=1e-5 + float(np.abs(sdc["pts_linears.0.weight"]).max()) * (6 * 1023 + 3) * dx)
    _CHAIN_REF[vd] = (g64, g32)
    return _CHAIN_REF[vd]


@pytest.mark.parametrize("chunk", [16, 4096])
@pytest.mark.parametrize("vd", [True, False])
def test_camera_gradients_through_batchify_rays(dev, vd, chunk):
    """CameraPoses (N = 3) + CameraIntrinsics -> pose.camera_rows(ndc=True, near=0, far=1) of 37 pixels over the three views ->
    batchify_rays (chunk 16: three slices) of two D4 / W128 networks, 16 + 16 samples, the mixed loss of the rays-form tests ->
    backward.  rows.grad (origins, directions, view directions) passes the float64 check against the oracle's render_rays fed the
    same NDC rows; poses.rot.grad / poses.trans.grad, K.grad and the intrinsics' parameter gradients equal, bit for bit, the
    backward kernels (and autograd of the nine-float composition) applied to the rows.grad autograd kept.
    Measured on the MI355X: rows.grad err 1.2e-5 / 8.3e-6 / 8.5e-7 (origins / directions / view directions; bounds 4.9e-5 / 3.4e-5 /
    1e-5) with view directions, 2.6e-5 / 1.2e-5 (bounds 1.0e-4 / 4.8e-5) without, the float32 oracle within 7 % of the same figures:
    both evaluate the encoding at positions rounded to fp32 (test_rays_form_against_float64)."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.pose import camera_rows
    (coarse, _), (fine, _) = make_model(4, 128, vd, 5, 31, dev), make_model(4, 128, vd, 5, 32, dev)
    poses, intr, coords, view = _chain_camera(dev)
    c2w, K = poses(), intr()
    assert CR.min_abs_dz(WH, WW, K.detach().cpu().tolist(), c2w.detach().cpu().numpy(), coords.cpu(), view.cpu()) >= 0.85
    assert K.shape == (3, 3) and K.requires_grad and c2w.requires_grad
    K.retain_grad()
    rows = camera_rows(WH, WW, K, c2w, coords, view, near=0., far=1., use_viewdirs=vd, ndc=True)
    assert rows.shape == (WB, 11 if vd else 8) and rows.requires_grad
    rows.retain_grad()
    out = R.batchify_rays(rows, chunk, _with_depth=True, **_kwargs(coarse, fine, WNC, WNF, 0.0, False, 0.0, False))
    _loss(out, _chain_G(), lambda g: T(g, dev)).backward()
    g = rows.grad
    assert g is not None and torch.isfinite(g).all() and g[:, 0:6].abs().max() > 0
    g64, g32 = _chain_reference(dev, vd, rows)
    _check("rows.grad, origins", g[:, 0:3], g64[:, 0:3], g32[:, 0:3])
    _check("rows.grad, directions", g[:, 3:6], g64[:, 3:6], g32[:, 3:6])
    if vd:
        _check("rows.grad, view directions", g[:, 8:11], g64[:, 8:11], g32[:, 8:11])
    d_c2w, d_K = ops.camera_rows_bwd(g, WH, WW, K.detach(), c2w.detach().reshape(3, 12), coords, view, vd, True)
    want_rot, want_trans = ops.pose_compose_bwd(poses.c2w0, poses.rot.detach(), d_c2w)
    for name, got, want in (("rot", poses.rot.grad, want_rot), ("trans", poses.trans.grad, want_trans), ("K", K.grad, d_K)):
        assert got is not None and torch.isfinite(got).all() and got.any(), name
        assert torch.equal(got, want), name
    want_f, want_c = torch.autograd.grad(intr(), [intr.log_focal, intr.center], d_K)
    assert intr.log_focal.grad.shape == (2,) and torch.equal(intr.log_focal.grad, want_f) and intr.log_focal.grad.abs().min() > 0
    assert torch.equal(intr.center.grad, want_c) and intr.center.grad.abs().min() > 0
    assert coarse.kernel_tensors()[0].grad is not None      # (the networks learn in the same backward)


def test_camera_rows_surface(dev):
    """pose.camera_rows: the rows of render(c2w=...)'s batch (ops.gen_rays) bit for bit with a host K; a [4,4] pose (zeros for
    its bottom row), a single [3,4] pose with a first / B window, no graph without grad; tensor near / far and a host pose raise."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.pose import camera_rows
    from consistentnerf_amd.run_nerf_helpers import ndc_coefficients
    H, W = 6, 8
    c2w = CR.forward_poses(1, 31)[0]
    want = ops.gen_rays(H, W, K1, c2w, 0., 1., True, True, dev, ndc_coefficients(H, W, K1[0][0]))
    pose = T(np.concatenate([c2w, [[0, 0, 0, 1]]], 0).astype(np.float32), dev).requires_grad_(True)
    rows = camera_rows(H, W, K1, pose, use_viewdirs=True)
    assert rows.requires_grad and torch.equal(rows, want)
    rows.sum().backward()
    assert pose.grad.shape == (4, 4) and not pose.grad[3].any() and pose.grad[:3].any()
    win = camera_rows(H, W, K1, pose.detach()[:3], first=11, B=20, use_viewdirs=True)
    assert not win.requires_grad and torch.equal(win, want[11:31])
    with torch.no_grad():
        assert not camera_rows(H, W, K1, pose, use_viewdirs=True).requires_grad
    with pytest.raises(ops.CnerfError, match="near / far"):
        camera_rows(H, W, K1, pose, near=torch.zeros(H * W, device=dev))
    with pytest.raises(ops.CnerfError, match="GPU"):
        camera_rows(H, W, K1, c2w)
    with pytest.raises(ops.CnerfError, match=r"\[3, 3\]"):
        camera_rows(H, W, torch.eye(4, device=dev), pose)


# ------------------------------------------------------------------------------------------------ what keeps raising
def test_the_pinned_errors_name_the_new_route(dev):
    """render(rays=<grad>, ndc=True), render(c2w=<grad>) and render(c2w_staticcam=<grad>) still raise CnerfError, with the strings
    the earlier tests match on, and now name camera_rows + batchify_rays."""
    from consistentnerf_amd import ops, run_nerf as R, run_nerf_view as V
    coarse, _ = make_model(2, 64, True, 5, 21, dev)
    kw = _kwargs(coarse, None, 8, 0, 0.0, False, 0.0, False)
    o = torch.zeros(5, 3, device=dev).requires_grad_(True)
    d = torch.tensor([0.1, 0.2, -1.0], device=dev).expand(5, 3)
    pose = torch.eye(4, device=dev)[:3].requires_grad_(True)
    still = torch.eye(4, device=dev)[:3]
    for mod in (R, V):
        with pytest.raises(ops.CnerfError, match="ndc=True") as e:
            mod.render(4, 4, KCAM, rays=(o, d), ndc=True, near=0., far=1., use_viewdirs=True, **kw)
        assert "camera_rows" in str(e.value) and "batchify_rays" in str(e.value)
        with pytest.raises(ops.CnerfError, match="c2w.*get_rays") as e:
            mod.render(4, 4, KCAM, c2w=pose, ndc=False, near=2., far=6., use_viewdirs=True, **kw)
        assert "camera_rows" in str(e.value) and "batchify_rays" in str(e.value)
        with pytest.raises(ops.CnerfError, match="c2w_staticcam") as e:
            mod.render(4, 4, KCAM, c2w=still, c2w_staticcam=pose, ndc=False, near=2., far=6., use_viewdirs=True, **kw)
        assert "camera_rows" in str(e.value) and "batchify_rays" in str(e.value)
