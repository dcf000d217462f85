"""Camera pose gradients (csrc/rays_grad.hip): cnerf_gen_rays_at / cnerf_gen_rays_at_bwd, cnerf_pose_compose / _bwd, and the Python
route get_rays / get_rays_at / CameraPoses -> render(rays=..., ndc=False) -> backward.

Kernel level: against float64 autograd of tests/_pose_ref.py (which tests/test_pose_cpu.py holds to the reference's own get_rays).
Error measure and bound are those of tests/test_gpu_input_grads.py: err = max|g - g64| / max|g64| per tensor, bound = max(1e-5, 4 x
err of the float32 CPU evaluation of the same restatement); both printed by every check.
Wiring: the rays' gradients are held to float64 by test_gpu_input_grads.py, so the pose gradients of a whole render + backward are
compared, bit for bit, with the two backward kernels applied to the rays' gradients autograd kept.
"""
import numpy as np
import pytest
import torch

import _pose_ref as P
from test_gpu_input_grads import FAR, KCAM, NEAR, _check, _loss
from test_gpu_parity import T, _kwargs, dev, make_model  # noqa: F401  (dev: the device fixture)

pytestmark = pytest.mark.gpu

K1 = [[23.5, 0.0, 13.25], [0.0, 21.75, 8.5], [0.0, 0.0, 1.0]]      # non-centred principal point, fx != fy
GUARD, NAN = 64, float("nan")


def _poses(n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([np.concatenate([np.linalg.qr(rs.normal(size=(3, 3)))[0], rs.uniform(-2, 2, size=(3, 1))], 1)
                     for _ in range(n)]).astype(np.float32)


def _case(name):
    """name -> (H, W, n_views, coords [B, 2] | None, view [B] | None, first, B)"""
    rs = np.random.RandomState(41)
    if name == "one_ray":
        return 5, 7, 1, np.array([[2, 3]]), None, 0, 1
    if name == "image_5x7":               # 35 rays: less than one wave
        return 5, 7, 1, None, None, 0, 35
    if name == "image_19x29":             # 551 rays: 9 chunks of 64 over 3 workgroups, a ragged last one
        return 19, 29, 1, None, None, 0, 551
    if name == "coords_300":              # duplicates, unsorted
        c = np.stack([rs.randint(0, 19, size=300), rs.randint(0, 29, size=300)], -1)
        c[7], c[250] = c[100], c[100]
        return 19, 29, 1, c, None, 0, 300
    if name == "window_mid_row":          # first / B window that starts and ends inside a row
        return 19, 29, 1, None, None, 3 * 29 + 11, 200
    if name == "views_3_one_empty":       # a random view per ray; view 1 gets none
        c = np.stack([rs.randint(0, 19, size=300), rs.randint(0, 29, size=300)], -1)
        return 19, 29, 3, c, rs.choice([0, 2], size=300), 0, 300
    if name == "views_window":            # view without coords
        return 19, 29, 3, None, rs.randint(0, 3, size=130), 40, 130
    raise KeyError(name)


CASES = ["one_ray", "image_5x7", "image_19x29", "coords_300", "window_mid_row", "views_3_one_empty", "views_window"]


def _dev_args(dev, coords, view):
    return (None if coords is None else T(coords.astype(np.int64), dev)), (None if view is None else T(view.astype(np.int64), dev))


def _upstream(B, seed=9):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(B, 3)).astype(np.float32), rs.normal(size=(B, 3)).astype(np.float32)


def _ref_grad(H, W, n_views, coords, view, first, B, c2w, G_o, G_d, dtype):
    pose = T(c2w).to(dtype).requires_grad_(True)
    cc = P.pixel_coords(H, W, first, B) if coords is None else T(coords.astype(np.int64))
    o, d = P.get_rays_at(H, W, K1, pose, cc, None if view is None else T(view.astype(np.int64)))
    ((o * T(G_o).to(dtype)).sum() + (d * T(G_d).to(dtype)).sum()).backward()
    return pose.grad.double().reshape(n_views, 12)


# ------------------------------------------------------------------------------------------------ the rays kernels, forward
@pytest.mark.parametrize("name", CASES)
def test_rays_forward_equals_gen_rays(dev, name):
    """cnerf_gen_rays_at against cnerf_gen_rays of the same pose (host floats) and pixel, bit for bit: the full image, a coords list
    (= indexing the full image), a row-major window, and a view per ray."""
    from consistentnerf_amd import ops
    H, W, n_views, coords, view, first, B = _case(name)
    c2w = _poses(n_views, 5)
    full = torch.stack([ops.gen_rays(H, W, K1, c2w[n], 0.0, 1.0, False, False, dev)[:, 0:6] for n in range(n_views)])   # [n, HW, 6]
    dc, dv = _dev_args(dev, coords, view)
    o, d = ops.gen_rays_at(H, W, K1, T(c2w.reshape(n_views, 12), dev), dc, dv, first, B)
    assert o.shape == (B, 3) and d.shape == (B, 3)
    flat = torch.arange(first, first + B, device=dev) if coords is None else dc[:, 0] * W + dc[:, 1]
    want = full[dv if view is not None else torch.zeros(B, dtype=torch.int64, device=dev), flat]
    assert torch.equal(o, want[:, 0:3]) and torch.equal(d, want[:, 3:6])


# ------------------------------------------------------------------------------------------------ the rays kernels, backward
@pytest.mark.parametrize("name", CASES)
def test_rays_backward_against_float64(dev, name):
    """cnerf_gen_rays_at_bwd of a random upstream gradient against float64 autograd of the restatement; the gradient rows of a view
    without a ray are exactly zero; the call repeated, and with 1, 2, 3 and 7 workgroups in the first launch, gives the same bits.
    Measured on the MI355X (profiles/pose_gpu_tests.txt): err 5.0e-9 (one ray) .. 3.0e-8 over the seven cases, the float32 restatement
    (fp32 sums) 5.0e-9 .. 5.7e-7; every bound is the 1e-5 floor."""
    from consistentnerf_amd import ops
    H, W, n_views, coords, view, first, B = _case(name)
    c2w, (G_o, G_d) = _poses(n_views, 5), _upstream(B)
    g64 = _ref_grad(H, W, n_views, coords, view, first, B, c2w, G_o, G_d, torch.float64)
    g32 = _ref_grad(H, W, n_views, coords, view, first, B, c2w, G_o, G_d, torch.float32)
    dc, dv = _dev_args(dev, coords, view)
    run = lambda grid=0: ops.gen_rays_at_bwd(T(G_o, dev), T(G_d, dev), H, W, K1, n_views, dc, dv, first, grid)  # noqa: E731
    got = run()
    assert got.shape == (n_views, 12)
    _check(f"d_c2w ({name})", got, g64, g32)
    if name == "views_3_one_empty":
        assert not got[1].any() and not g64[1].any() and got[0].any() and got[2].any()
    assert torch.equal(got, run())
    for grid in (1, 2, 3, 7):
        assert torch.equal(got, run(grid)), f"grid {grid} changed the bits"


@pytest.mark.parametrize("name", ["one_ray", "image_19x29", "views_3_one_empty"])
def test_rays_backward_guarded_buffers(dev, name):
    """The C entry point on d_c2w and a workspace of exactly the queried size, each followed by a NaN guard band: the guards stay NaN,
    every element of both is written, and the result equals the ops wrapper's."""
    from consistentnerf_amd import _lib, ops
    from consistentnerf_amd.ops import _p, _stream
    H, W, n_views, coords, view, first, B = _case(name)
    G_o, G_d = (T(g, dev) for g in _upstream(B))
    dc, dv = _dev_args(dev, coords, view)
    lib = _lib.load()
    nws = lib.cnerf_gen_rays_at_bwd_ws_floats(B, n_views)
    assert nws == 2 * 12 * n_views * ((B + 63) // 64)
    ws = torch.full((nws + GUARD,), NAN, device=dev)
    out = torch.full((n_views * 12 + GUARD,), NAN, device=dev)
    fx, fy, cx, cy = K1[0][0], K1[1][1], K1[0][2], K1[1][2]
    _lib.check(lib.cnerf_gen_rays_at_bwd(H, W, fx, fy, cx, cy, _p(G_o), _p(G_d), n_views, _p(dc), _p(dv), first, B, _p(out), _p(ws), 0,
                                         _stream()), "cnerf_gen_rays_at_bwd")
    assert torch.isnan(ws[nws:]).all() and torch.isnan(out[n_views * 12:]).all(), "a write past the end"
    assert not torch.isnan(ws[:nws].view(torch.float64)).any(), "a record that was not written"
    assert not torch.isnan(out[:n_views * 12]).any()
    assert torch.equal(out[:n_views * 12].view(n_views, 12), ops.gen_rays_at_bwd(G_o, G_d, H, W, K1, n_views, dc, dv, first))
    # the forward likewise
    o, d = torch.full((B * 3 + GUARD,), NAN, device=dev), torch.full((B * 3 + GUARD,), NAN, device=dev)
    c2w = T(_poses(n_views, 5).reshape(n_views, 12), dev)
    _lib.check(lib.cnerf_gen_rays_at(H, W, fx, fy, cx, cy, _p(c2w), n_views, _p(dc), _p(dv), first, B, _p(o), _p(d), _stream()),
               "cnerf_gen_rays_at")
    for buf in (o, d):
        assert torch.isnan(buf[B * 3:]).all() and not torch.isnan(buf[:B * 3]).any()


# ------------------------------------------------------------------------------------------------ the pose composition
ANGLES = [0.0, 1e-6, 1e-4, 1e-2, 1.0, 3.0]
ULP1 = 2.0 ** -23


def _compose_inputs(N, mag):
    rs = np.random.RandomState(int(1000 * N + 7))
    ax = rs.normal(size=(N, 3))
    rot = (ax / np.linalg.norm(ax, axis=-1, keepdims=True) * mag).astype(np.float32)
    return _poses(N, 13), rot, rs.uniform(-1, 1, size=(N, 3)).astype(np.float32), rs.normal(size=(N, 3, 4)).astype(np.float32)


def _compose_ref(c2w0, rot, trans, G, dtype):
    r, t = T(rot).to(dtype).requires_grad_(True), T(trans).to(dtype).requires_grad_(True)
    c2w = P.pose_compose(T(c2w0).to(dtype), r, t)
    (c2w * T(G).to(dtype)).sum().backward()
    return c2w.detach().double(), r.grad.double(), t.grad.double()


@pytest.mark.parametrize("mag", ANGLES)
@pytest.mark.parametrize("N", [1, 3])
def test_pose_compose_against_float64(dev, N, mag):
    """cnerf_pose_compose and cnerf_pose_compose_bwd at |rot| = 0 exactly, 1e-6, 1e-4, 1e-2, 1 (the series / closed-form threshold)
    and 3 on random axes: value, d_rot and d_trans against float64; at rot = 0 the value is c2w0 bit for bit and d_rot the three
    generators applied to R0; R^T R - I of the value within 8 ulps of 1 (9.5e-7): each element of R = E R0 is three products and
    two sums of numbers below 1 in magnitude (at most 2.5 ulps), on an E that Rodrigues' formula gives to a few ulps and an R0 rounded to
    fp32 (half an ulp per element), and an element of R^T R sums three such products.
    Measured on the MI355X (profiles/pose_gpu_tests.txt): rotation err 0 (rot = 0) .. 2.3e-7 (|rot| = 3), d_rot err 3.7e-8 .. 2.1e-7
    (float32 restatement 3.3e-8 .. 5.7e-7), d_trans exact; max|R^T R - I| 4.0e-8 .. 1.2e-7 up to |rot| = 1e-2, 2.2e-7 at 1 and 5.1e-7
    (4.3 ulp) at 3, with R0's own 5.7e-8.  Since the forward forms the value in fp64 and rounds once (tests/test_gpu_grad_envelope.py
    D found 13 u of R R^T - I near pi): rotation err 2.3e-8 .. 3.3e-8 at every non-zero angle, max|R^T R - I| 5.7e-8 .. 1.1e-7 (0.93 ulp);
    d_rot as before."""
    from consistentnerf_amd import ops
    c2w0, rot, trans, G = _compose_inputs(N, mag)
    v64, r64, t64 = _compose_ref(c2w0, rot, trans, G, torch.float64)
    v32, r32, t32 = _compose_ref(c2w0, rot, trans, G, torch.float32)
    d0, drot, dtr = T(c2w0, dev), T(rot, dev), T(trans, dev)
    c2w = ops.pose_compose(d0, drot, dtr)
    assert c2w.shape == (N, 3, 4)
    g_rot, g_trans = ops.pose_compose_bwd(d0, drot, T(G, dev))
    _check(f"c2w (N {N}, |rot| {mag:g})", c2w, v64, v32)
    _check(f"its rotation (N {N}, |rot| {mag:g})", c2w[:, :, :3], v64[:, :, :3], v32[:, :, :3])
    _check(f"d_rot (N {N}, |rot| {mag:g})", g_rot, r64, r32)
    _check(f"d_trans (N {N}, |rot| {mag:g})", g_trans, t64, t32)
    R = c2w[:, :, :3].double().cpu()
    ortho = float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max())
    R0 = T(c2w0)[:, :, :3].double()
    print(f"  max|R^T R - I| = {ortho:.3e} = {ortho / ULP1:.2f} ulp (R0 itself: {float((R0.transpose(1, 2) @ R0 - torch.eye(3, dtype=torch.float64)).abs().max()):.3e})")
    assert ortho <= 8 * ULP1
    assert torch.equal(c2w[:, :, 3].cpu(), T(c2w0)[:, :, 3] + T(trans))
    if mag == 0.0:
        assert torch.equal(c2w[:, :, :3], d0[:, :, :3])
        gen = torch.stack([(T(G)[:, :, :3] * (P.hat(torch.eye(3)[k:k + 1]) @ T(c2w0)[:, :, :3])).sum((1, 2)) for k in range(3)], -1)
        assert float((g_rot.cpu() - gen).abs().max()) <= 1e-5 * float(gen.abs().max())
    only_rot = ops.pose_compose_bwd(d0, drot, T(G, dev), True, False)
    only_trans = ops.pose_compose_bwd(d0, drot, T(G, dev), False, True)
    assert only_rot[1] is None and only_trans[0] is None and torch.equal(only_rot[0], g_rot) and torch.equal(only_trans[1], g_trans)


# ------------------------------------------------------------------------------------------------ wiring
WH, WW = 9, 11
WK = [[24.0, 0.0, 5.25], [0.0, 22.0, 4.75], [0.0, 0.0, 1.0]]


def _look_at(o, tgt):
    """OpenGL camera at o looking at tgt (down its -z, +y up)."""
    z = (o - tgt) / np.linalg.norm(o - tgt)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), o[:, None]], 1)


def _wiring_poses(dev):
    """Three cameras on the shell of radius 4 looking near the origin (the geometry of _inputs.ray_batch: near 2 / far 6 then span the
    region in which the random networks have density — a ray that meets none takes no gradient at all), moved off their initial
    poses by rot ~ 0.05 rad and trans ~ 0.1 so that the composition's backward is not at its trivial point."""
    from consistentnerf_amd.pose import CameraPoses
    rs = np.random.RandomState(23)

    def cam():
        o = rs.normal(size=3)
        return _look_at(4.0 * o / np.linalg.norm(o), rs.uniform(-0.3, 0.3, size=3))
    poses = CameraPoses(T(np.stack([cam() for _ in range(3)]).astype(np.float32), dev))
    with torch.no_grad():
        poses.rot.copy_(T((0.05 * rs.normal(size=(3, 3))).astype(np.float32), dev))
        poses.trans.copy_(T((0.1 * rs.normal(size=(3, 3))).astype(np.float32), dev))
    coords = T(np.stack([rs.randint(0, WH, size=37), rs.randint(0, WW, size=37)], -1).astype(np.int64), dev)
    view = T(rs.randint(0, 3, size=37).astype(np.int64), dev)
    return poses, coords, view


@pytest.mark.parametrize("chunk", [16, 4096])
@pytest.mark.parametrize("vd", [True, False])
def test_pose_gradients_through_render(dev, vd, chunk):
    """CameraPoses (N = 3) -> get_rays_at (37 pixels over the three views) -> render(rays=(o, d), ndc=False) of two D4 / W128 networks, 16 + 16
    samples, the mixed loss of test_rays_form_against_float64 -> backward: poses.rot.grad and poses.trans.grad are finite, non-zero and equal, bit for
    bit, ops.pose_compose_bwd(ops.gen_rays_at_bwd(o.grad, d.grad)) on the rays' gradients autograd kept."""
    from consistentnerf_amd import ops, run_nerf_view as V
    from consistentnerf_amd.run_nerf_helpers import get_rays_at
    (coarse, _), (fine, _) = make_model(4, 128, vd, 5, 31, dev), make_model(4, 128, vd, 5, 32, dev)
    poses, coords, view = _wiring_poses(dev)
    c2w = poses()
    assert c2w.shape == (3, 3, 4) and c2w.requires_grad
    o, d = get_rays_at(WH, WW, WK, c2w, coords, view)
    assert o.shape == (37, 3) and d.shape == (37, 3) and o.requires_grad and d.requires_grad
    o.retain_grad(), d.retain_grad()
    rgb, disp, acc, depth, extras = V.render(1, 1, KCAM, chunk=chunk, rays=(o, d), ndc=False, near=NEAR, far=FAR, use_viewdirs=vd,
                                             **_kwargs(coarse, fine, 16, 16, 0.0, False, 0.0, False))
    maps = dict(extras, rgb_map=rgb, depth_map=depth, acc_map=acc)
    rs = np.random.RandomState(7)
    G = {k: rs.normal(size=(37, 3) if k.startswith("rgb") else (37,)).astype(np.float32) for k in ("rgb_map", "depth_map", "acc_map", "rgb0", "depth0")}
    _loss(maps, G, lambda g: T(g, dev)).backward()
    d_c2w = ops.gen_rays_at_bwd(o.grad, d.grad, WH, WW, WK, 3, coords, view)
    want_rot, want_trans = ops.pose_compose_bwd(poses.c2w0, poses.rot.detach(), d_c2w)
    for name, got, want in (("rot", poses.rot.grad, want_rot), ("trans", poses.trans.grad, want_trans)):
        assert got is not None and got.shape == (3, 3) and torch.isfinite(got).all() and got.abs().min() > 0, name
        assert torch.equal(got, want), name
    assert coarse.kernel_tensors()[0].grad is not None      # (the networks learn in the same backward)


def test_camera_poses_module(dev):
    """Zero-initialised parameters (forward() = c2w0 bit for bit), the freeze flags, c2w(i), a [N,4,4] initial pose, and ordinary GPU
    parameters: one torch.optim.Adam step moves them."""
    from consistentnerf_amd.pose import CameraPoses
    c2w0 = T(_poses(3, 2), dev)
    poses = CameraPoses(torch.cat([c2w0, torch.tensor([0.0, 0, 0, 1], device=dev).expand(3, 1, 4)], 1))
    assert [n for n, _ in poses.named_parameters()] == ["rot", "trans"] and all(p.is_cuda and not p.any() for p in poses.parameters())
    assert torch.equal(poses.c2w0, c2w0) and torch.equal(poses(), c2w0) and torch.equal(poses.c2w(1), c2w0[1])
    opt = torch.optim.Adam(poses.parameters(), lr=1e-2)
    (poses() * T(np.random.RandomState(0).normal(size=(3, 3, 4)).astype(np.float32), dev)).sum().backward()
    opt.step()
    assert poses.rot.abs().min() > 0 and poses.trans.abs().min() > 0 and not torch.equal(poses(), c2w0)
    frozen = CameraPoses(c2w0, learn_rot=False)
    frozen().sum().backward()
    assert frozen.rot.grad is None and torch.equal(frozen.trans.grad, torch.ones(3, 3, device=dev))
    assert not CameraPoses(c2w0, learn_rot=False, learn_trans=False)().requires_grad


@pytest.mark.parametrize("rows", [3, 4])
def test_get_rays_keeps_the_pose_graph(dev, rows):
    """get_rays(H, W, K, pose) with a [3,4] / [4,4] device pose requiring grad on a 6 x 8 image: the rays carry a graph, the forward
    equals the no-grad call bit for bit, pose.grad of (rays_o * Go + rays_d * Gd).sum() passes the float64 check, and the bottom row of
    a 4 x 4 pose gets zeros.  run_nerf_view.get_rays is the same function.  Measured on the MI355X: err 3.4e-8 (float32 restatement 1.1e-7)."""
    from consistentnerf_amd import run_nerf_view as V
    from consistentnerf_amd.run_nerf_helpers import get_rays
    assert V.get_rays is get_rays
    H, W = 6, 8
    c2w = _poses(1, 31)[0]
    G_o, G_d = _upstream(H * W, seed=4)
    full = np.concatenate([c2w, [[0, 0, 0, 1]]], 0).astype(np.float32)[:rows]
    pose = T(full, dev).requires_grad_(True)
    o, d = get_rays(H, W, K1, pose)
    assert o.shape == (H, W, 3) and d.shape == (H, W, 3) and o.requires_grad and d.requires_grad
    o0, d0 = get_rays(H, W, K1, pose.detach())
    assert not d0.requires_grad and torch.equal(o, o0) and torch.equal(d, d0)
    with torch.no_grad():
        assert not get_rays(H, W, K1, pose)[1].requires_grad
    ((o * T(G_o, dev).view(H, W, 3)).sum() + (d * T(G_d, dev).view(H, W, 3)).sum()).backward()
    assert pose.grad.shape == (rows, 4)
    g64 = _ref_grad(H, W, 1, None, None, 0, H * W, c2w[None], G_o, G_d, torch.float64)
    g32 = _ref_grad(H, W, 1, None, None, 0, H * W, c2w[None], G_o, G_d, torch.float32)
    _check(f"pose.grad ([{rows},4])", pose.grad[:3].reshape(1, 12), g64, g32)
    if rows == 4:
        assert not pose.grad[3].any()


def test_get_rays_without_grad_takes_none_of_the_new_paths(dev, monkeypatch):
    """A pose that does not require grad (tensor or host array): none of the new ops functions is called, and the values are those of
    ops.gen_rays."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.run_nerf_helpers import get_rays
    calls = []
    for name in ("gen_rays_at", "gen_rays_at_bwd", "pose_compose", "pose_compose_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    c2w = _poses(1, 31)[0]
    want = ops.gen_rays(6, 8, K1, c2w, 0.0, 1.0, False, False, dev)
    for pose in (T(c2w, dev), c2w, T(c2w)):
        o, d = get_rays(6, 8, K1, pose)
        assert torch.equal(o.reshape(-1, 3), want[:, 0:3]) and torch.equal(d.reshape(-1, 3), want[:, 3:6])
    assert not calls, calls


def test_render_c2w_requiring_grad_still_raises(dev):
    """render(c2w=pose) with the pose requiring grad raises CnerfError naming c2w (and get_rays, the route that now works)."""
    from consistentnerf_amd import ops, run_nerf_view as V
    coarse, _ = make_model(2, 64, True, 5, 21, dev)
    pose = torch.eye(4, device=dev)[:3].requires_grad_(True)
    with pytest.raises(ops.CnerfError, match="c2w.*get_rays"):
        V.render(4, 4, KCAM, c2w=pose, ndc=False, near=NEAR, far=FAR, use_viewdirs=True, **_kwargs(coarse, None, 8, 0, 0.0, False, 0.0, False))
