"""CPU-side tests of the camera pose gradient: the restatement the GPU tests check the kernels against (tests/_pose_ref.py) reproduces
the reference's own get_rays and its autograd (fixture `pose_grad_tiny`, tests/golden/make_golden_pose.py), its pose composition agrees
with central differences, and the five new C entry points are declared, bound, exported and reject bad arguments before any launch
(probed through the library with dummy host buffers, no device)."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

import _pose_ref as P
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnerf_gen_rays_at", "cnerf_gen_rays_at_bwd_ws_floats", "cnerf_gen_rays_at_bwd", "cnerf_pose_compose",
                "cnerf_pose_compose_bwd")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_restatement_reproduces_the_reference():
    """_pose_ref.get_rays_at over all pixels of the 5 x 7 camera (non-centred principal point, fx != fy) against the reference's
    H.get_rays driven with a pose requiring grad: rays bit for bit in float32, d_c2w within 1e-12 (relative to its largest element) in
    float64 — the same ATen operations — and within 1e-6 in float32 (35-term sums in another order)."""
    g = golden("pose_grad_tiny")
    K, (H, W) = g["K"].tolist(), g["G_o"].shape[:2]
    coords = P.pixel_coords(H, W)
    for dtype, sfx, tol in ((torch.float32, "", 1e-6), (torch.float64, "64", 1e-12)):
        pose = T(g["c2w"]).to(dtype).requires_grad_(True)
        o, d = P.get_rays_at(H, W, K, pose, coords)
        assert o.dtype == dtype and o.shape == (H * W, 3) and d.shape == (H * W, 3)
        ((o * T(g["G_o"]).to(dtype).reshape(-1, 3)).sum() + (d * T(g["G_d"]).to(dtype).reshape(-1, 3)).sum()).backward()
        for name, got in (("rays_o", o), ("rays_d", d)):
            want = g[name + sfx].reshape(-1, 3)
            if dtype == torch.float32:
                assert np.array_equal(got.detach().numpy(), want), name
            else:
                assert np.abs(got.detach().numpy() - want).max() <= 1e-15 * np.abs(want).max(), name
        want = g["d_c2w" + sfx]
        err = np.abs(pose.grad.numpy() - want).max() / np.abs(want).max()
        print(f"  d_c2w {dtype}: err {err:.3e} (tol {tol:g})")
        assert err <= tol
    # a subset with duplicates, out of order, equals indexing the full image
    sel = torch.tensor([[4, 6], [0, 0], [2, 3], [4, 6], [1, 5]])
    o, d = P.get_rays_at(H, W, K, T(g["c2w"]), sel)
    flat = sel[:, 0] * W + sel[:, 1]
    assert np.array_equal(d.numpy(), g["rays_d"].reshape(-1, 3)[flat]) and np.array_equal(o.numpy(), g["rays_o"].reshape(-1, 3)[flat])


def test_views_select_their_pose():
    """view picks the pose per ray; a pose no ray uses gets an exactly zero gradient."""
    g = golden("pose_grad_tiny")
    K = g["K"].tolist()
    rs = np.random.RandomState(3)
    poses = torch.stack([T(g["c2w"]).double() + 0.1 * n for n in range(3)]).requires_grad_(True)
    coords, view = T(rs.randint(0, 5, size=(11, 2))), T(rs.choice([0, 2], size=11))
    o, d = P.get_rays_at(5, 7, K, poses, coords, view)
    for b in range(11):
        ob, db = P.get_rays_at(5, 7, K, poses[int(view[b])], coords[b:b + 1])
        assert torch.equal(ob[0], o[b]) and torch.equal(db[0], d[b])
    (o.sum() + (d * d).sum()).backward()
    assert not poses.grad[1].any() and poses.grad[0].any() and poses.grad[2].any()


def test_composition_against_central_differences():
    """_pose_ref.pose_compose in float64: a rotation (R^T R = I, det 1) times R0, the translation added; c2w0 bit for bit at rot = 0;
    and autograd of a random linear functional against central differences with h = 1e-6 (truncation h^2 ~ 1e-12, round-off
    1e-16 / h ~ 1e-10: about 1e-9 in all; asserted <= 1e-6) at |rot| = 0 exactly and 1e-6 .. 3."""
    rs = np.random.RandomState(11)
    N = 3
    c2w0 = T(np.stack([np.concatenate([np.linalg.qr(rs.normal(size=(3, 3)))[0], rs.normal(size=(3, 1))], 1) for _ in range(N)]))
    G = T(rs.normal(size=(N, 3, 4)))
    h = 1e-6
    for mag in (0.0, 1e-6, 1e-4, 1e-2, 1.0, 3.0):
        ax = rs.normal(size=(N, 3))
        rot = T(ax / np.linalg.norm(ax, axis=-1, keepdims=True) * mag).requires_grad_(True)
        trans = T(rs.normal(size=(N, 3))).requires_grad_(True)
        c2w = P.pose_compose(c2w0, rot, trans)
        R = (c2w[:, :, :3] @ c2w0[:, :, :3].transpose(1, 2)).detach()
        assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14
        assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-14
        assert torch.equal(c2w[:, :, 3], c2w0[:, :, 3] + trans)
        if mag == 0.0:
            assert torch.equal(c2w[:, :, :3], c2w0[:, :, :3])
        (c2w * G).sum().backward()
        f = lambda r, t: float((P.pose_compose(c2w0, r, t) * G).sum())  # noqa: E731
        worst = 0.0
        for which, p in (("rot", rot), ("trans", trans)):
            for n in range(N):
                for k in range(3):
                    e = torch.zeros(N, 3, dtype=torch.float64)
                    e[n, k] = h
                    args = lambda s: (rot.detach() + s * e, trans.detach()) if which == "rot" else (rot.detach(), trans.detach() + s * e)  # noqa: E731
                    fd = (f(*args(1)) - f(*args(-1))) / (2 * h)
                    worst = max(worst, abs(fd - float(p.grad[n, k])))
        scale = float(max(rot.grad.abs().max(), trans.grad.abs().max()))
        print(f"  |rot| = {mag:g}: largest |autograd - central difference| / largest gradient = {worst / scale:.2e}")
        assert worst / scale <= 1e-6
    # at rot = 0 the gradient is the three generators applied to R0: d/d rot_k <G_R, Exp(rot) R0> = <G_R, hat(e_k) R0>
    rot = torch.zeros(N, 3, dtype=torch.float64, requires_grad=True)
    (P.pose_compose(c2w0, rot, torch.zeros(N, 3, dtype=torch.float64)) * G).sum().backward()
    gen = torch.stack([(G[:, :, :3] * (P.hat(torch.eye(3, dtype=torch.float64)[k:k + 1]) @ c2w0[:, :, :3])).sum((1, 2)) for k in range(3)], -1)
    assert float((rot.grad - gen).abs().max()) <= 1e-15


def test_entry_points_declared_bound_and_exported():
    """The five entry points are in include/cnerf.h (with the ABI number still 6), in _lib.SIGNATURES, and exported by the built
    library."""
    import ctypes as C
    from consistentnerf_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "cnerf.h")).read()
    assert "#define CNERF_ABI_VERSION 6" in header
    lib = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"^int(64_t)? %s\(" % name, header, re.M), f"{name} is not declared in include/cnerf.h"
        assert name in L.SIGNATURES, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libcnerf_hip.so"
    assert "H:164-173" in header[header.index("cnerf_pack_rays_bwd("):]


def test_entry_points_reject_bad_arguments():
    """cnerf_gen_rays_at / cnerf_gen_rays_at_bwd / cnerf_pose_compose / cnerf_pose_compose_bwd return CNERF_E_ARG for null pointers,
    B <= 0, n_views <= 0, H / W <= 0, zero fx / fy, a row-major window outside the image, a misaligned workspace and a negative
    grid — before any launch (dummy host buffers stand in for the device pointers: nothing dereferences them), in a child process
    like test_lossforms_host.py; the workspace query counts 12 doubles per view and chunk of 64 rays."""
    code = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
from consistentnerf_amd import _lib as L
lib = C.CDLL(L.LIB_PATH)
for n in %r:
    f = getattr(lib, n); f.restype, f.argtypes = L.SIGNATURES[n]
buf = (C.c_double * 4096)()
p = C.cast(buf, C.c_void_p)
odd = C.c_void_p(p.value + 4)
ws = lib.cnerf_gen_rays_at_bwd_ws_floats
out = {"ws_1_1": ws(1, 1), "ws_64_1": ws(64, 1), "ws_65_3": ws(65, 3), "ws_4096_3": ws(4096, 3), "ws_0_1": ws(0, 1), "ws_5_0": ws(5, 0),
       "ws_m1_1": ws(-1, 1)}
def fwd(H=5, W=7, fx=6.5, fy=5.75, c2w=p, nv=1, coords=None, view=None, first=0, B=35, o=p, d=p):
    return lib.cnerf_gen_rays_at(H, W, fx, fy, 3.25, 2.75, c2w, nv, coords, view, first, B, o, d, None)
def bwd(H=5, W=7, fx=6.5, fy=5.75, do=p, dd=p, nv=1, coords=None, view=None, first=0, B=35, dc=p, w=p, grid=0):
    return lib.cnerf_gen_rays_at_bwd(H, W, fx, fy, 3.25, 2.75, do, dd, nv, coords, view, first, B, dc, w, grid, None)
for tag, f in (("fwd", fwd), ("bwd", bwd)):
    out[tag + "_H0"] = f(H=0)
    out[tag + "_Wneg"] = f(W=-3)
    out[tag + "_fx0"] = f(fx=0.0)
    out[tag + "_fy0"] = f(fy=0.0)
    out[tag + "_nv0"] = f(nv=0)
    out[tag + "_B0"] = f(B=0)
    out[tag + "_Bneg"] = f(B=-4)
    out[tag + "_B0_coords"] = f(B=0, coords=p)
    out[tag + "_window_past_end"] = f(first=1, B=35)
    out[tag + "_first_neg"] = f(first=-1, B=3)
out["fwd_null_c2w"] = fwd(c2w=None)
out["fwd_null_o"] = fwd(o=None)
out["fwd_null_d"] = fwd(d=None)
out["bwd_null_do"] = bwd(do=None)
out["bwd_null_dd"] = bwd(dd=None)
out["bwd_null_dc2w"] = bwd(dc=None)
out["bwd_null_ws"] = bwd(w=None)
out["bwd_odd_ws"] = bwd(w=odd)
out["bwd_grid_neg"] = bwd(grid=-1)
out["compose_null_c2w0"] = lib.cnerf_pose_compose(None, p, p, 3, p, None)
out["compose_null_rot"] = lib.cnerf_pose_compose(p, None, p, 3, p, None)
out["compose_null_trans"] = lib.cnerf_pose_compose(p, p, None, 3, p, None)
out["compose_null_out"] = lib.cnerf_pose_compose(p, p, p, 3, None, None)
out["compose_N0"] = lib.cnerf_pose_compose(p, p, p, 0, p, None)
out["compose_Nneg"] = lib.cnerf_pose_compose(p, p, p, -2, p, None)
out["cbwd_null_c2w0"] = lib.cnerf_pose_compose_bwd(None, p, p, 3, p, p, None)
out["cbwd_null_rot"] = lib.cnerf_pose_compose_bwd(p, None, p, 3, p, p, None)
out["cbwd_null_g"] = lib.cnerf_pose_compose_bwd(p, p, None, 3, p, p, None)
out["cbwd_no_output"] = lib.cnerf_pose_compose_bwd(p, p, p, 3, None, None, None)
out["cbwd_N0"] = lib.cnerf_pose_compose_bwd(p, p, p, 0, p, p, None)
for k, v in out.items():
    print(k, v, flush=True)
""" % (ROOT, ENTRY_POINTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    seen = {k: int(v) for k, v in (ln.split() for ln in r.stdout.strip().splitlines())}
    assert [seen.pop(k) for k in ("ws_1_1", "ws_64_1", "ws_65_3", "ws_4096_3", "ws_0_1", "ws_5_0", "ws_m1_1")] == \
        [24, 24, 2 * 12 * 3 * 2, 2 * 12 * 3 * 64, 0, 0, 0]
    assert len(seen) == 40 and all(v == -1 for v in seen.values()), {k: v for k, v in seen.items() if v != -1}
