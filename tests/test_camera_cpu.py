"""CPU-side tests of the NDC and intrinsics gradients: the restatement the GPU tests check the kernels against
(tests/_camera_ref.py) reproduces the reference's own get_rays + ndc_rays and their autograd w.r.t. the pose and K (fixture
`ndc_grad_tiny`, tests/golden/make_golden_ndc.py); pose.CameraIntrinsics starts at K0 and agrees with central differences; the four
new C entry points are declared, bound, exported and reject bad arguments before any launch (probed through the library with
dummy host buffers, no device)."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

import _camera_ref as CR
import _pose_ref as P
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnerf_camera_rows", "cnerf_camera_rows_bwd_ws_floats", "cnerf_camera_rows_bwd", "cnerf_ndc_rays_bwd")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_restatement_reproduces_the_reference():
    """_camera_ref.rows over all pixels of the 5 x 7 forward-facing camera against the reference's H.get_rays + H.ndc_rays (+ the
    view directions of the pre-NDC rays) driven with a pose and a K requiring grad: the NDC origins, NDC directions and view
    directions bit for bit in float32, d_c2w and d_K within 1e-12 (relative to the largest element of each) in float64 — the same
    ATen operations — and within 1e-5 in float32 (printed)."""
    g = golden("ndc_grad_tiny")
    H, W = g["G_o"].shape[:2]
    coords = P.pixel_coords(H, W)
    G = np.concatenate([g["G_o"].reshape(-1, 3), g["G_d"].reshape(-1, 3), np.zeros((H * W, 2), np.float32), g["G_v"].reshape(-1, 3)], -1)
    assert CR.min_abs_dz(H, W, g["K"].tolist(), g["c2w"], coords, None) >= 0.85
    for dtype, sfx, tol in ((torch.float32, "", 1e-5), (torch.float64, "64", 1e-12)):
        K = T(g["K"]).to(dtype).requires_grad_(True)
        pose = T(g["c2w"]).to(dtype).requires_grad_(True)
        r = CR.rows(H, W, K, pose, coords, None, 0., 1., True, True)
        assert r.dtype == dtype and r.shape == (H * W, 11)
        (r * T(G).to(dtype)).sum().backward()
        got = torch.cat([r[:, 0:6], r[:, 8:11]], -1).detach().numpy()
        assert np.array_equal(r[:, 6:8].detach().numpy(), np.tile([[0., 1.]], (H * W, 1)))
        if dtype == torch.float32:
            assert np.array_equal(got, g["rows"]), "the float32 rows differ from the reference's"
        else:
            assert np.abs(got - g["rows64"]).max() <= 1e-15 * np.abs(g["rows64"]).max()
        for name, grad in (("d_c2w", pose.grad), ("d_K", K.grad)):
            want = g[name + sfx]
            err = np.abs(grad.numpy() - want).max() / np.abs(want).max()
            print(f"  {name} {dtype}: err {err:.3e} (tol {tol:g})")
            assert err <= tol, name
    # the reference's K gradient reaches exactly the four entries the kernel reads
    assert set(zip(*np.nonzero(g["d_K64"]))) == {(0, 0), (1, 1), (0, 2), (1, 2)}


def test_coefficient_paths_are_visible_in_d_K():
    """With the graph from K[0][0] to the two NDC coefficients cut (coef_paths=False) the float64 d_K[0][0] moves by far more than
    the 1e-5 the GPU test allows, every other gradient entry not at all: the GPU must-fail check rests on this."""
    g = golden("ndc_grad_tiny")
    H, W = g["G_o"].shape[:2]
    coords = P.pixel_coords(H, W)
    G = np.concatenate([g["G_o"].reshape(-1, 3), g["G_d"].reshape(-1, 3), np.zeros((H * W, 2), np.float32), g["G_v"].reshape(-1, 3)], -1)
    _, c_full, k_full = CR.grads(H, W, g["K"].tolist(), g["c2w"], coords, None, G, True, True, torch.float64)
    _, c_cut, k_cut = CR.grads(H, W, g["K"].tolist(), g["c2w"], coords, None, G, True, True, torch.float64, coef_paths=False)
    assert torch.equal(c_full, c_cut)
    diff = (k_full - k_cut).abs()
    assert float(diff[0, 0]) > 1e-3 * float(k_full.abs().max())
    diff[0, 0] = 0
    assert not diff.any()


def test_camera_intrinsics_module():
    """pose.CameraIntrinsics on the CPU: zero parameters and forward() == K0 bit for bit (tied and untied, float32 and float64);
    the freeze flags; in float64 the gradient of a random linear functional of K w.r.t. log_focal / center against central
    differences with h = 1e-6 (truncation h^2 ~ 1e-12, round-off 1e-16 / h ~ 1e-10; asserted <= 1e-6 of the largest gradient)."""
    from consistentnerf_amd.pose import CameraIntrinsics
    K0 = T(np.asarray(CR.K1, np.float32))
    G = T(np.random.RandomState(2).normal(size=(3, 3)))
    for tie in (True, False):
        m = CameraIntrinsics(K0, learn_focal=True, learn_center=True, tie_focal=tie)
        assert [n for n, _ in m.named_parameters()] == ["log_focal", "center"] and not any(p.any() for p in m.parameters())
        assert m.log_focal.shape == (1 if tie else 2,) and m.center.shape == (2,)
        assert m().dtype == torch.float32 and torch.equal(m(), K0) and m().requires_grad
        m = m.double()
        assert torch.equal(m(), K0.double())
        rs = np.random.RandomState(3)
        with torch.no_grad():
            m.log_focal.copy_(T(rs.uniform(-0.2, 0.2, size=m.log_focal.shape)))
            m.center.copy_(T(rs.uniform(-1, 1, size=2)))
        K = m()
        e = torch.exp(m.log_focal.detach())
        assert torch.allclose(K[0, 0], K0[0, 0].double() * e[0], rtol=1e-15) and torch.allclose(K[1, 1], K0[1, 1].double() * e[-1], rtol=1e-15)
        assert torch.equal(K[0, 2], K0[0, 2].double() + m.center[0]) and torch.equal(K[1, 2], K0[1, 2].double() + m.center[1])
        assert torch.equal(K[2], K0[2].double()) and K[0, 1] == 0 and K[1, 0] == 0
        (K * G).sum().backward()
        h, worst = 1e-6, 0.0
        for p in (m.log_focal, m.center):
            for k in range(p.numel()):
                vals = []
                for s in (1, -1):
                    with torch.no_grad():
                        p[k] += s * h
                        vals.append(float((m() * G).sum()))
                        p[k] -= s * h
                worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - float(p.grad[k])))
        scale = float(max(m.log_focal.grad.abs().max(), m.center.grad.abs().max()))
        print(f"  tie_focal={tie}: largest |autograd - central difference| / largest gradient = {worst / scale:.2e}")
        assert worst / scale <= 1e-6
    frozen = CameraIntrinsics(K0, learn_focal=False, learn_center=False)
    assert not frozen().requires_grad and torch.equal(frozen(), K0)
    only_center = CameraIntrinsics(K0, learn_focal=False, learn_center=True)
    only_center().sum().backward()
    assert only_center.log_focal.grad is None and torch.equal(only_center.center.grad, torch.ones(2))


def test_entry_points_declared_bound_and_exported():
    """The four entry points are in include/cnerf.h (with the ABI number still 6, after every earlier declaration: append-only), in
    _lib.SIGNATURES, and exported by the built library; the Python surface exists."""
    import ctypes as C
    from consistentnerf_amd import _lib as L, ops, pose
    header = open(os.path.join(ROOT, "include", "cnerf.h")).read()
    assert "#define CNERF_ABI_VERSION 6" in header
    lib = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"^int(64_t)? %s\(" % name, header, re.M), f"{name} is not declared in include/cnerf.h"
        assert name in L.SIGNATURES, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libcnerf_hip.so"
    tail = header[header.index("int cnerf_pose_compose_bwd("):]
    assert all(name + "(" in tail for name in ENTRY_POINTS) and all(ref in tail for ref in ("H:164-173", "R:103-116", "H:186-202"))
    assert list(L.SIGNATURES)[-4:] == list(ENTRY_POINTS)
    for mod, names in ((ops, ("camera_rows", "camera_rows_bwd", "ndc_rays_bwd")), (pose, ("camera_rows", "CameraIntrinsics"))):
        assert all(callable(getattr(mod, n)) for n in names)


def test_entry_points_reject_bad_arguments():
    """cnerf_camera_rows / cnerf_camera_rows_bwd / cnerf_ndc_rays_bwd return CNERF_E_ARG for null pointers, B <= 0, n_views <= 0,
    H / W <= 0, zero fx / fy on the host source, a row-major window outside the image, a misaligned workspace and a negative grid —
    before any launch (dummy host buffers stand in for the device pointers: nothing dereferences them), in a child process like
    test_pose_cpu.py; the workspace query counts 12 doubles per view and 4 for K, per chunk of 64 rays."""
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
ws = lib.cnerf_camera_rows_bwd_ws_floats
out = {"ws_1_1": ws(1, 1), "ws_64_1": ws(64, 1), "ws_65_3": ws(65, 3), "ws_4096_3": ws(4096, 3), "ws_0_1": ws(0, 1), "ws_5_0": ws(5, 0),
       "ws_m1_1": ws(-1, 1)}
def fwd(H=5, W=7, fx=6.5, fy=5.75, K=None, c2w=p, nv=1, coords=None, view=None, first=0, B=35, rows=p):
    return lib.cnerf_camera_rows(H, W, fx, fy, 3.25, 2.75, -1.0, -1.0, K, c2w, nv, coords, view, first, B, 0.0, 1.0, 1, 1, rows, None)
def bwd(H=5, W=7, fx=6.5, fy=5.75, K=None, c2w=p, nv=1, coords=None, view=None, first=0, B=35, g=p, dc=p, dk=p, w=p, grid=0):
    return lib.cnerf_camera_rows_bwd(H, W, fx, fy, 3.25, 2.75, -1.0, -1.0, K, c2w, nv, coords, view, first, B, 1, 1, g, dc, dk, w, grid,
                                     None)
for tag, f in (("fwd", fwd), ("bwd", bwd)):
    out[tag + "_H0"] = f(H=0)
    out[tag + "_Wneg"] = f(W=-3)
    out[tag + "_fx0"] = f(fx=0.0)
    out[tag + "_fy0"] = f(fy=0.0)
    out[tag + "_nv0"] = f(nv=0)
    out[tag + "_B0"] = f(B=0)
    out[tag + "_Bneg"] = f(B=-4)
    out[tag + "_B0_coords"] = f(B=0, coords=p)
    out[tag + "_B0_devK"] = f(B=0, K=p)
    out[tag + "_window_past_end"] = f(first=1, B=35)
    out[tag + "_first_neg"] = f(first=-1, B=3)
    out[tag + "_null_c2w"] = f(c2w=None)
out["fwd_null_rows"] = fwd(rows=None)
out["bwd_null_g"] = bwd(g=None)
out["bwd_no_output"] = bwd(dc=None, dk=None)
out["bwd_null_ws"] = bwd(w=None)
out["bwd_odd_ws"] = bwd(w=odd)
out["bwd_grid_neg"] = bwd(grid=-1)
def nb(go=p, gd=p, o=p, d=p, B=35, do=p, dd=p):
    return lib.cnerf_ndc_rays_bwd(go, gd, o, d, B, -1.0, -1.0, do, dd, None)
for k in ("go", "gd", "o", "d", "do", "dd"):
    out["ndc_null_" + k] = nb(**{k: None})
out["ndc_B0"] = nb(B=0)
out["ndc_Bneg"] = nb(B=-1)
for k, v in out.items():
    print(k, v, flush=True)
""" % (ROOT, ENTRY_POINTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    seen = {k: int(v) for k, v in (ln.split() for ln in r.stdout.strip().splitlines())}
    assert [seen.pop(k) for k in ("ws_1_1", "ws_64_1", "ws_65_3", "ws_4096_3", "ws_0_1", "ws_5_0", "ws_m1_1")] == \
        [2 * 16, 2 * 16, 2 * (12 * 3 + 4) * 2, 2 * (12 * 3 + 4) * 64, 0, 0, 0]
    assert len(seen) == 38 and all(v == -1 for v in seen.values()), {k: v for k, v in seen.items() if v != -1}
