"""CPU-side tests of the camera gradients on the folded training step: the three pair entry points (cnerf_mlp_input_grad_pair,
cnerf_rays_input_grad_pair, cnerf_composite_norm_grad_pair) are declared at the end of include/cnerf.h, bound, exported and reject
bad arguments before any launch (probed through the library with dummy host buffers, no device)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnerf_mlp_input_grad_pair", "cnerf_rays_input_grad_pair", "cnerf_composite_norm_grad_pair")


def test_entry_points_declared_bound_and_exported():
    """The three entry points are in include/cnerf.h after cnerf_ndc_rays_bwd (append-only, the ABI number still 6), in
    _lib.SIGNATURES next to cnerf_mlp_input_grad (the camera entry points stay the last four of the dict), and exported by the built
    library; the Python surface exists."""
    import ctypes as C
    import inspect
    from consistentnerf_amd import _lib as L, ops, run_nerf as R, run_nerf_view as V
    header = open(os.path.join(ROOT, "include", "cnerf.h")).read()
    assert "#define CNERF_ABI_VERSION 6" in header
    lib = C.CDLL(L.LIB_PATH)
    tail = header[header.index("int cnerf_ndc_rays_bwd("):]
    for name in ENTRY_POINTS:
        assert len(re.findall(r"^int %s\(" % name, header, re.M)) == 1, f"{name} is not declared (once) in include/cnerf.h"
        assert re.search(r"^int %s\(" % name, tail, re.M), f"{name} is not declared after cnerf_ndc_rays_bwd"
        assert name in L.SIGNATURES, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libcnerf_hip.so"
    assert not re.search(r"^int(64_t)? cnerf_(?!%s)\w+\(" % "|".join(n[6:] for n in ENTRY_POINTS), tail[10:], re.M), \
        "a declaration other than the three follows cnerf_ndc_rays_bwd"
    names = list(L.SIGNATURES)
    at = names.index("cnerf_composite_norm_grad")
    assert names[at + 1:at + 4] == list(ENTRY_POINTS)
    assert names[-1] == "cnerf_ndc_rays_bwd"
    for n in ("mlp_input_grad_pair", "rays_input_grad_pair", "composite_norm_grad_pair"):
        assert callable(getattr(ops, n))
    assert "ws" in inspect.signature(ops.mlp_backward_pair).parameters
    for mod in (R, V):
        p = inspect.signature(mod.render_loss).parameters
        assert "rows" in p and p["rows"].default is None


def test_entry_points_reject_bad_arguments():
    """Each of the three returns CNERF_E_ARG for null pointers, B <= 0, S <= 0, ray_stride < 8 and d_dirs_pt given for a network
    without view directions — before any launch (dummy host buffers stand in for the device pointers: nothing dereferences them), in a
    child process like test_camera_cpu.py."""
    code = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
from consistentnerf_amd import _lib as L
lib = C.CDLL(L.LIB_PATH)
for n in %r:
    f = getattr(lib, n); f.restype, f.argtypes = L.SIGNATURES[n]
buf = (C.c_float * 4096)()
p = C.cast(buf, C.c_void_p)
vd, novd = L.Net(4, 128, 10, 4, 1, 4, 4), L.Net(4, 128, 10, 4, 0, 4, 4)
out = {}
def mlp(n0=vd, pk0=p, B0=3, S0=5, st0=p, ws0=p, dp0=p, dd0=p, n1=vd, pk1=p, B1=3, S1=7, st1=p, ws1=p, dp1=p, dd1=p):
    return lib.cnerf_mlp_input_grad_pair(C.byref(n0), pk0, B0, S0, st0, ws0, dp0, dd0, C.byref(n1), pk1, B1, S1, st1, ws1, dp1, dd1, None)
for lv in "01":
    for k in ("pk", "st", "ws", "dp"):
        out["mlp_null_%%s%%s" %% (k, lv)] = mlp(**{k + lv: None})
    out["mlp_B0_" + lv] = mlp(**{"B" + lv: 0})
    out["mlp_Bneg_" + lv] = mlp(**{"B" + lv: -2})
    out["mlp_S0_" + lv] = mlp(**{"S" + lv: 0})
    out["mlp_Sneg_" + lv] = mlp(**{"S" + lv: -1})
    out["mlp_dirs_without_viewdirs_" + lv] = mlp(**{"n" + lv: novd})
def rays(dp0=p, dd0=p, z0=p, S0=5, dp1=p, dd1=p, z1=p, S1=7, B=3, o=p, rs=11):
    return lib.cnerf_rays_input_grad_pair(dp0, dd0, z0, S0, dp1, dd1, z1, S1, B, o, rs, None)
for k in ("dp0", "z0", "dp1", "z1", "o"):
    out["rays_null_" + k] = rays(**{k: None})
out["rays_one_dirs_0"] = rays(dd1=None)
out["rays_one_dirs_1"] = rays(dd0=None)
out["rays_B0"] = rays(B=0)
out["rays_Bneg"] = rays(B=-1)
out["rays_S0_0"] = rays(S0=0)
out["rays_S0_1"] = rays(S1=0)
out["rays_Sneg"] = rays(S0=-3)
out["rays_stride_7"] = rays(dd0=None, dd1=None, rs=7)
out["rays_stride_0"] = rays(dd0=None, dd1=None, rs=0)
out["rays_dirs_stride_8"] = rays(rs=8)
def norm(dr0=p, r0=p, ch0=4, n0=None, S0=5, dr1=p, r1=p, ch1=5, n1=None, S1=7, rows=p, rs=8, B=3, o=p):
    return lib.cnerf_composite_norm_grad_pair(dr0, r0, ch0, n0, S0, dr1, r1, ch1, n1, S1, rows, rs, B, o, None)
for k in ("dr0", "r0", "dr1", "r1", "rows", "o"):
    out["norm_null_" + k] = norm(**{k: None})
out["norm_B0"] = norm(B=0)
out["norm_Bneg"] = norm(B=-5)
out["norm_S0_0"] = norm(S0=0)
out["norm_S0_1"] = norm(S1=0)
out["norm_ch3_0"] = norm(ch0=3)
out["norm_ch3_1"] = norm(ch1=3)
out["norm_stride_7"] = norm(rs=7)
out["norm_stride_6"] = norm(rs=6)
for k, v in out.items():
    print(k, v, flush=True)
""" % (ROOT, ENTRY_POINTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    seen = {k: int(v) for k, v in (ln.split() for ln in r.stdout.strip().splitlines())}
    assert len(seen) == 2 * 9 + 15 + 14 and all(v == -1 for v in seen.values()), {k: v for k, v in seen.items() if v != -1}
