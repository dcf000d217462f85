"""CPU-side tests of the loss forms other than `--hardmask` (run_nerf_view.render_loss(rgb_form=, depth_form=)): the ATen
restatement of the reference's lines that the GPU tests check the kernels against reproduces the reference's own values and
gradients (fixture `lossforms`, tests/golden/make_golden_lossforms.py), render_loss enforces its argument rules before it touches
the library, and the new C entry points reject null, empty and out-of-range arguments (probed through the library, no device)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 6.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def eq(a, b, name=""):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=True), f"{name}: max|d|={np.nanmax(np.abs(a.astype(np.float64) - b))}"


def test_softmask_lambdas_golden():
    """img2mse_softmask / img2mse_depth_softmask (V:50 / V:55) on CPU tensors = the reference's expression: value, d / dx and the
    gradient of the TEMPERATURE (the denominator detaches the residual only) at softplus(-0.7) and 0.1, exactly."""
    from consistentnerf_amd import run_nerf_view as V
    g = golden("lossforms")
    assert abs(float(g["temp.sp"]) - float(torch.nn.functional.softplus(torch.tensor(-0.7)))) < 1e-7 and float(g["temp.p1"]) == np.float32(0.1)
    for tname in ("sp", "p1"):
        for tag, fn, (xk, yk) in (("rgb", V.img2mse_softmask, ("x3", "y3")), ("depth", V.img2mse_depth_softmask, ("x1", "y1"))):
            x = T(g[xk]).requires_grad_(True)
            t = torch.tensor(g[f"temp.{tname}"].item(), dtype=torch.float32, requires_grad=True)
            loss = fn(x, T(g[yk]), t)
            loss.backward()
            eq(loss, g[f"soft.{tag}.{tname}.loss"], "loss")
            eq(x.grad, g[f"soft.{tag}.{tname}.d_x"], f"{tag} {tname} d_x")
            eq(t.grad, g[f"soft.{tag}.{tname}.d_temp"], f"{tag} {tname} d_temp")
            assert float(t.grad) < 0          # a larger temperature flattens the weights: the loss falls


def test_softmask_formulas_equal_autograd():
    """The closed forms the kernels use — L = N / Dn, dL/dt = -(sum(w d^4) / Dn - L^2) / t^2, dL/dd_i = w_i (2 d_i + 2 d_i^3 / t) / Dn —
    against autograd of V:50 in float64."""
    from consistentnerf_amd import run_nerf_view as V
    g = golden("lossforms")
    for tv in (0.40318605, 0.1):
        x = T(g["x3"]).double().requires_grad_(True)
        t = torch.tensor(tv, dtype=torch.float64, requires_grad=True)
        V.img2mse_softmask(x, T(g["y3"]).double(), t).backward()
        d = (x - T(g["y3"]).double()).detach()
        w = torch.exp(d ** 2 / tv)
        Dn, L = w.sum(), (w * d ** 2).sum() / w.sum()
        assert abs(float(-((w * d ** 4).sum() / Dn - L * L) / tv ** 2) - float(t.grad)) <= 1e-12 * abs(float(t.grad))
        assert float((w * (2 * d + 2 * d ** 3 / tv) / Dn - x.grad).abs().max()) <= 1e-14


@pytest.mark.parametrize("mtag", ["mixed", "ones"])
def test_depth_form_lines_golden(mtag):
    """run_nerf_view._form_depth_lines (what `_render_loss_lines` evaluates for "norm" / "plain" / "hardmask_coef") on CPU tensors
    against the reference's own statements V:1762-1771 and VC:1550-1551: loss and d / d depth exactly, with a mixed mask and with an
    all-ones one (the `!= N_rand` guard); the prior the reference leaves behind is where(mask == 0, 0, prior), and OUR caller's
    prior is left alone."""
    from consistentnerf_amd import run_nerf_view as V
    g = golden("lossforms")
    mask = T(g["mask"]) if mtag == "mixed" else torch.ones(512)
    for form, key in (("norm", "norm"), ("plain", "plain"), ("hardmask_coef", "coef")):
        d = T(g["depth"]).requires_grad_(True)
        prior = T(g["prior"]).clone()
        loss = V._form_depth_lines(d, prior, mask, FAR, 0.2, form, 0.0, None, None)
        loss.backward()
        eq(loss, g[f"{key}.{mtag}.loss"], form)
        eq(d.grad, g[f"{key}.{mtag}.d_depth"], form + " d_depth")
        eq(prior, g["prior"], "the caller's prior")
        want_after = g["prior"] if form == "hardmask_coef" else np.where(mask.numpy() == 0, np.float32(0), g["prior"])
        eq(g[f"{key}.{mtag}.prior_after"], want_after, "the reference's prior after its lines")
    assert float(g["norm.ones.loss"]) == float(g["coef.ones.loss"])


def test_render_loss_argument_rules():
    """Every refusal is a ValueError raised before rays are packed or the library is loaded (CPU tensors, no GPU here)."""
    from consistentnerf_amd import run_nerf_view as V
    tgt, rays = torch.zeros(8, 3), (torch.zeros(8, 3), torch.ones(8, 3))
    call = lambda **kw: V.render_loss(4, 4, None, tgt, rays=rays, depth_prior=torch.ones(8), **kw)  # noqa: E731
    t = torch.tensor(0.4)
    for kw, word in ((dict(rgb_form="l1"), "unknown loss form"), (dict(depth_form="softLp"), "unknown loss form"),
                     (dict(rgb_form="softmask"), "temp_rgb"), (dict(depth_form="softmask", temp_rgb=t), "temp_depth"),
                     (dict(rgb_form="softmask", temp_rgb=(t, None)), "temp_rgb"),
                     (dict(rgb_form="softlp"), "lp_coef"), (dict(depth_form="softlp", lp_coef=0.0), "lp_coef"),
                     (dict(depth_form="norm", _ss_coins=(1, 1, 1, 1)), "_ss_coins"),
                     (dict(rgb_form="softlp", lp_coef=1.0, _ss_coins=(1, 0, 1, 0)), "_ss_coins"),
                     (dict(rgb_form="softlp", lp_coef=1.0, counts=torch.tensor([5.0, 3.0])), "counts"),
                     (dict(depth_form="softmask", temp_depth=t, counts=torch.tensor([5.0, 3.0])), "counts")):
        with pytest.raises(ValueError, match=word):
            call(**kw)


def test_new_entry_points_reject_null_empty_and_out_of_range():
    """cnerf_composite_fwd_lossform / cnerf_lossform_finish / cnerf_composite_bwd_lossform / cnerf_softmask_loss return CNERF_E_ARG
    for null pointers, for B = 0 and for a form out of range — before any launch (dummy host buffers stand in for the device
    pointers: nothing dereferences them), in a child process like the null-argument test of test_host.py."""
    code = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
from consistentnerf_amd import _lib as L
lib = C.CDLL(L.LIB_PATH)
for n in ("cnerf_lossform_ws_floats", "cnerf_composite_fwd_lossform", "cnerf_lossform_finish", "cnerf_composite_bwd_lossform", "cnerf_softmask_loss"):
    f = getattr(lib, n); f.restype, f.argtypes = L.SIGNATURES[n]
buf = (C.c_double * 4096)()
p = C.cast(buf, C.c_void_p)
closs = L.Closs(p, p, p, 6.0, 0)
tail = L.ClossTail(p, p, 264, None, 0.2, 6.0, 1.0, 1.0, 0.001, 1, None, None, None, 0, 256)
ok_form = L.LossForm(2, 5, 1.0, p, p)
def fwd(B, cl, fm): return lib.cnerf_composite_fwd_lossform(p, 4, p, p, 8, None, B, 32, 0, cl, fm, p, p, p, p, p, p, None)
def fin(t, f0, f1): return lib.cnerf_lossform_finish(t, f0, f1, 0, 0.0, None, None, None, p, p, None, None, p, None)
def bwd(B, cl, fm, dt=None, gt=None):
    return lib.cnerf_composite_bwd_lossform(p, 4, p, p, 8, None, B, 32, 0, cl, fm, p, p, p, None, 1.0, 1.0, 0.001, 0.2, None, 0, 0.0,
                                            None, 0, dt, gt, p, None)
out = {"ws0": lib.cnerf_lossform_ws_floats(0), "ws264": lib.cnerf_lossform_ws_floats(264), "ws13": lib.cnerf_lossform_ws_floats(13)}
out["fwd_null"] = fwd(264, None, None)
out["fwd_noform"] = fwd(264, C.byref(closs), None)
out["fwd_B0"] = fwd(0, C.byref(closs), C.byref(ok_form))
out["bwd_B0"] = bwd(0, C.byref(closs), C.byref(ok_form))
out["bwd_noform"] = bwd(264, C.byref(closs), None)
out["bwd_half_temp"] = bwd(264, C.byref(closs), C.byref(ok_form), p, None)
for i, (rf, df) in enumerate(((3, 0), (-1, 0), (0, 6), (0, -1))):
    bad = L.LossForm(rf, df, 1.0, p, p)
    out["fwd_range%%d" %% i] = fwd(264, C.byref(closs), C.byref(bad))
    out["bwd_range%%d" %% i] = bwd(264, C.byref(closs), C.byref(bad))
    out["fin_range%%d" %% i] = fin(C.byref(tail), C.byref(bad), C.byref(ok_form))
out["fwd_softmask_no_temp"] = fwd(264, C.byref(closs), C.byref(L.LossForm(2, 0, 0.0, None, None)))
out["fwd_softlp_no_coef"] = fwd(264, C.byref(closs), C.byref(L.LossForm(1, 0, 0.0, None, None)))
out["fin_null"] = fin(None, None, None)
out["fin_no_coarse_form"] = fin(C.byref(tail), C.byref(ok_form), None)
tail0 = L.ClossTail(p, p, 0, None, 0.2, 6.0, 1.0, 1.0, 0.001, 1, None, None, None, 0, 256)
out["fin_B0"] = fin(C.byref(tail0), C.byref(ok_form), C.byref(ok_form))
tailc = L.ClossTail(p, p, 264, p, 0.2, 6.0, 1.0, 1.0, 0.001, 1, None, None, None, 0, 256)
out["fin_soft_counts"] = fin(C.byref(tailc), C.byref(ok_form), C.byref(ok_form))
out["soft_null"] = lib.cnerf_softmask_loss(None, None, 0, None, None, None, None, None)
out["soft_n0"] = lib.cnerf_softmask_loss(p, p, 0, p, p, p, p, None)
out["soft_no_temp"] = lib.cnerf_softmask_loss(p, p, 16, None, p, p, p, None)
for k, v in out.items():
    print(k, v, flush=True)
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    seen = {k: int(v) for k, v in (ln.split() for ln in r.stdout.strip().splitlines())}
    assert seen.pop("ws0") == 0 and seen.pop("ws264") == 2 * 10 * 33 and seen.pop("ws13") == 2 * 10 * 2
    assert len(seen) == 27 and all(v == -1 for v in seen.values()), {k: v for k, v in seen.items() if v != -1}
