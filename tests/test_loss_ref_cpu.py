"""Default-run (no GPU) checks of tests/_loss_ref.py, the float64 statements and derived bounds that tests/test_gpu_loss_envelope.py
holds csrc/loss.hip and csrc/adam.hip to:
  * the statements equal the project's own (oracle.mse, mse_soft_lp, masked_rgb_loss, masked_depth_loss, adam_step, patch_depth_loss)
    and the reference's captured values (losses_mask.npz, altlosses.npz, patch.npz);
  * the bounds are not too tight: numpy float32 evaluations in three other association orders stay inside them, and so does the
    fp32 restatement of Adam against its float64 step;
  * the bounds are not loose: every mutant of a statement misses its bound by at least 4x on the GPU test's own inputs (the least
    ratio is printed).
"""
import numpy as np
import pytest
import torch

import _loss_ref as R
from conftest import golden
from oracle import nerf_oracle as O

torch.set_num_threads(4)


def T64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.abs(a - b) <= rel * np.abs(b).max() + 1e-300), (float(np.abs(a - b).max()), float(np.abs(b).max()))


# ------------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("mask_kind", ["mixed", "ones"])
def test_masked64_is_the_oracles_statement(mask_kind):
    """masked64 = oracle.masked_rgb_loss / masked_depth_loss in float64 under autograd (local counts, g_scale 1), 1e-12."""
    d = R.masked_inputs(1025, mask_kind)
    ref = R.masked64(d["rgb"], d["tgt"], d["depth"], d["prior"], d["mask"])
    c, z = T64(d["rgb"]).requires_grad_(True), T64(d["depth"]).requires_grad_(True)
    m = T64(d["mask"])
    il = O.masked_rgb_loss(c, T64(d["tgt"]), m, R.COEF)
    dl = O.masked_depth_loss(z, T64(d["prior"]), m, R.FAR)
    (il + dl).backward()
    close(ref["img"], il.item()); close(ref["dep"], dl.item())
    close(ref["d_rgb"], c.grad.numpy()); close(ref["d_depth"], z.grad.numpy())


def test_masked64_counts_g_scale_gate_and_odd_values():
    """What the oracle does not state: global counts divide instead of the local set sizes, g_scale multiplies the seeds and not the
    values, a mask value other than 0 / 1 puts its ray into neither set, and without an m == 0 ray the coef branch is absent."""
    d = R.masked_inputs(1025, "odd")
    a = (d["rgb"], d["tgt"], d["depth"], d["prior"], d["mask"])
    loc = R.masked64(*a)
    odd = (d["mask"] != 0) & (d["mask"] != 1)
    assert 50 < odd.sum() < 400 and loc["N1"] + loc["N0"] + odd.sum() == 1025
    assert not loc["d_rgb"][odd].any() and not loc["d_depth"][d["mask"] != 1].any() and loc["d_depth"][d["mask"] == 1].all()
    cnt = R.global_counts(d["mask"], 1025)
    glo = R.masked64(*a, counts=cnt, g_scale=0.125)
    s1 = d["mask"] == 1
    e = ((d["rgb"].astype(np.float64) - d["tgt"]) ** 2).sum(1)
    close(glo["img"], e[s1].sum() / (3 * float(cnt[0])) + R.COEF * e[d["mask"] == 0].sum() / (3 * float(cnt[1])))
    close(glo["d_rgb"][s1], 0.125 * loc["d_rgb"][s1] * loc["N1"] / float(cnt[0]))
    close(glo["dep"], loc["dep"] * loc["N1"] / float(cnt[0]))
    ones = R.masked_inputs(64, "ones")
    o = R.masked64(ones["rgb"], ones["tgt"], None, None, ones["mask"])
    close(o["img"], R.mse64(ones["rgb"], ones["tgt"])[0])
    assert o["N0"] == 0 and o["d_depth"] is None
    z = R.masked64(ones["rgb"], ones["tgt"], ones["depth"], ones["prior"], np.zeros(64, np.float32))
    assert np.isnan(z["img"]) and np.isnan(z["dep"]) and np.isfinite(z["d_rgb"]).all() and not z["d_depth"].any()


def test_mse_softlp_softmask_statements():
    x, y = R.mse_inputs(1025)
    xt = T64(x).requires_grad_(True)
    L = O.mse(xt, T64(y)); L.backward()
    v, s = R.mse64(x, y)
    close(v, L.item()); close(s, xt.grad.numpy())
    x, y = R.soft_inputs(1025)
    nz = x != y
    assert 50 < (~nz).sum() < 200
    for coef in R.SOFT_COEFS:
        L, g = R.softlp_aten(x, y, coef, torch.float64)
        v, s = R.softlp64(x, y, coef)
        close(v, L); close(s[nz], g[nz])
        assert not s[~nz].any() and np.isfinite(s).all()
        assert np.isnan(g[~nz]).all() == (coef < 1)               # autograd's inf * 0 at an exact zero: the statement takes the limit
    for t in R.SOFT_TEMPS:
        L, g, dt = R.softmask_aten(x, y, t, torch.float64)
        v, s, d = R.softmask64(x, y, t)
        close(v, L); close(s, g); close(d, dt, 1e-9)
        assert not s[~nz].any()


def test_statements_against_the_captured_values():
    """The reference's own numbers (fp32 captures): losses_mask.npz, altlosses.npz, patch.npz, to fp32 round-off of the capture."""
    g = golden("losses_mask")
    far, coef = float(g["far"]), float(g["coef"])
    for tag, m in (("mixed", g["mask"]), ("allone", np.ones_like(g["mask"]))):
        r = R.masked64(g["rgb"], g["target"], g["depth"], g["prior"], m, far, coef)
        close(r["img"], g[tag + ".l_rgb"], 1e-6); close(r["dep"], g[tag + ".l_depth"], 1e-6)
        close(r["d_rgb"], g[tag + ".d_rgb"], 1e-6); close(r["d_depth"], g[tag + ".d_depth"], 1e-6)
    g = golden("altlosses")
    for c in ("2.0", "1.0", "0.5"):
        for kind, x, y in (("rgb", g["x3"], g["y3"]), ("depth", g["x1"], g["y1"])):
            v, s = R.softlp64(x.reshape(-1), y.reshape(-1), float(c))
            want = g[f"{kind}.c{c}.d_x"].reshape(-1)
            ok = np.isfinite(want)
            close(v, g[f"{kind}.c{c}.loss"], 1e-6); close(s[ok], want[ok], 2e-6)
    g = golden("patch")
    for tag in ("a", "b"):
        L, d = R.patch_lines(g[f"term_{tag}_depth"], g[f"term_{tag}_mono"], 4, 256, torch.float64)
        want = g[f"term_{tag}_grad"]
        assert np.array_equal(np.isnan(d), np.isnan(want))
        close(L, g[f"term_{tag}_loss"], 1e-5)
        for p in range(4):
            sl = slice(256 * p, 256 * (p + 1))
            assert np.nanmax(np.abs(d[sl] - want[sl])) <= 1e-4 * np.nanmax(np.abs(want[sl])) + 1e-30


def test_adam_statements():
    """adam64 = oracle.adam_step in float64 (1e-12); adam32 = the same in float32 to a few ulp of lerp-vs-mul_add association; the
    scalars are cnerf_adam_step's: computed in double, cast once."""
    for clip, gs in ((0.0, 1.0), (R.f32(0.1), 0.125)):
        p, g, m, v = R.adam_inputs(5000, clip, gs)
        fin = np.isfinite(g) & (np.abs(g.astype(np.float64) * gs) < 1e18)
        p, g, m, v = p[fin], g[fin], m[fin], v[fin]
        for step in (1, 7, 200000):
            lr = R.adam_lr(step)
            (p2, m2, v2), _ = R.adam64(p, g, m, v, step, lr, clip, gs)
            pr, mr, vr = T64(p), T64(m), T64(v)
            O.adam_step(pr, T64(g) * gs, mr, vr, step, lr, clip=clip)
            close(m2, mr.numpy()); close(v2, vr.numpy()); close(p2, pr.numpy())
            p3, m3, v3 = R.adam32(p, g, m, v, step, lr, clip, gs)
            assert np.abs(v3 - v2).max() <= 4e-7 * np.abs(v2).max() and np.abs(p3 - p2).max() <= 4e-7 * np.abs(p2).max()
    s = R.adam_scalars32(7, 3e-4)
    assert s[0] == np.float32(0.1) and s[1] == np.float32(0.999) and s[2] == np.float32(1.0 - 0.999) and s[2] != np.float32(1) - s[1]
    assert s[3] == np.float32(3e-4 / (1 - 0.9 ** 7)) and s[4] == np.float32(np.sqrt(1 - 0.999 ** 7)) and s[5] == np.float32(1e-8)


def test_clamp_keeps_nan_as_torch_clamp_does():
    g = np.array([np.nan, np.inf, -np.inf, 0.1, -0.1, 0.05, -0.0, 3.0], np.float32)
    want = torch.from_numpy(g).clamp(-0.1, 0.1).numpy()
    got = R.clamp_keep_nan(g, np.float32(0.1))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[0]) and got[1] == np.float32(0.1) and got[2] == -np.float32(0.1)
    p, m, v = (np.ones(1, np.float32) for _ in range(3))
    for clip in (0.0, R.f32(0.1)):
        out = R.adam32(p, g[:1], m, v, 4, 5e-4, clip)
        assert all(np.isnan(o).all() for o in out)


# ------------------------------------------------------------------------------------------------ bounds not too tight
@pytest.mark.parametrize("B", [1, 65, 1025, 16385, 49153])
@pytest.mark.parametrize("mask_kind", ["mixed", "ones", "odd", None])
def test_masked_bounds_admit_three_other_association_orders(B, mask_kind):
    worst = 0.0
    for wd, wc, gs in R.masked_variants():
        kw = R.masked_case(B, mask_kind, wd, wc, gs)
        for order in R.MASKED_ORDERS:
            r = R.masked_ratio(R.masked32(order=order, **kw), kw)
            worst = max(worst, r)
            assert r <= 1.0, (order, wd, wc, gs, r)
    print(f"masked B={B} mask={mask_kind}: worst fp32 / bound = {worst:.3f}")


@pytest.mark.parametrize("n", [1, 1025, 16385, 65537])
def test_mse_bounds_admit_three_association_orders(n):
    x, y = R.mse_inputs(n)
    (v, s), (bv, bs) = R.mse64(x, y), R.mse_bounds(x, y)
    for order in R.MSE_ORDERS:
        gv, gs_ = R.mse32(x, y, order)
        r = max(R.ratio(gv, v, bv), R.ratio(gs_, s, bs))
        print(f"mse n={n} {order}: fp32 / bound = {r:.3f}")
        assert r <= 1.0, (order, r)


def test_adam_bounds_admit_the_fp32_restatement():
    """adam32 against adam64 per element, over every small case and the first large one: inside the derived bound wherever the fp32
    results are finite (g g overflows to inf in fp32 only)."""
    worst = 0.0
    for n, clip, gs, step in R.adam_cases():
        if n > R.ADAM_LARGE[0]:
            continue
        p, g, m, v = R.adam_inputs(n, R.f32(clip), gs)
        got = R.adam32(p, g, m, v, step, R.adam_lr(step), R.f32(clip), gs)
        ref, bnd = R.adam64(p, g, m, v, step, R.adam_lr(step), R.f32(clip), gs)
        fin = np.isfinite(got[0]) & np.isfinite(got[1]) & np.isfinite(got[2])
        assert fin.sum() >= n - 16
        for name, a, b, c in zip("pmv", got, ref, bnd):
            r = R.ratio(a[fin], b[fin], c[fin])
            worst = max(worst, r)
            assert r <= 1.0, (name, n, clip, gs, step, r)
    print(f"adam: worst fp32 restatement / bound = {worst:.3f}")


def test_soft_and_patch_yardsticks_are_small():
    """The 4 A + floor yardsticks on the GPU test's inputs: A (fp32 ATen against float64) is round-off, not conditioning."""
    for n in R.SOFT_SIZES:
        x, y = R.soft_inputs(n)
        for coef in R.SOFT_COEFS:
            ref, A, bnd = R.soft_yardstick("softlp", x, y, coef)
            assert bnd[0] <= 1e-5 * abs(ref[0]) + 1e-30 and bnd[1] <= 1e-5, (n, coef, A, bnd)
        for t in R.SOFT_TEMPS:
            ref, A, bnd = R.soft_yardstick("softmask", x, y, t)
            assert bnd[0] <= 1e-4 * abs(ref[0]) + 1e-30 and bnd[1] <= 1e-4, (n, t, A, bnd)
    for P, n in R.PATCH_SIZES:
        for fam in R.PATCH_FAMILIES:
            d, mo = R.patch_inputs(P, n, fam)
            L64, g64 = R.patch_lines(d, mo, P, n, torch.float64)
            L32, g32 = R.patch_lines(d, mo, P, n, torch.float32)
            assert np.array_equal(np.isnan(g64), np.isnan(g32))
            if n == 1:
                assert L64 == 0 and not g64.any()
            elif n > 2:
                assert abs(L32 - L64) <= 1e-6 * abs(L64) + 1e-30, (P, n, fam)


# ------------------------------------------------------------------------------------------------ bounds not loose
def test_every_mutant_misses_its_bound_by_4x():
    rows = R.mutant_ratios()
    least = {}
    for fam, mu, case, r in rows:
        if r < least.get((fam, mu), (np.inf, None))[0] or (fam, mu) not in least:
            least[(fam, mu)] = (r, case)
    for (fam, mu), (r, case) in sorted(least.items()):
        print(f"mutant {fam:9s} {mu:18s} least ratio {r:.3g} at {case}")
    want = {("masked", m) for m in R.MASKED_MUTANTS} | {("mse", m) for m in R.MSE_MUTANTS} | {("softmask", m) for m in R.SOFTMASK_MUTANTS}
    want |= {("adam", m) for m in R.ADAM_MUTANTS}
    assert set(least) == want
    overall = min(r for r, _ in least.values())
    print(f"least mutant ratio: {overall:.3g}")
    assert overall >= 4.0, least
