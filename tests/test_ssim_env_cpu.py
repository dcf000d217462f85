"""Default-run (no GPU) checks of tests/_ssim_env_ref.py, the float64 statements and bounds tests/test_gpu_ssim_envelope.py holds
csrc/ssim.hip to.  The cases are that file's own (shared data), so everything here runs on them:
  * the window restatement, and the truth with fp32 taps against _ssim_ref's float64 window;
  * the explicit backward (ssim.hpp's formula, level by level) equals float64 autograd of _ssim_ref;
  * honest fp32 arithmetic sits inside both bounds on EVERY case: the forward in the kernel's order of operations inside the forward
    bound, the fp32 ATen lines inside the forward bound with their own filter roundings, and the fp32 ATen autograd inside the
    elementwise gradient bound, whose C_GRAD is re-derived here from that same autograd;
  * every mutant of the statements misses the bound it belongs to on at least one case; the table printed shows by what factor, and
    which of them the suite's earlier rule (max-relative, 2 d32 + 1e-6) would have passed.
"""
import numpy as np
import pytest
import torch

import _ssim_env_ref as E
import _ssim_ref as R

torch.set_num_threads(4)

SSIM_CASES, MS_CASES = E.ssim_cases(), E.ms_cases()


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ window and truth
@pytest.mark.parametrize("win,sigma", [(1, 1.5), (3, 1.5), (7, 1.5), (11, 1.5), (31, 5.0), (7, 1.0), (31, 3.0)])
def test_taps32_against_the_reference_window(win, sigma):
    """cn_ssim_window's sequence in numpy float32.  Its exponentials are _ssim_ref.window(dtype=float32)'s bit for bit; its sum runs in
    index order where ATen's is vectorised, so the normalised taps are bit-equal where the two sums are (windows 1 and 3) and within
    2 win u elsewhere (either sum is within (win - 1) u of the exact one; 2 ulps at window 31): what the library filters with is NOT always the reference's fp32 window, which is why the truth takes the
    taps from here."""
    g = E.taps32(win, sigma)
    w = R.window(win, sigma, torch.float32).numpy()
    coords = torch.arange(win, dtype=torch.float32) - win // 2
    e = torch.exp(-(coords ** 2) / (2 * sigma ** 2)).numpy()
    s = np.float32(0)
    for t in e:
        s = np.float32(s + t)
    assert np.array_equal((e / s).view(np.uint32), g.view(np.uint32)), "the exponentials differ"
    assert (np.abs(g.astype(np.float64) - w) <= 2 * win * E.U * w).all(), _ulps(g, w)
    if win <= 3:
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert g.dtype == np.float32 and (g > 0).all() and abs(float(g.astype(np.float64).sum()) - 1) < 4 * E.U * win
    assert np.array_equal(R.window(win, sigma, torch.float64, taps=g).numpy(), g.astype(np.float64))


@pytest.mark.parametrize("c", [c for c in SSIM_CASES if c.fam in ("noise", "flat")][::4], ids=lambda c: c.name)
def test_truth_with_fp32_taps_equals_ssim_ref_within_the_taps_difference(c):
    """S with the library's taps against _ssim_ref's own float64 window: the first-order effect of the taps' difference,
    sum_k |dg_k| x |d S / d g_k| <= sum_k |dg_k| x (A-like magnitude); stated as the forward bound with the taps' largest relative
    difference (rel u, at most (win + 2) u by the summation bound) as the roundings of each filtered sum."""
    t = E.truth(c)
    taps64 = R.window(c.win, c.sigma).numpy()
    rel = float((np.abs(t.taps.astype(np.float64) - taps64) / taps64).max() / E.U)
    assert rel <= c.win + 2
    s, cs = R.maps(t.X.double(), t.Y.double(), data_range=c.dr, win_size=c.win, win_sigma=c.sigma, consts=(t.C1, t.C2))
    S, CS = s.flatten(2).mean(-1), cs.flatten(2).mean(-1)
    bS, bC = E.fwd_bounds(t.p, nf=max(1, int(np.ceil(rel))))
    assert ((S - t.S).abs() <= bS).all() and ((CS - t.cs).abs() <= bC).all(), ((S - t.S).abs().max(), bS.min())


# ------------------------------------------------------------------------------------------------ the explicit backward
@pytest.mark.parametrize("c", SSIM_CASES + MS_CASES, ids=lambda c: c.name)
def test_explicit_backward_is_float64_autograd(c):
    """ssim.hpp's formula (and cnerf_msssim_bwd's level walk) in float64 equals autograd of _ssim_ref to 1e-11 of A: the mutants
    below are mutants of a statement that is right."""
    t = E.truth(c)
    X, Y, seed = t.X.double(), t.Y.double(), t.seed.double()
    if hasattr(c, "levels"):
        gx, gy = E.ms_explicit(X, Y, t.taps, t.C1, t.C2, seed)
    else:
        gx, gy = E.level_grad(t.p, X, Y, seed, False)
    assert ((gx - t.gx).abs() <= 1e-11 * t.Ax + 1e-300).all() and ((gy - t.gy).abs() <= 1e-11 * t.Ay + 1e-300).all()
    assert (t.Ax >= t.gx.abs() * (1 - 1e-9)).all() and (t.Ay >= t.gy.abs() * (1 - 1e-9)).all()


# ------------------------------------------------------------------------------------------------ honest fp32 inside the bounds
def test_fp32_arithmetic_inside_both_bounds_on_every_case():
    """No case is left out.  Forward: the kernel-order fp32 lines inside the forward bound; the ATen fp32 lines inside the same
    propagation with their filter's roundings.  Backward: the ATen fp32 autograd inside C_GRAD u A elementwise, and C_GRAD is what its
    largest ratio derives."""
    worst = {"ssim": 0.0, "msssim": 0.0, "patch": 0.0}
    frac = {"kernel-order forward": 0.0, "ATen fp32 forward": 0.0}
    for c in SSIM_CASES:
        t = E.truth(c)
        kS, kC = E.kernel_order_lines(t.X, t.Y, t.taps, t.C1, t.C2)
        f = max(float(((kS - t.S).abs() / t.bS).max()), float(((kC - t.cs).abs() / t.bcs).max()))
        f32 = max(float(((t.S32 - t.S).abs() / t.bS32).max()), float(((t.cs32 - t.cs).abs() / t.bcs32).max()))
        r = max(E.grad_ratio(t.gx32, t.gx, t.Ax), E.grad_ratio(t.gy32, t.gy, t.Ay))
        assert f <= 1 and f32 <= 1 and r <= E.C_GRAD["ssim"], (c.name, f, f32, r)
        frac["kernel-order forward"], frac["ATen fp32 forward"] = max(frac["kernel-order forward"], f), max(frac["ATen fp32 forward"], f32)
        worst["ssim"] = max(worst["ssim"], r)
        if c.fam == "same":
            assert ((kS - 1).abs() <= t.bS).all() and ((t.S - 1).abs() <= 1e-12).all()
    for c in MS_CASES:
        t = E.truth(c)
        kv = E.kernel_order_ms_lines(t.X, t.Y, t.taps, t.C1, t.C2, c.levels)
        f, f32 = float(((kv - t.v).abs() / t.bv).max()), float(((t.v32 - t.v).abs() / t.bv32).max())
        r = max(E.grad_ratio(t.gx32, t.gx, t.Ax), E.grad_ratio(t.gy32, t.gy, t.Ay))
        assert f <= 1 and f32 <= 1 and r <= E.C_GRAD["msssim"], (c.name, f, f32, r)
        frac["kernel-order forward"], frac["ATen fp32 forward"] = max(frac["kernel-order forward"], f), max(frac["ATen fp32 forward"], f32)
        worst["msssim"] = max(worst["msssim"], r)
    for P in range(1, 17):
        for fam in E.PATCH_FAMILIES:
            t = E.patch_truth(P, fam)
            sh = (1, 1, -1, 3)
            r = E.grad_ratio(t.g32.reshape(sh), t.g.reshape(sh), t.A.reshape(sh))
            assert abs(t.v32 - t.v) <= t.bv32 and r <= E.C_GRAD["patch"], (P, fam, abs(t.v32 - t.v), t.bv32, r)
            worst["patch"] = max(worst["patch"], r)
    print(f"largest fraction of the forward bound: {frac}")
    print(f"largest |g32 - g64| / (u A) of the fp32 ATen autograd: {worst}; C_GRAD {E.C_GRAD}")
    for k, r in worst.items():
        # C_GRAD = c_from(REF_RATIO_MEASURED) exactly; the ratio measured now (ATen's summation order may differ between builds) still
        # leaves the 4 x margin and C_GRAD is no more than 4 x beyond what it derives
        assert E.c_from(E.REF_RATIO_MEASURED[k]) == E.C_GRAD[k] and 4 * r <= E.C_GRAD[k] <= 16 * r, (k, r, E.REF_RATIO_MEASURED[k])


def test_pool_bound_admits_fp32_pooling():
    for H in (1, 2, 3, 4, 5, 64, 65):
        for W in (1, 2, 3, 4, 5, 64, 65):
            X = torch.rand(2, 2, H, W, generator=torch.Generator().manual_seed(H * 100 + W)) * 2 - 1
            ref, b = E.pool64(X)
            assert ((R.pool(X).double() - ref).abs() <= b).all() and torch.equal(ref, R.pool(X.double()))


# ------------------------------------------------------------------------------------------------ mutants
def test_every_mutant_misses_its_bound_and_the_old_rule_table():
    rows = E.mutant_rows()
    summ = E.mutant_summary(rows)
    print("\nmutant                 worst miss: new bound   old rule   cases outside / run   of those the old rule passes / sees")
    for mu in E.MUTANTS:
        o = summ[mu]
        print(f"{mu:22s} {o['worst factor']:20.3g} {o['worst factor, old rule']:10.3g}   {o['cases outside']:6d} / {o['cases']:<6d} "
              f"{o['outside, passing the old rule']:18d} / {o['outside, seen by the old rule']}")
    inside = [mu for mu in E.MUTANTS if summ[mu]["cases outside"] == 0]
    assert not inside, f"mutants no case catches (a failure of the test design): {inside}"
    for mu in E.MUTANTS:
        assert summ[mu]["worst factor"] >= 4.0, (mu, summ[mu])
