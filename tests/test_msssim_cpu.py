"""MS-SSIM's backward without a GPU: the level walk the HIP kernels implement (csrc/ssim.hip: the cs coefficients of the levels
below the last, the SSIM coefficients of the last, the transposed filter, the pooled-back quarter) written in float64 and checked
against autograd of the restatement in tests/_ssim_ref.py; and the four C entry points declared, bound and exported."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _ssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, win_size, weights): odd sides at every level on both axes; a last level of 1 x 1 map at the default window; six levels
# ending at 2 x 2 where both filters are skipped; three levels; one level (the SSIM seed alone)
CASES = [((2, 2, 33, 50), 3, None), ((1, 3, 161, 175), 11, None), ((1, 1, 33, 50), 3, (0.05, 0.2, 0.3, 0.2, 0.15, 0.1)),
         ((1, 2, 33, 34), 3, (0.2, 0.5, 0.3)), ((2, 1, 33, 36), 3, (1.0,))]


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _level_grads(X, Y, g_nc, on_cs, nX, nY, win_size, win_sigma=1.5, data_range=1.0):
    """One level: the coefficient maps of a seed g_nc on the mean of cs (on_cs) or of S, the transposed (zero-padded full) filter,
    and, last in the sum, a quarter of the next level's gradient at ((i + H % 2) // 2, (j + W % 2) // 2)."""
    g = R.window(win_size, win_sigma)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = R.gfilter(X, g), R.gfilter(Y, g)
    sxx, syy, sxy = R.gfilter(X * X, g) - mx * mx, R.gfilter(Y * Y, g) - my * my, R.gfilter(X * Y, g) - mx * my
    B1, B2 = mx * mx + my * my + C1, sxx + syy + C2
    cs = (2 * sxy + C2) / B2
    if on_cs:
        b, c = -cs / B2, 2 / B2
        ax, ay = 2 * (mx * cs - my) / B2, 2 * (my * cs - mx) / B2
    else:
        lum = (2 * mx * my + C1) / B1
        S = lum * cs
        b, c = -S / B2, 2 * lum / B2
        ax = cs * 2 * (my - lum * mx) / B1 + 2 * mx * S / B2 - 2 * lum * my / B2
        ay = cs * 2 * (mx - lum * my) / B1 + 2 * my * S / B2 - 2 * lum * mx / B2
    scale = g_nc[:, :, None, None] / (cs.shape[2] * cs.shape[3])
    Cc, k, (H, W) = X.shape[1], g.numel(), X.shape[2:]

    def ft(a):
        a = a * scale
        if W >= k:
            a = F.conv_transpose2d(a, g.view(1, 1, 1, k).repeat(Cc, 1, 1, 1), groups=Cc)
        if H >= k:
            a = F.conv_transpose2d(a, g.view(1, 1, k, 1).repeat(Cc, 1, 1, 1), groups=Cc)
        return a
    fb, fc = ft(b), ft(c)
    dX, dY = ft(ax) + 2 * X * fb + Y * fc, ft(ay) + 2 * Y * fb + X * fc
    if nX is not None:
        i = (torch.arange(H) + H % 2) // 2
        j = (torch.arange(W) + W % 2) // 2
        dX = dX + 0.25 * nX[:, :, i][:, :, :, j]
        dY = dY + 0.25 * nY[:, :, i][:, :, :, j]
    return dX, dY


def _walk(X, Y, g_v, win_size):
    """The gradient of sum(g_v * v), v [L, N, C] the per-plane means (cs below the last level, SSIM at the last)."""
    L = g_v.shape[0]
    xs, ys = [X], [Y]
    for _ in range(L - 1):
        xs.append(R.pool(xs[-1]))
        ys.append(R.pool(ys[-1]))
    dX = dY = None
    for l in range(L - 1, -1, -1):
        dX, dY = _level_grads(xs[l], ys[l], g_v[l], l < L - 1, dX, dY, win_size)
    return dX, dY


def _v(X, Y, L, win_size):
    v = []
    for l in range(L):
        s, cs = R.per_channel(X, Y, data_range=1, win_size=win_size)
        v.append(s if l == L - 1 else cs)
        if l < L - 1:
            X, Y = R.pool(X), R.pool(Y)
    return torch.stack(v, 0)


@pytest.mark.parametrize("shape,win_size,weights", CASES)
def test_level_walk_equals_autograd_of_ms_ssim(shape, win_size, weights):
    X, Y = _rand(*shape, seed=1), _rand(*shape, seed=2)
    Y = (0.7 * X + 0.3 * Y)                        # correlated, so every level's cs is positive and the product is live
    L = 5 if weights is None else len(weights)
    # the seeds on v: autograd through the product, relu and powers, which the product leaves to ATen
    v = _v(X, Y, L, win_size).requires_grad_()
    w = X.new_tensor(R.MS_WEIGHTS if weights is None else weights)
    up = _rand(shape[0], seed=3)
    val = torch.prod(torch.relu(v) ** w.view(-1, 1, 1), dim=0).mean(1)
    g_v, = torch.autograd.grad((val * up).sum(), (v,))
    assert float(v.detach().min()) > 0
    ax, ay = _walk(X, Y, g_v, win_size)
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    ref = R.ms_ssim(x, y, data_range=1, size_average=False, win_size=win_size, weights=weights)
    assert torch.allclose(ref, val.detach(), rtol=1e-13, atol=0)
    gx, gy = torch.autograd.grad((ref * up).sum(), (x, y))
    for a, r in ((ax, gx), (ay, gy)):
        d = (a - r).abs().max().item() / r.abs().max().item()
        assert d <= 1e-12, d


def test_pooled_back_quarter_is_avg_pool_backward():
    for H, W in ((33, 50), (17, 25), (2, 2), (1, 7)):
        x = _rand(1, 2, H, W).requires_grad_()
        up = _rand(*R.pool(x).shape, seed=4)
        g, = torch.autograd.grad((R.pool(x) * up).sum(), (x,))
        i, j = (torch.arange(H) + H % 2) // 2, (torch.arange(W) + W % 2) // 2
        assert torch.equal(g, 0.25 * up[:, :, i][:, :, :, j])


def test_the_four_entry_points_are_declared_bound_and_exported():
    from consistentnerf_amd import _lib, build
    names = {"cnerf_msssim_ws_floats", "cnerf_msssim_fwd", "cnerf_msssim_bwd_ws_floats", "cnerf_msssim_bwd"}
    hdr = open(os.path.join(ROOT, "include", "cnerf.h")).read()
    assert names <= set(re.findall(r"\b(cnerf_[a-z0-9_]+)\s*\(", hdr))
    assert "#define CNERF_ABI_VERSION 6" in hdr
    assert names <= set(_lib.SIGNATURES)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r" T (cnerf_[a-z0-9_]+)", out))
    lib = _lib.load()
    # sizes: 5 levels of 2 x 3 x 161 x 175 -> sides 161, 81, 41, 21, 11 / 175, 88, 44, 22, 11; the coefficient maps of level 1
    # (151 x 165 outputs) are the largest, the coarser levels' gradients of X and of Y come on top
    half = 6 * (81 * 88 + 41 * 44 + 21 * 22 + 11 * 11)
    assert lib.cnerf_msssim_bwd_ws_floats(2, 3, 161, 175, 11, 5) == 4 * 6 * 151 * 165 + 2 * half
    assert lib.cnerf_msssim_ws_floats(2, 3, 161, 175, 11, 5) == lib.cnerf_ssim_ws_floats(2, 3, 161, 175, 11)
    # a level whose map is larger than the level before it (11 -> 1 output row at win 11, then 6 rows unfiltered)
    assert lib.cnerf_msssim_bwd_ws_floats(1, 1, 11, 11, 11, 2) == 4 * 36 + 2 * 36
    for bad in ((0, 3, 161, 175, 11, 5), (2, 3, 161, 175, 11, 0), (2, 3, 161, 175, 11, 25), (2, 3, 161, 175, 10, 5)):
        assert lib.cnerf_msssim_ws_floats(*bad) == 0 and lib.cnerf_msssim_bwd_ws_floats(*bad) == 0


def test_ms_ssim_keeps_its_argument_checks_when_a_gradient_is_asked_for():
    from consistentnerf_amd import ssim as S
    x = torch.rand(1, 3, 20, 20, requires_grad=True)
    with pytest.raises(TypeError):              # CPU tensors: no CPU path, with or without a gradient asked for
        S.ms_ssim(x, x)
    with pytest.raises(NotImplementedError):
        S.ms_ssim(x, x, win=R.window(11).float())
    with pytest.raises(NotImplementedError):
        S.ms_ssim(torch.rand(1, 3, 12, 12, 12, requires_grad=True), torch.rand(1, 3, 12, 12, 12))
