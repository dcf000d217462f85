"""SSIM without a GPU: the float64 restatement of pytorch-msssim 0.2.1 (tests/_ssim_ref.py) pinned on closed forms, the analytic
backward the HIP kernels implement (csrc/ssim.hpp) checked against autograd of that restatement, and the Python argument checks of
consistentnerf_amd.ssim that run before any device work."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import _ssim_ref as R


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_window_is_symmetric_and_normalised():
    for ws, sg in ((11, 1.5), (7, 1.0), (31, 4.0), (1, 1.5)):
        g = R.window(ws, sg)
        assert g.numel() == ws and torch.allclose(g, g.flip(0), atol=0, rtol=0)
        assert abs(float(g.sum()) - 1.0) < 1e-15
    g = R.window()
    assert int(torch.argmax(g)) == 5
    assert torch.allclose(g[4] / g[5], torch.exp(torch.tensor(-1 / 4.5, dtype=torch.float64)), rtol=1e-14)


def test_identical_inputs_give_one():
    X = _rand(2, 3, 40, 50)
    assert abs(float(R.ssim(X, X, data_range=1)) - 1.0) < 1e-12
    assert torch.allclose(R.ssim(X, X, data_range=1, size_average=False), torch.ones(2, dtype=torch.float64), atol=1e-12)


@pytest.mark.parametrize("a,b,dr", [(0.2, 0.7, 1.0), (30.0, 200.0, 255.0), (0.5, 0.5, 1.0)])
def test_constant_images_closed_form(a, b, dr):
    X = torch.full((1, 2, 20, 24), a, dtype=torch.float64)
    Y = torch.full((1, 2, 20, 24), b, dtype=torch.float64)
    C1 = (0.01 * dr) ** 2
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    assert abs(float(R.ssim(X, Y, data_range=dr)) - want) < 1e-10


def test_patch_quirk_shape_and_unfiltered_small_images():
    # V:1701: a [1, 16, 16, 3] NHWC patch read as NCHW: H filtered to 6 rows, W = 3 < 11 left alone
    s, cs = R.maps(_rand(1, 16, 16, 3), _rand(1, 16, 16, 3, seed=1), data_range=1)
    assert s.shape == (1, 16, 6, 3) and cs.shape == (1, 16, 6, 3)
    # [1, 3, 8, 8]: both sides below the window -> per-pixel SSIM with zero variances: l(x, y) exactly
    X, Y = _rand(1, 3, 8, 8), _rand(1, 3, 8, 8, seed=2)
    s, cs = R.maps(X, Y, data_range=1)
    C1 = 0.01 ** 2
    assert s.shape == X.shape
    assert torch.allclose(s, (2 * X * Y + C1) / (X * X + Y * Y + C1), atol=1e-10)
    assert torch.allclose(cs, torch.ones_like(cs), atol=1e-9)


def test_ms_ssim_identical_and_size_limits():
    X = _rand(1, 1, 161, 170)
    assert abs(float(R.ms_ssim(X, X, data_range=1)) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        R.ms_ssim(_rand(1, 1, 160, 170), _rand(1, 1, 160, 170), data_range=1)
    float(R.ms_ssim(X, _rand(1, 1, 161, 170, seed=3), data_range=1))


def test_odd_side_pools_with_counted_padding():
    X = _rand(1, 2, 301, 400)
    P = R.pool(X)
    assert P.shape == (1, 2, 151, 200)
    # first / last rows: one real row + one padded zero row, divided by 4
    # first row: one padded zero row + one real row, still divided by 4; last row: rows 299 and 300
    assert torch.allclose(P[0, 0, 0, 0], (X[0, 0, 0, 0] + X[0, 0, 0, 1]) / 4)
    assert torch.allclose(P[0, 0, 150, 5], X[0, 0, 299:301, 10:12].sum() / 4)


def _analytic_grads(X, Y, g_nc, data_range=1.0, win_size=11, win_sigma=1.5):
    """csrc/ssim.hpp's backward in float64: the coefficient maps, then the transposed (zero-padded full) filter."""
    g = R.window(win_size, win_sigma)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = R.gfilter(X, g), R.gfilter(Y, g)
    exx, eyy, exy = R.gfilter(X * X, g), R.gfilter(Y * Y, g), R.gfilter(X * Y, g)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    B1, B2 = mx * mx + my * my + C1, sxx + syy + C2
    cs = (2 * sxy + C2) / B2
    lum = (2 * mx * my + C1) / B1
    S = lum * cs
    b, c = -S / B2, 2 * lum / B2
    ax = cs * 2 * (my - lum * mx) / B1 + 2 * mx * S / B2 - 2 * lum * my / B2
    ay = cs * 2 * (mx - lum * my) / B1 + 2 * my * S / B2 - 2 * lum * mx / B2
    scale = g_nc[:, :, None, None] / (S.shape[2] * S.shape[3])
    Cc, k = X.shape[1], g.numel()

    def ft(a):
        a = a * scale
        if X.shape[3] >= k:
            a = F.conv_transpose2d(a, g.view(1, 1, 1, k).repeat(Cc, 1, 1, 1), groups=Cc)
        if X.shape[2] >= k:
            a = F.conv_transpose2d(a, g.view(1, 1, k, 1).repeat(Cc, 1, 1, 1), groups=Cc)
        return a
    fb, fc = ft(b), ft(c)
    return ft(ax) + 2 * X * fb + Y * fc, ft(ay) + 2 * Y * fb + X * fc


@pytest.mark.parametrize("shape", [(2, 3, 30, 41), (1, 16, 16, 3), (1, 3, 8, 8), (1, 2, 9, 20)])
def test_analytic_backward_equals_autograd(shape):
    X, Y = _rand(*shape).requires_grad_(), _rand(*shape, seed=5).requires_grad_()
    g_nc = _rand(shape[0], shape[1], seed=6)
    s, _ = R.per_channel(X, Y, data_range=1)
    gx, gy = torch.autograd.grad((s * g_nc).sum(), (X, Y))
    ax, ay = _analytic_grads(X.detach(), Y.detach(), g_nc)
    assert torch.allclose(ax, gx, rtol=1e-9, atol=1e-13) and torch.allclose(ay, gy, rtol=1e-9, atol=1e-13)


def test_patch_level_is_the_mean_of_the_quirk_maps():
    rgb, tgt = _rand(1024 + 100, 3), _rand(1024 + 100, 3, seed=8)
    v = R.patch_level(rgb, tgt, 4)
    want = sum(float(R.maps(rgb[p * 256:(p + 1) * 256].reshape(1, 16, 16, 3), tgt[p * 256:(p + 1) * 256].reshape(1, 16, 16, 3),
                            data_range=1)[0].mean()) for p in range(4)) / 4
    assert abs(float(v) - want) < 1e-12


def test_product_argument_checks_without_a_gpu():
    from consistentnerf_amd import ssim as S
    x = torch.rand(1, 3, 20, 20)
    with pytest.raises(ValueError):
        S.ssim(x, torch.rand(1, 3, 20, 21))
    with pytest.raises(NotImplementedError):
        S.ssim(torch.rand(1, 3, 12, 12, 12), torch.rand(1, 3, 12, 12, 12))
    with pytest.raises(ValueError):
        S.ssim(x, x, win_size=10)
    with pytest.raises(NotImplementedError):
        S.ssim(x, x, win=R.window(11).float())
    with pytest.raises(ValueError):
        S.ms_ssim(x, x, win_size=4)
    with pytest.raises(TypeError):          # CPU tensors: no CPU path
        S.ssim(x, x)
    with pytest.raises(TypeError):
        S.ms_ssim(x, x)


def test_signatures_follow_pytorch_msssim():
    from consistentnerf_amd import ssim as S
    assert list(inspect.signature(S.ssim).parameters) == ["X", "Y", "data_range", "size_average", "win_size", "win_sigma", "win", "K",
                                                          "nonnegative_ssim"]
    assert list(inspect.signature(S.ms_ssim).parameters) == ["X", "Y", "data_range", "size_average", "win_size", "win_sigma", "win",
                                                             "weights", "K"]
    p = inspect.signature(S.ssim).parameters
    assert p["data_range"].default == 255 and p["win_size"].default == 11 and p["win_sigma"].default == 1.5
    assert p["K"].default == (0.01, 0.03) and p["size_average"].default is True


def test_render_loss_rejects_ssim_on_the_a15_route_and_odd_patches():
    from consistentnerf_amd import run_nerf_view as V
    t = torch.rand(512, 3)
    with pytest.raises(ValueError):
        V.render_loss(8, 8, None, t, mask=torch.ones(512), rays=None, ssim_w=0.005, _ss_coins=(1, 1, 1, 1))
    with pytest.raises(ValueError):
        V.render_loss(8, 8, None, t, rays=None, ssim_w=0.005, patch_size=8)
    with pytest.raises(ValueError):
        V.patch_ssim(t, t, 2, 8)
