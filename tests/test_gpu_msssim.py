"""GPU tests of MS-SSIM's backward (csrc/ssim.hip: cnerf_msssim_fwd / cnerf_msssim_bwd; consistentnerf_amd/ssim.py ms_ssim, MS_SSIM)
against float64 autograd of the restatement of pytorch-msssim 0.2.1 in tests/_ssim_ref.py, and of the forward's unchanged bits."""
import pytest
import torch

import _ssim_ref as R

pytestmark = pytest.mark.gpu

# (shape, win_size, weights): tests/test_msssim_cpu.py's cases
CASES = [((2, 2, 33, 50), 3, None), ((1, 3, 161, 175), 11, None), ((1, 1, 33, 50), 3, (0.05, 0.2, 0.3, 0.2, 0.15, 0.1)),
         ((1, 2, 33, 34), 3, (0.2, 0.5, 0.3)), ((2, 1, 33, 36), 3, (1.0,))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _pair(shape, seed, dev, noise=0.15):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(*shape, generator=g)
    Y = (X + noise * torch.randn(*shape, generator=g)).clamp(0, 1)
    return X.to(dev), Y.to(dev)


def _grads(fn, X, Y, g_out, dt=None, **kw):
    x = (X if dt is None else X.to(dt)).clone().requires_grad_()
    y = (Y if dt is None else Y.to(dt)).clone().requires_grad_()
    v = fn(x, y, data_range=1, **kw)
    gx, gy = torch.autograd.grad((v * g_out.to(v.dtype)).sum(), (x, y))
    return gx.double(), gy.double()


def _assert_bound(k, r, f, what):
    """d = the kernel's distance from float64 relative to max|ref64|, d32 = the restatement's own in fp32, same run."""
    scale = r.abs().max().item()
    d, d32 = (k - r).abs().max().item() / scale, (f - r).abs().max().item() / scale
    print(f"msssim {what}: d={d:.3e} d32={d32:.3e}")
    assert d <= 2 * d32 + 1e-6 and d <= 1e-3, (what, d, d32)


@pytest.mark.parametrize("size_average", [True, False])
@pytest.mark.parametrize("shape,win_size,weights", CASES)
def test_ms_ssim_gradients(dev, shape, win_size, weights, size_average):
    from consistentnerf_amd import ssim as S
    X, Y = _pair(shape, 5, dev)
    g_out = torch.rand(shape[0], generator=torch.Generator().manual_seed(9)).to(dev)
    g_out = g_out.sum() if size_average else g_out
    kw = dict(size_average=size_average, win_size=win_size, weights=weights)
    (kx, ky), (rx, ry), (fx, fy) = (_grads(S.ms_ssim, X, Y, g_out, **kw), _grads(R.ms_ssim, X, Y, g_out, torch.float64, **kw),
                                    _grads(R.ms_ssim, X, Y, g_out, torch.float32, **kw))
    _assert_bound(kx, rx, fx, f"dX {shape} sa={size_average}")
    _assert_bound(ky, ry, fy, f"dY {shape} sa={size_average}")


def test_backward_is_deterministic_and_dx_alone_is_the_same_dx(dev):
    from consistentnerf_amd import ssim as S
    X, Y = _pair((2, 2, 33, 50), 6, dev)
    g = torch.ones((), device=dev)
    a, b = _grads(S.ms_ssim, X, Y, g, win_size=3), _grads(S.ms_ssim, X, Y, g, win_size=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0].abs().max()) > 0
    x = X.clone().requires_grad_()
    gx1, = torch.autograd.grad(S.ms_ssim(x, Y, data_range=1, win_size=3), (x,))
    assert torch.equal(gx1.double(), a[0])
    y = Y.clone().requires_grad_()
    gy1, = torch.autograd.grad(S.ms_ssim(X, y, data_range=1, win_size=3), (y,))
    assert torch.equal(gy1.double(), a[1])


def test_gated_plane_gets_an_exactly_zero_gradient(dev):
    """Y = 1 - X on plane 0: cs of levels 1-3 is about -0.99 / -0.86 / -0.48 there, relu gates the plane's product to 0."""
    from consistentnerf_amd import ssim as S
    X, Y = _pair((1, 2, 33, 50), 7, dev)
    Y[:, 0] = 1 - X[:, 0]
    g = torch.ones((), device=dev)
    k, r, f = (_grads(S.ms_ssim, X, Y, g, win_size=3), _grads(R.ms_ssim, X, Y, g, torch.float64, win_size=3),
               _grads(R.ms_ssim, X, Y, g, torch.float32, win_size=3))
    for i, n in enumerate(("dX", "dY")):
        assert bool(torch.isfinite(k[i]).all())
        assert float(k[i][:, 0].abs().max()) == 0.0 and float(r[i][:, 0].abs().max()) == 0.0
        _assert_bound(k[i][:, 1], r[i][:, 1], f[i][:, 1], f"{n} plane 1 beside a gated plane")


def _todays_loop(X, Y, data_range=1, size_average=True):
    """ms_ssim as it was before the one-call forward: ops.ssim_forward / ops.avg_pool2 level by level."""
    from consistentnerf_amd import ops, ssim as S
    w = X.new_tensor(S.MS_WEIGHTS)
    C1, C2 = S._consts(data_range, (0.01, 0.03))
    mcs = []
    for i in range(w.shape[0]):
        s, cs = ops.ssim_forward(X, Y, 11, 1.5, float(C1), float(C2))
        if i < w.shape[0] - 1:
            mcs.append(torch.relu(cs))
            X, Y = ops.avg_pool2(X), ops.avg_pool2(Y)
    val = torch.prod(torch.stack(mcs + [torch.relu(s)], dim=0) ** w.view(-1, 1, 1), dim=0)
    return val.mean() if size_average else val.mean(1)


@pytest.mark.parametrize("shape", [(2, 3, 301, 401), (1, 3, 161, 175)])
def test_forward_bits_unchanged(dev, shape):
    from consistentnerf_amd import ssim as S
    X, Y = _pair(shape, 8, dev)
    for sa in (True, False):
        want = _todays_loop(X, Y, size_average=sa)
        assert torch.equal(S.ms_ssim(X, Y, data_range=1, size_average=sa), want)
        with torch.no_grad():
            assert torch.equal(S.ms_ssim(X, Y, data_range=1, size_average=sa), want)
        x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
        got = S.ms_ssim(x, y, data_range=1, size_average=sa)
        assert got.requires_grad and torch.equal(got.detach(), want)
        with torch.no_grad():
            assert torch.equal(S.ms_ssim(x, y, data_range=1, size_average=sa), want)


def test_module_as_a_loss_and_img2ssim(dev):
    from consistentnerf_amd import io_formats as F, ssim as S
    X, Y = _pair((2, 3, 161, 175), 10, dev)
    x = X.clone().requires_grad_()
    m = S.MS_SSIM(data_range=1)
    loss = 1 - m(x, Y)
    loss.backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    r = X.double().requires_grad_()
    (1 - R.ms_ssim(r, Y.double(), data_range=1)).backward()
    assert (x.grad.double() - r.grad).abs().max().item() <= 1e-3 * r.grad.abs().max().item()
    # the metric: numpy images [N, H, W, 3] in, the same bits as the level-by-level loop
    xi, yi = X.permute(0, 2, 3, 1).contiguous(), Y.permute(0, 2, 3, 1).contiguous()
    s, ms = F.img2ssim(xi.cpu().numpy(), yi.cpu().numpy())
    assert torch.equal(ms, _todays_loop(X, Y)) and torch.equal(s, S.ssim(X, Y, data_range=1))
    assert not ms.requires_grad
