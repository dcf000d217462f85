"""The SSIM / MS-SSIM statement of pytorch-msssim 0.2.1 (the version the reference pins), restated on ATen in any dtype: the
checker of tests/test_ssim_cpu.py and tests/test_gpu_ssim.py (float64 = the truth; float32 = the reference's own arithmetic).
The product never imports it."""
import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(win_size=11, win_sigma=1.5, dtype=torch.float64, taps=None):
    """taps (optional): the window as given numbers (the library's fp32 taps, say), cast to dtype instead of being computed in it."""
    if taps is not None:
        return torch.as_tensor(taps).to(dtype)
    coords = torch.arange(win_size, dtype=dtype) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    return g / g.sum()


def gfilter(x, g):
    """Valid correlation along H, then W; a side shorter than the window is skipped."""
    C, k = x.shape[1], g.numel()
    g = g.to(device=x.device, dtype=x.dtype)
    if x.shape[2] >= k:
        x = F.conv2d(x, g.view(1, 1, k, 1).repeat(C, 1, 1, 1), groups=C)
    if x.shape[3] >= k:
        x = F.conv2d(x, g.view(1, 1, 1, k).repeat(C, 1, 1, 1), groups=C)
    return x


def maps(X, Y, data_range=255, win_size=11, win_sigma=1.5, K=(0.01, 0.03), taps=None, consts=None):
    """-> (ssim_map, cs_map) with single-pass variances.  taps: see window(); consts (optional) = (C1, C2) as given numbers."""
    g = window(win_size, win_sigma, X.dtype, taps)
    C1, C2 = ((K[0] * data_range) ** 2, (K[1] * data_range) ** 2) if consts is None else consts
    mu1, mu2 = gfilter(X, g), gfilter(Y, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = gfilter(X * X, g) - mu1_sq
    s22 = gfilter(Y * Y, g) - mu2_sq
    s12 = gfilter(X * Y, g) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map, cs_map


def per_channel(X, Y, **kw):
    s, cs = maps(X, Y, **kw)
    return torch.flatten(s, 2).mean(-1), torch.flatten(cs, 2).mean(-1)


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    s, _ = per_channel(X, Y, data_range=data_range, win_size=win_size, win_sigma=win_sigma, K=K)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def pool(X):
    return F.avg_pool2d(X, kernel_size=2, padding=[s % 2 for s in X.shape[2:]])


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    if not min(X.shape[-2:]) > (win_size - 1) * 16:
        raise ValueError("image too small for 4 downsamplings")
    w = X.new_tensor(MS_WEIGHTS if weights is None else weights)
    mcs = []
    for i in range(w.shape[0]):
        s, cs = per_channel(X, Y, data_range=data_range, win_size=win_size, win_sigma=win_sigma, K=K)
        if i < w.shape[0] - 1:
            mcs.append(torch.relu(cs))
            X, Y = pool(X), pool(Y)
    val = torch.prod(torch.stack(mcs + [torch.relu(s)], dim=0) ** w.view(-1, 1, 1), dim=0)
    return val.mean() if size_average else val.mean(1)


def patch_level(rgb, target, P=4):
    """V:1696-1720: sum_p ssim(rgb_p.reshape(1, 16, 16, 3), target_p.reshape(1, 16, 16, 3), data_range=1, size_average=False) / 4."""
    tot = 0.0
    for p in range(P):
        a = rgb[p * 256:(p + 1) * 256].reshape(1, 16, 16, 3)
        b = target[p * 256:(p + 1) * 256].reshape(1, 16, 16, 3)
        tot = tot + ssim(a, b, data_range=1, size_average=False)
    return (tot / 4)[0]


def img2ssim(x, y, mask=None):
    """alky/vis_utils.py:44-53 on this restatement (x, y [N, H, W, 3] tensors)."""
    if mask is not None:
        x, y = mask.unsqueeze(-1) * x, mask.unsqueeze(-1) * y
    x, y = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    return ssim(x, y, data_range=1), ms_ssim(x, y, data_range=1)
