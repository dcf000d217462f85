"""SSIM / MS-SSIM with pytorch-msssim 0.2.1's signatures (the version the reference pins), on the HIP kernels of csrc/ssim.hip.

The reference calls the library in its training loss (V:1701, V:1836) and in its metrics (alky/vis_utils.py img2ssim); this module
can stand in for it:  `sys.modules['pytorch_msssim'] = consistentnerf_amd.ssim`.  The statement is restated in DESIGN.md (§SSIM):
an 11-tap Gaussian window (sigma 1.5) filtering along H then W (a side shorter than the window is left unfiltered), single-pass
variances in fp32, per-channel means; MS-SSIM over five levels with 2x2 average pooling in between.

Inputs: CUDA float32 [N, C, H, W] tensors (no CPU path: anything else raises).  `ssim` is differentiable w.r.t. X and Y through the
HIP backward; `ms_ssim` is a metric (forward only).  Not supported: an explicit `win=` tensor, 5-D (volumetric) inputs.
"""
import torch

from . import ops

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM"]

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _check(X, Y, win, win_size):
    if win is not None:
        raise NotImplementedError("ssim: an explicit `win` tensor is not supported; pass win_size / win_sigma")
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError("ssim: X and Y must be tensors")
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}.")
    if X.dim() == 5:
        raise NotImplementedError("ssim: 5-D (volumetric) inputs are not supported")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors, but got {tuple(X.shape)}")
    if X.dtype != Y.dtype:
        raise ValueError("Input images should have the same dtype.")
    if int(win_size) % 2 != 1:
        raise ValueError("Window size should be odd.")
    if not 0 < int(win_size) <= 31:
        raise ValueError(f"ssim: win_size must be an odd number in 1..31, got {win_size}")
    if not (X.is_cuda and Y.is_cuda and X.dtype == torch.float32):
        raise TypeError(f"ssim: takes CUDA float32 tensors (consistentnerf_amd has no CPU path), got {X.dtype} on {X.device}")


def _consts(data_range, K):
    K1, K2 = K
    return (K1 * data_range) ** 2, (K2 * data_range) ** 2


class _SsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, Y, win_size, win_sigma, C1, C2):
        s, _ = ops.ssim_forward(X, Y, win_size, win_sigma, C1, C2, want_cs=False)
        ctx.save_for_backward(X, Y)
        ctx.cfg = (win_size, win_sigma, C1, C2)
        return s

    @staticmethod
    def backward(ctx, g):
        X, Y = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 6
        dX, dY = ops.ssim_backward(X, Y, *ctx.cfg, g.contiguous(), want_dY=ctx.needs_input_grad[1])
        return (dX if ctx.needs_input_grad[0] else None), dY, None, None, None, None


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: the mean SSIM per (image, channel) -> its mean (size_average) or the mean over channels, [N]."""
    _check(X, Y, win, win_size)
    C1, C2 = _consts(data_range, K)
    s = _SsimFn.apply(X, Y, int(win_size), float(win_sigma), float(C1), float(C2))
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: prod_l relu(cs_l) ** w_l over the first four levels times relu(ssim_5) ** w_5, the levels 2x2
    average-pooled (odd sides padded, the padding counted).  Needs min(H, W) > (win_size - 1) * 16.  Forward only."""
    _check(X, Y, win, win_size)
    if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad):
        raise NotImplementedError("ms_ssim: no backward (a metric here); call it under torch.no_grad() or on detached tensors")
    smaller_side = min(X.shape[-2:])
    if not smaller_side > (win_size - 1) * (2 ** 4):
        raise ValueError(f"Image size should be larger than {(win_size - 1) * (2 ** 4)} due to the 4 downsamplings in ms-ssim")
    w = X.new_tensor(MS_WEIGHTS if weights is None else weights)
    C1, C2 = _consts(data_range, K)
    mcs = []
    for i in range(w.shape[0]):
        s, cs = ops.ssim_forward(X, Y, int(win_size), float(win_sigma), float(C1), float(C2))
        if i < w.shape[0] - 1:
            mcs.append(torch.relu(cs))
            X, Y = ops.avg_pool2(X), ops.avg_pool2(Y)
    s = torch.relu(s)
    val = torch.prod(torch.stack(mcs + [s], dim=0) ** w.view(-1, 1, 1), dim=0)
    return val.mean() if size_average else val.mean(1)


class SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, K=(0.01, 0.03),
                 nonnegative_ssim=False):
        super().__init__()
        self.kw = dict(data_range=data_range, size_average=size_average, win_size=win_size, win_sigma=win_sigma, K=K,
                       nonnegative_ssim=nonnegative_ssim)

    def forward(self, X, Y):
        return ssim(X, Y, **self.kw)


class MS_SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None,
                 K=(0.01, 0.03)):
        super().__init__()
        self.kw = dict(data_range=data_range, size_average=size_average, win_size=win_size, win_sigma=win_sigma, weights=weights, K=K)

    def forward(self, X, Y):
        return ms_ssim(X, Y, **self.kw)
