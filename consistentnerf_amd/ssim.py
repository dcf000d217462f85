"""SSIM / MS-SSIM with pytorch-msssim 0.2.1's signatures (the version the reference pins), on the HIP kernels of csrc/ssim.hip.

The reference calls the library in its training loss (V:1701, V:1836) and in its metrics (alky/vis_utils.py img2ssim); this module
can stand in for it:  `sys.modules['pytorch_msssim'] = consistentnerf_amd.ssim`.  The statement is restated in DESIGN.md (§SSIM):
an 11-tap Gaussian window (sigma 1.5) filtering along H then W (a side shorter than the window is left unfiltered), single-pass
variances in fp32, per-channel means; MS-SSIM over five levels with 2x2 average pooling in between.

Inputs: CUDA float32 [N, C, H, W] tensors (no CPU path: anything else raises).  `ssim` and `ms_ssim` are differentiable w.r.t. X and
Y through the HIP backward, so `loss = 1 - ms_ssim(x, y)` trains: MS-SSIM's per-level means come from one C call and go back through
one (two launches per level, the pooling backward inside the transposed filter's); the product over the levels, its relu and powers
are ATen lines on levels x N x C numbers, so a plane with a level at cs <= 0 gets the gradient 0 exactly, as in the package.
Not supported: an explicit `win=` tensor, 5-D (volumetric) inputs.
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


class _MsSsimFn(torch.autograd.Function):
    """(X, Y) -> v [levels, N, C]: the per-channel mean of cs at every level below the last, of SSIM at the last (one C call);
    the backward walks the levels back in 2 * levels launches.  X, Y and the pooled levels are kept only when a gradient can be
    asked for."""

    @staticmethod
    def forward(ctx, X, Y, win_size, win_sigma, C1, C2, levels):
        v, pyr = ops.msssim_forward(X, Y, win_size, win_sigma, C1, C2, levels)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(X, Y, pyr)
            ctx.cfg = (win_size, win_sigma, C1, C2)
        return v

    @staticmethod
    def backward(ctx, g):
        X, Y, pyr = ctx.saved_tensors
        dX, dY = ops.msssim_backward(X, Y, *ctx.cfg, pyr, g.contiguous(), want_dY=ctx.needs_input_grad[1])
        return (dX if ctx.needs_input_grad[0] else None), dY, None, None, None, None, None


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: prod_l relu(cs_l) ** w_l over the first four levels times relu(ssim_5) ** w_5, the levels 2x2
    average-pooled (odd sides padded, the padding counted).  Needs min(H, W) > (win_size - 1) * 16.  Differentiable w.r.t. X and
    Y; a plane with a level at cs_l <= 0 (ssim_5 <= 0) has the value 0 and the gradient 0."""
    _check(X, Y, win, win_size)
    smaller_side = min(X.shape[-2:])
    if not smaller_side > (win_size - 1) * (2 ** 4):
        raise ValueError(f"Image size should be larger than {(win_size - 1) * (2 ** 4)} due to the 4 downsamplings in ms-ssim")
    w = X.new_tensor(MS_WEIGHTS if weights is None else weights)
    C1, C2 = _consts(data_range, K)
    v = _MsSsimFn.apply(X, Y, int(win_size), float(win_sigma), float(C1), float(C2), int(w.shape[0]))
    val = torch.prod(torch.relu(v) ** w.view(-1, 1, 1), dim=0)
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
