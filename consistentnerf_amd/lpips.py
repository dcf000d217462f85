"""LPIPS with the `lpips` package's signatures (LPIPS(net='vgg'), version 0.1, eval mode), on the HIP kernels of csrc/lpips.hip.

The reference builds `lpips.LPIPS(net="vgg")` at import (V:40) and calls it in its training loss (V:1699-1728) and its metrics
(V:2055-2087); this module can stand in for the package:  `sys.modules['lpips'] = consistentnerf_amd.lpips`.  The statement is in
DESIGN.md §4e: the scaling layer, the 13 convolutions of VGG16 with five taps, per tap the channel-normalised squared difference under
the `lin` weights averaged over the map, the five summed.

Inputs: CUDA float32 [N, 3, H, W] in [-1, 1] (`normalize=True`: in [0, 1]), sides >= 16; anything else raises.  Differentiable in
both inputs through the HIP backward (the network itself is frozen: no weight gradients).  Not supported: other nets, `spatial=True`,
`lpips=False` (NotImplementedError).

Weights are NEVER fetched.  They come from `weights=` (a state dict or the path of one saved with torch.save) or from the file named
by the environment variable CNERF_LPIPS_WEIGHTS (so that V:40's bare call works).  Accepted layouts (KEY_TABLE): the package's own
state dict, or torchvision's VGG16 `features.N.*` together with the package's `lin*` entries.  The key names are written from memory
of the package and of torchvision; they could not be checked against either while this was written, so a file that does not load is
first of all a reason to compare its keys with KEY_TABLE.
"""
import os

import torch

from . import ops

__all__ = ["LPIPS", "KEY_TABLE", "load_state"]

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
_VGG_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)       # torchvision's vgg16().features index of the 13 convolutions
_SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)               # the package's net.slice{k} holding each


def _key_table():
    """our name -> (shape, the keys it may be stored under, in order of preference)"""
    t = {}
    for l, ((ci, co), idx, sl) in enumerate(zip(ops.LPIPS_CHANNELS, _VGG_IDX, _SLICE_OF)):
        for part, shape in (("weight", (co, ci, 3, 3)), ("bias", (co,))):
            t[f"conv{l}.{part}"] = (shape, (f"net.slice{sl}.{idx}.{part}", f"features.{idx}.{part}"))
    for k, l in enumerate(ops.LPIPS_TAPS):
        c = ops.LPIPS_CHANNELS[l][1]
        t[f"lin{k}"] = ((1, c, 1, 1), (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"))
    return t


KEY_TABLE = _key_table()
_SCALING_KEYS = {"shift": "scaling_layer.shift", "scale": "scaling_layer.scale"}


def load_state(weights):
    """A state dict (or the path of one) in either accepted layout -> {our name: float32 CPU tensor}, every entry of KEY_TABLE plus
    `shift` / `scale` (the package's constants when the file has no scaling layer).  A missing or mis-shaped key: ValueError."""
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(os.fspath(weights), map_location="cpu")
    if not isinstance(weights, dict):
        raise TypeError(f"LPIPS: weights must be a state dict or a path, got {type(weights).__name__}")
    out = {}
    for name, (shape, keys) in KEY_TABLE.items():
        key = next((k for k in keys if k in weights), None)
        if key is None:
            raise ValueError(f"LPIPS weights: no key for {name}: expected one of {', '.join(keys)}")
        t = torch.as_tensor(weights[key])
        if tuple(t.shape) != shape:
            raise ValueError(f"LPIPS weights: {key} has shape {tuple(t.shape)}, expected {shape}")
        out[name] = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
    for name, const in (("shift", SHIFT), ("scale", SCALE)):
        key = _SCALING_KEYS[name]
        if key in weights:
            t = torch.as_tensor(weights[key])
            if t.numel() != 3:
                raise ValueError(f"LPIPS weights: {key} has shape {tuple(t.shape)}, expected 3 values")
            out[name] = t.detach().to(device="cpu", dtype=torch.float32).reshape(3).contiguous()
        else:
            out[name] = torch.tensor(const, dtype=torch.float32)
    return out


class _LpipsFn(torch.autograd.Function):
    """(value [N], taps [5, N]) of one batched forward; the gradient w.r.t. in0 from the kept activations, w.r.t. in1 from a second
    kept forward with the roles swapped (d is symmetric in its inputs)."""

    @staticmethod
    def forward(ctx, X, Y, packed, keep):
        value, taps, ws, _ = ops.lpips_forward(X, Y, packed, keep=keep, want_taps=True)
        ctx.save_for_backward(X, Y)
        ctx.packed, ctx.ws = packed, ws
        ctx.mark_non_differentiable(taps)
        return value, taps

    @staticmethod
    def backward(ctx, g, _g_taps):
        X, Y = ctx.saved_tensors
        dX = dY = None
        g = g.contiguous()
        if ctx.needs_input_grad[0]:
            dX = ops.lpips_backward(ctx.packed, ctx.ws, g, X.shape)
        if ctx.needs_input_grad[1]:
            _, _, ws, _ = ops.lpips_forward(Y, X, ctx.packed, keep=True)
            dY = ops.lpips_backward(ctx.packed, ws, g, X.shape)
        return dX, dY, None, None


class LPIPS(torch.nn.Module):
    def __init__(self, pretrained=True, net='vgg', version='0.1', lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
                 use_dropout=True, model_path=None, eval_mode=True, verbose=True, weights=None):
        super().__init__()
        if net not in ('vgg', 'vgg16'):
            raise NotImplementedError(f"LPIPS: only net='vgg' is built (the reference's choice, V:40), got {net!r}")
        if str(version) != '0.1':
            raise NotImplementedError(f"LPIPS: only version '0.1' is built, got {version!r}")
        if spatial or not lpips or pnet_rand or pnet_tune:
            raise NotImplementedError("LPIPS: spatial=True, lpips=False, pnet_rand and pnet_tune are not built")
        src = weights if weights is not None else (model_path or os.environ.get("CNERF_LPIPS_WEIGHTS"))
        if src is None:
            raise RuntimeError("LPIPS: no weights.  They are never downloaded: pass weights= (a state dict or a path: the lpips package's "
                               "state dict, or torchvision VGG16 `features.*` plus the package's `lin*` entries), or name such a file in the "
                               "environment variable CNERF_LPIPS_WEIGHTS")
        for name, t in load_state(src).items():
            self.register_buffer(name.replace(".", "_"), t)
        self._packed = None
        self.eval()

    def _tensors(self):
        convs = [getattr(self, f"conv{l}_{p}") for l in range(13) for p in ("weight", "bias")]
        return convs, [getattr(self, f"lin{k}") for k in range(5)], self.shift, self.scale

    def _apply(self, fn, *a, **k):
        self._packed = None                       # the buffers move or change: pack again on the next call
        return super()._apply(fn, *a, **k)

    def packed(self, device):
        """The kernels' weight blob on `device` (packed once per device the module is used on)."""
        if self._packed is None or self._packed.device != device:
            convs, lins, shift, scale = self._tensors()
            mv = lambda t: t.detach().to(device)  # noqa: E731
            self._packed = ops.lpips_pack([mv(t) for t in convs], [mv(t) for t in lins], mv(shift), mv(scale))
        return self._packed

    @staticmethod
    def _check(in0, in1):
        if not (torch.is_tensor(in0) and torch.is_tensor(in1)):
            raise TypeError("LPIPS: in0 and in1 must be tensors")
        for t in (in0, in1):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise TypeError(f"LPIPS: takes CUDA float32 tensors (consistentnerf_amd has no CPU path), got {t.dtype} on {t.device}")
        if in0.dim() != 4 or in0.shape != in1.shape:
            raise ValueError(f"LPIPS: in0 and in1 must be [N, 3, H, W] tensors of one shape, got {tuple(in0.shape)} / {tuple(in1.shape)}")
        if in0.shape[1] != 3:
            raise ValueError(f"LPIPS: 3 channels expected, got {in0.shape[1]}")
        if min(in0.shape[2:]) < 16 or in0.shape[0] == 0:
            raise ValueError(f"LPIPS: needs at least one image with sides >= 16 (four 2x2 pools), got {tuple(in0.shape)}")

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        self._check(in0, in1)
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        keep = torch.is_grad_enabled() and (in0.requires_grad or in1.requires_grad)
        value, taps = _LpipsFn.apply(in0, in1, self.packed(in0.device), keep)
        value = value.reshape(-1, 1, 1, 1)
        if retPerLayer:
            return value, [t.reshape(-1, 1, 1, 1) for t in taps]
        return value
