"""Tensor-level wrappers over the C ABI (include/cnerf.h).  Device memory, streams and allocation are
PyTorch-ROCm plumbing; every computation here is a HIP kernel of libcnerf_hip.so.  No fallbacks."""
import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import Closs, ClossTail, CnerfError, LossForm, Net, PixelBatch, Ptrs, RayGen, RenderCfg, RenderGrads, RenderOut, Rng, SsWarp

Tensor = torch.Tensor


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-kernel timing with HIP events recorded on the stream the kernels are launched on
# (bench.py's live roofline measurement).  PROFILE = None disables it (zero overhead).
PROFILE = None


class _timed:
    def __init__(self, name, units):
        self.name, self.units = name, units

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e1.record(torch.cuda.current_stream())
            PROFILE.append((self.name, self.units, self.e0, self.e1))
        return False


def _p(t: Optional[Tensor]):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _addr(t: Optional[Tensor]) -> Optional[int]:
    """Address or None: a pointer field of a ctypes struct."""
    return None if t is None else t.data_ptr()


def _chk(t: Optional[Tensor], name: str, dtype=torch.float32) -> Optional[Tensor]:
    if t is None:
        return None
    if not t.is_cuda:
        raise CnerfError(f"{name} must live on the GPU: consistentnerf_amd has no CPU path (got {t.device})")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


@dataclass(frozen=True)
class NetSpec:
    """Architecture of one MLP (mirror of struct cnerf_net)."""
    D: int = 8
    W: int = 256
    multires: int = 10
    multires_views: int = 4
    use_viewdirs: bool = True
    output_ch: int = 4
    skip: int = 4

    def c(self) -> Net:
        return Net(self.D, self.W, self.multires, self.multires_views, int(self.use_viewdirs), self.output_ch,
                   self.skip)

    @property
    def raw_ch(self) -> int:
        return 4 if self.use_viewdirs else self.output_ch

    def num_tensors(self) -> int:
        return _lib.load().cnerf_num_tensors(C.byref(self.c()))

    def tensor_shapes(self):
        lib, net, out = _lib.load(), self.c(), []
        r, c = C.c_int64(), C.c_int64()
        for i in range(self.num_tensors()):
            _lib.check(lib.cnerf_tensor_shape(C.byref(net), i, C.byref(r), C.byref(c)), "cnerf_tensor_shape")
            out.append((r.value,) if i & 1 else (r.value, c.value))
        return out


def _ptrs(tensors: Sequence[Optional[Tensor]]) -> Ptrs:
    p = Ptrs()
    for i, t in enumerate(tensors):
        p.p[i] = None if t is None else t.data_ptr()
    return p


def device_info(dev: int = 0):
    lib = _lib.load()
    name = C.create_string_buffer(64)
    cus, lds = C.c_int(), C.c_int()
    rc = lib.cnerf_device_info(dev, name, C.byref(cus), C.byref(lds))
    return rc == 0, name.value.decode(), cus.value, lds.value


# ------------------------------------------------------------------------------------------ weights
def pack_weights(spec: NetSpec, params: Sequence[Tensor], out: Optional[Tensor] = None) -> Tensor:
    lib, net = _lib.load(), spec.c()
    params = [_chk(p, f"param{i}") for i, p in enumerate(params)]
    n = lib.cnerf_packed_floats(C.byref(net))
    if n < 0:
        raise CnerfError(f"unsupported network {spec}")
    if out is None:
        out = torch.empty(n, device=params[0].device, dtype=torch.float32)
    ptrs = _ptrs(params)
    _lib.check(lib.cnerf_pack_weights(C.byref(net), C.byref(ptrs), _p(out), _stream()), "cnerf_pack_weights")
    return out


def pack_weights_pair(spec0: NetSpec, params0: Sequence[Tensor], out0: Optional[Tensor], spec1: NetSpec, params1: Sequence[Tensor],
                      out1: Optional[Tensor]):
    """cnerf_pack_weights_pair: both networks of a render_rays call re-packed by one launch -> (packed0, packed1)."""
    lib, n0, n1 = _lib.load(), spec0.c(), spec1.c()
    params0 = [_chk(p, f"param0[{i}]") for i, p in enumerate(params0)]
    params1 = [_chk(p, f"param1[{i}]") for i, p in enumerate(params1)]
    outs = []
    for net, spec, out, ps in ((n0, spec0, out0, params0), (n1, spec1, out1, params1)):
        n = lib.cnerf_packed_floats(C.byref(net))
        if n < 0:
            raise CnerfError(f"unsupported network {spec}")
        outs.append(out if out is not None else torch.empty(n, device=ps[0].device, dtype=torch.float32))
    p0, p1 = _ptrs(params0), _ptrs(params1)
    _lib.check(lib.cnerf_pack_weights_pair(C.byref(n0), C.byref(p0), _p(outs[0]), C.byref(n1), C.byref(p1), _p(outs[1]),
                                           _stream()), "cnerf_pack_weights_pair")
    return outs[0], outs[1]


# ------------------------------------------------------------------------------------------ sampling
_TVALS = {}


def _t_vals(n: int, device) -> Tensor:
    """torch.linspace(0,1,n) evaluated on the CPU (the reference's constants), cached per device."""
    key = (n, str(device))
    if key not in _TVALS:
        _TVALS[key] = torch.linspace(0., 1., steps=n).to(device)
    return _TVALS[key]


# In-kernel uniform streams (csrc/rng.hpp).  A stream is named by (seed, offset): both come from torch's OWN generator of the device
# — seed = its current seed, offset = its philox offset, which every draw advances by RNG_STRIDE (host-side integers: no launch, no
# sync) — so torch.manual_seed() / get_rng_state() / set_rng_state() govern these streams exactly like they govern torch.rand, and
# torch.rand calls in between keep their own numbers.  Under hipGraph capture the pair lives in device memory instead
# (RngCapture: graph.GraphedStep uploads {seed, offset} before every replay and advances the generator by what a replay consumes).
RNG_STRIDE = 4          # (torch's generator wants offsets in multiples of 4); one render_rays call: +0 jitter, +1 resampling
                        # (uniform), +2 coarse density noise, +3 fine density noise (standard normal)
IN_KERNEL_RNG = True    # False: render_rays draws t_rand / u with torch.rand and hands the tensors to the kernels (round-3 form)


class RngCapture:
    """Device-resident {seed, base offset} of the recording in progress; `used` = offsets one replay consumes."""
    active = None

    def __init__(self, device):
        self.state = torch.zeros(2, device=device, dtype=torch.int64)
        self.used = 0


@dataclass
class RngStream:
    seed: int
    offset: int
    state: Optional[Tensor] = None     # device int64[2] (capture mode)
    row0: int = 0

    def c(self, offset_add: int = 0, row0: Optional[int] = None) -> Rng:
        return Rng(self.seed & 0xFFFFFFFFFFFFFFFF, (self.offset + offset_add) & 0xFFFFFFFFFFFFFFFF,
                   None if self.state is None else self.state.data_ptr(), self.row0 if row0 is None else row0)


def rng_draw(device, row0: int = 0) -> RngStream:
    """Reserve RNG_STRIDE consecutive stream offsets from the device's generator.  One render_rays call: +0 jitter t_rand, +1
    resampling u (uniform streams), +2 density noise of the coarse level, +3 density noise of the fine level (normal streams);
    stand-alone raw2outputs: +2; run_nerf_view.add_label_noise: +0 rgb, +1 depth, +2 rgb0, +3 depth0 (normal streams)."""
    cap = RngCapture.active
    if cap is not None:
        st = RngStream(0, cap.used, cap.state, row0)
        cap.used += RNG_STRIDE
        return st
    if torch.cuda.is_current_stream_capturing():
        raise CnerfError("in-kernel random streams inside a hipGraph recording need graph.GraphedStep (or ops.IN_KERNEL_RNG = False)")
    gen = torch.cuda.default_generators[torch.device(device).index if torch.device(device).index is not None
                                        else torch.cuda.current_device()]
    off = gen.get_offset()
    gen.set_offset(off + RNG_STRIDE)
    return RngStream(gen.initial_seed(), off, None, row0)


def uniform_rng(rng: RngStream, rows: int, cols: int, device, offset_add: int = 0) -> Tensor:
    out = torch.empty(rows, cols, device=device, dtype=torch.float32)
    r = rng.c(offset_add)
    _lib.check(_lib.load().cnerf_uniform_rng(C.byref(r), rows, cols, _p(out), _stream()), "cnerf_uniform_rng")
    return out


def normal_rng(rng: RngStream, rows: int, cols: int, device, offset_add: int = 0, scale: float = 1.0,
               row0: Optional[int] = None) -> Tensor:
    """[rows, cols] = scale * the standard-normal stream `offset_add` of the block `rng` names (csrc/rng.hpp), rows
    [row0, row0 + rows) of the global draw (`row0` None: the stream's own)."""
    out = torch.empty(rows, cols, device=device, dtype=torch.float32)
    if rows == 0:      # (an empty tensor has no storage to point at)
        return out
    r = rng.c(offset_add, row0)
    _lib.check(_lib.load().cnerf_normal_rng(C.byref(r), rows, cols, float(scale), _p(out), _stream()), "cnerf_normal_rng")
    return out


def density_noise(rng: RngStream, B: int, Nc: int, S1: int, std: float, device):
    """The density noise (R:287-288) of one render_rays call, one launch: (noise0 [B, Nc], noise1 [B, S1] or None when S1 == 0) =
    std * the normal streams +2 and +3 of the block `rng` names."""
    noise0 = torch.empty(B, Nc, device=device, dtype=torch.float32)
    noise1 = torch.empty(B, S1, device=device, dtype=torch.float32) if S1 > 0 else None
    if B == 0:
        return noise0, noise1
    r = rng.c(2)
    _lib.check(_lib.load().cnerf_density_noise_rng(C.byref(r), B, Nc, S1, float(std), _p(noise0), _p(noise1), _stream()),
               "cnerf_density_noise_rng")
    return noise0, noise1


def coarse_z(rays: Tensor, Nc: int, t_rand: Optional[Tensor], lindisp: bool, rng: Optional[RngStream] = None) -> Tensor:
    rays = _chk(rays, "rays")
    B = rays.shape[0]
    t_rand = _chk(t_rand, "t_rand")
    z = torch.empty(B, Nc, device=rays.device, dtype=torch.float32)
    # the jitter: generated in the kernel (stream offset + 0), or t_rand (None: no jitter)
    name, jitter = ("cnerf_coarse_z_rng", C.byref(rng.c(0))) if rng is not None else ("cnerf_coarse_z", _p(t_rand))
    _lib.check(getattr(_lib.load(), name)(_p(rays), rays.shape[1], B, Nc, _p(_t_vals(Nc, rays.device)), jitter, int(lindisp), _p(z),
                                          _stream()), name)
    return z


def sample_pdf(bins: Tensor, weights: Tensor, u: Tensor, want_inds: bool = False):
    bins, weights, u = _chk(bins, "bins"), _chk(weights, "weights"), _chk(u, "u")
    B, Nb = bins.shape
    Nf = u.shape[-1]
    stride = 0 if u.dim() == 1 or u.shape[0] == 1 else Nf
    samples = torch.empty(B, Nf, device=bins.device, dtype=torch.float32)
    inds = torch.empty(B, Nf, device=bins.device, dtype=torch.int64) if want_inds else None
    _lib.check(_lib.load().cnerf_sample_pdf(_p(bins), _p(weights), _p(u), stride, B, Nb, Nf, _p(samples), _p(inds),
                                            _stream()), "cnerf_sample_pdf")
    return (samples, inds) if want_inds else samples


def resample(z: Tensor, weights: Tensor, u: Optional[Tensor], want_samples: bool = False, rng: Optional[RngStream] = None,
             Nf: Optional[int] = None):
    z, weights, u = _chk(z, "z"), _chk(weights, "weights"), _chk(u, "u")
    B, Nc = z.shape
    if rng is None:
        Nf = u.shape[-1]
    z_fine = torch.empty(B, Nc + Nf, device=z.device, dtype=torch.float32)
    z_std = torch.empty(B, device=z.device, dtype=torch.float32)
    samples = torch.empty(B, Nf, device=z.device, dtype=torch.float32) if want_samples else None
    inds = torch.empty(B, Nf, device=z.device, dtype=torch.int64) if want_samples else None
    if rng is not None:        # u generated in the kernel: stream offset + 1
        name, source = "cnerf_resample_rng", [C.byref(rng.c(1))]
    else:
        name, source = "cnerf_resample", [_p(u), 0 if u.dim() == 1 or u.shape[0] == 1 else Nf]
    _lib.check(getattr(_lib.load(), name)(_p(z), _p(weights), *source, B, Nc, Nf, _p(z_fine), _p(z_std), _p(samples), _p(inds), _stream()),
               name)
    return (z_fine, z_std, samples, inds) if want_samples else (z_fine, z_std)


# ------------------------------------------------------------------------------------------ MLP
def embed(x: Tensor, L: int) -> Tensor:
    x = _chk(x, "x")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, 3)
    out = torch.empty(x2.shape[0], 3 + 6 * L, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cnerf_embed(_p(x2), x2.shape[0], L, _p(out), _stream()), "cnerf_embed")
    return out.reshape(*lead, 3 + 6 * L)


# form of a forward -> (entry point, its arguments between (net, packed) and the stream, by the names _mlp_forward gathers)
_FWD_ENTRY = {
    "fp32": ("cnerf_mlp_fwd", ("pts", "rays", "rs", "dirs", "z", "B", "S", "raw", "stash")),
    "live": ("cnerf_mlp_fwd_live", ("rays", "rs", "z", "B", "S", "raw", "stash", "live")),
    "bf": ("cnerf_mlp_fwd_bf", ("planes", "pts", "rays", "rs", "dirs", "z", "B", "S", "raw")),
    "bf_train": ("cnerf_mlp_fwd_bf_train", ("pts", "rays", "rs", "dirs", "z", "B", "S", "raw", "stash")),
    "embedded": ("cnerf_mlp_fwd_embedded", ("x", "B", "raw", "stash")),
}
_FWD_INTS = ("rs", "B", "S", "planes")


def _mlp_forward(form, profile, spec: NetSpec, packed, shape, want_stash: bool, pts=None, rays=None, z=None, dirs=None, **more):
    """The one call of the forward wrappers: checks the inputs, allocates raw[*shape, raw_ch] (and the stash) and issues the entry point
    of `form` under the profile name -> (raw, stash or None).  `more`: what only one form takes (planes, live, x)."""
    lib, net, units = _lib.load(), spec.c(), int(np.prod(shape))
    a = dict(more, pts=_chk(pts, "pts"), rays=_chk(rays, "rays"), z=_chk(z, "z"), dirs=_chk(dirs, "dirs"), B=shape[0], S=shape[-1])
    a["rs"] = a["rays"].shape[1] if rays is not None else 0
    a["raw"] = torch.empty(*shape, spec.raw_ch, device=packed.device, dtype=torch.float32)
    a["stash"] = None
    if want_stash:
        a["stash"] = torch.empty(lib.cnerf_mlp_stash_floats(C.byref(net), units), device=packed.device, dtype=torch.float32)
    name, names = _FWD_ENTRY[form]
    with _timed(profile, units):
        _lib.check(getattr(lib, name)(C.byref(net), _p(packed), *[a[k] if k in _FWD_INTS else _p(a[k]) for k in names], _stream()), name)
    return a["raw"], a["stash"]


def mlp_forward(spec: NetSpec, packed: Tensor, B: int, S: int, *, pts: Optional[Tensor] = None,
                rays: Optional[Tensor] = None, z: Optional[Tensor] = None, dirs: Optional[Tensor] = None,
                want_stash: bool = False, live: Optional[Tensor] = None):
    """`live` (device int32 [1], training + rays form only): the batch is padded to the capacity B and only its first live[0] rays
    are real (cnerf_mlp_fwd_live): the launch is sized for B, tiles past the count leave zero raw outputs."""
    if live is None:
        return _mlp_forward("fp32", "mlp_fwd_train" if want_stash else "mlp_fwd", spec, packed, (B, S), want_stash, pts, rays, z, dirs)
    if not want_stash or rays is None or pts is not None or dirs is not None or live.dtype != torch.int32 or not live.is_cuda:
        raise CnerfError("mlp_forward(live=...) is the training forward on ray rows (no explicit points / directions); "
                         "live must be a device int32 tensor")
    return _mlp_forward("live", "mlp_fwd_train", spec, packed, (B, S), True, rays=rays, z=z, live=live)


# NeRF.inference_precision -> the `planes` argument of cnerf_packed_bf_bytes / cnerf_pack_weights_bf / cnerf_mlp_fwd_bf
PLANES_FP16X2 = 18                  # CNERF_PLANES_FP16X2: two fp16 planes per operand, three products on the f16 matrix cores
PRECISION_PLANES = {"bf16": 1, "bf16x2": 2, "bf16x3": 3, "fp16x2": PLANES_FP16X2}
# The fp16x2 scale rule (csrc/mlp_bf_common.hpp F16_SW / F16_SX; header of csrc/mlp_fwd_bf.hip): weights are packed as planes of
# w * 2^FP16X2_WEIGHT_SHIFT, encodings and activations split as planes of x * 2^FP16X2_ACT_SHIFT, so the fp32 accumulators hold
# 2^(sum) times the true value; biases are packed with that factor and the sigma / rgb head weights with its inverse.
FP16X2_WEIGHT_SHIFT, FP16X2_ACT_SHIFT = 8, 4
FP16X2_MAX_WEIGHT = 65504.0 / 2 ** FP16X2_WEIGHT_SHIFT       # |w| above this overflows the fp16 plane
FP16X2_MAX_ACTIVATION = 65504.0 / 2 ** FP16X2_ACT_SHIFT      # likewise sample positions, hidden activations and features
_BF_PROFILE = {1: "mlp_fwd_bf1", 2: "mlp_fwd_bf2", 3: "mlp_fwd_bf3", PLANES_FP16X2: "mlp_fwd_fp16x2"}


def pack_weights_bf(spec: NetSpec, params: Sequence[Tensor], planes: int, out: Optional[Tensor] = None) -> Tensor:
    """cnerf_pack_weights_bf: the bf16-plane (planes = 1, 2, 3) or fp16-plane (PLANES_FP16X2) panels of the opt-in
    reduced-precision inference forward (a byte buffer).  One launch, no host synchronisation: capturable."""
    lib, net = _lib.load(), spec.c()
    params = [_chk(p, f"param{i}") for i, p in enumerate(params)]
    n = lib.cnerf_packed_bf_bytes(C.byref(net), int(planes))
    if n < 0:
        raise CnerfError(f"reduced-precision inference is not compiled for {spec} with {planes} plane(s)")
    if out is None:
        out = torch.empty(n, device=params[0].device, dtype=torch.uint8)
    ptrs = _ptrs(params)
    _lib.check(lib.cnerf_pack_weights_bf(C.byref(net), C.byref(ptrs), int(planes), _p(out), _stream()), "cnerf_pack_weights_bf")
    return out


def mlp_forward_bf(spec: NetSpec, packed_bf: Tensor, planes: int, B: int, S: int, *, pts: Optional[Tensor] = None,
                   rays: Optional[Tensor] = None, z: Optional[Tensor] = None, dirs: Optional[Tensor] = None) -> Tensor:
    """cnerf_mlp_fwd_bf: inference forward on the bf16 / f16 matrix cores (opt-in); `planes` as packed."""
    return _mlp_forward("bf", _BF_PROFILE.get(int(planes), "mlp_fwd_bf%d" % planes), spec, packed_bf, (B, S), False, pts, rays, z, dirs,
                        planes=int(planes))[0]


def mlp_forward_bf_train(spec: NetSpec, packed_bf: Tensor, B: int, S: int, *, pts: Optional[Tensor] = None,
                         rays: Optional[Tensor] = None, z: Optional[Tensor] = None, dirs: Optional[Tensor] = None):
    """cnerf_mlp_fwd_bf_train: the OPT-IN bf16x3 training forward (three bf16 planes per operand, fp32 accumulation) ->
    (raw, stash); the stash is the fp32 kernel's (cnerf_mlp_dgrad / cnerf_mlp_wgrad consume it unchanged)."""
    return _mlp_forward("bf_train", "mlp_fwd_train_bf3", spec, packed_bf, (B, S), True, pts, rays, z, dirs)


def mlp_forward_embedded(spec: NetSpec, packed: Tensor, x: Tensor, want_stash: bool = False):
    """NeRF.forward on pre-embedded inputs x[M, in_ch + in_ch_views]."""
    x = _chk(x, "x")
    return _mlp_forward("embedded", "mlp_fwd_train" if want_stash else "mlp_fwd", spec, packed, (x.shape[0],), want_stash, x=x)


# (pair, live, bf) -> the calls of one backward as (stage, entry point, profile name): the two halves where they exist (bench.py's
# HIP events bracket each kernel), the combined call otherwise
_BWD_ENTRY = {
    (False, False, False): (("dgrad", "cnerf_mlp_dgrad", "mlp_dgrad"), ("wgrad", "cnerf_mlp_wgrad", "mlp_wgrad")),
    (False, False, True): (("dgrad", "cnerf_mlp_dgrad_bf", "mlp_dgrad_bf3"), ("wgrad", "cnerf_mlp_wgrad_bf", "mlp_wgrad_bf3")),
    (False, True, False): (("bwd", "cnerf_mlp_bwd_live", "mlp_bwd_live"),),
    (True, False, False): (("dgrad", "cnerf_mlp_dgrad_pair", "mlp_dgrad"), ("wgrad", "cnerf_mlp_wgrad_pair", "mlp_wgrad")),
    (True, False, True): (("dgrad", "cnerf_mlp_dgrad_bf_pair", "mlp_dgrad_bf3"), ("wgrad", "cnerf_mlp_wgrad_bf_pair", "mlp_wgrad_bf3")),
    (True, True, False): (("dgrad", "cnerf_mlp_dgrad_pair_live", "mlp_dgrad"), ("wgrad", "cnerf_mlp_wgrad_pair_live", "mlp_wgrad")),
}


def mlp_bwd_workspace(spec: NetSpec, B: int, S: int, device) -> Tensor:
    """The caller-owned workspace of one level's backward (cnerf_mlp_bwd_ws_floats): dZ of every layer, then the wgrad partials."""
    net = spec.c()
    return torch.empty(_lib.load().cnerf_mlp_bwd_ws_floats(C.byref(net), B * S), device=device, dtype=torch.float32)


def _mlp_backward(levels, accumulate, bf, live, first=(), ws=None):
    """One backward over `levels`, one or two of (spec, packed, d_raw, B, S, stash, grads) with `packed` the buffer of the chosen
    arithmetic.  `units` of the profile records is the launch CAPACITY (with `live` the point count is on the device: the bench
    rescales by the step's live rows).  `ws`: the workspace(s) to run in, for a caller that reads dZ afterwards — one tensor (one
    level) or a tuple with one per level (mlp_input_grad / mlp_input_grad_pair); otherwise allocated here and dropped."""
    lib = _lib.load()
    dgrad, wgrad, units, keep = [], [], 0, []
    own = ws if isinstance(ws, (tuple, list)) else (ws,) + (None,) * (len(levels) - 1)
    if len(own) != len(levels):
        raise CnerfError("_mlp_backward: one workspace per level")
    for i, (spec, packed, d_raw, B, S, stash, grads) in enumerate(levels):
        net, ptrs = spec.c(), _ptrs(grads)
        d_raw = _chk(d_raw, "d_raw" if len(levels) == 1 else "d_raw%d" % i)
        ws = own[i] if own[i] is not None else mlp_bwd_workspace(spec, B, S, packed.device)
        dgrad.append([C.byref(net), _p(packed), _p(d_raw), B, S, _p(stash), _p(ws)])
        wgrad.append([C.byref(net), B, S, _p(stash), _p(ws), C.byref(ptrs)])
        units += B * S
        keep += [d_raw, ws]      # (alive until the launches are enqueued: a freed workspace would be handed to the next level)
    tail = ([] if live is None else [_p(live)]) + [int(f) for f in first]
    args = {"dgrad": [a for lv in dgrad for a in lv] + tail,
            "wgrad": [a for lv in wgrad for a in lv] + [int(accumulate)] + tail,
            "bwd": [a for d, w in zip(dgrad, wgrad) for a in d + w[-1:]] + [int(accumulate)] + tail}
    for stage, name, profile in _BWD_ENTRY[len(levels) == 2, live is not None, bool(bf)]:
        with _timed(profile, units):
            _lib.check(getattr(lib, name)(*args[stage], _stream()), name)


def mlp_backward(spec: NetSpec, packed: Tensor, d_raw: Tensor, B: int, S: int, stash: Tensor,
                 grads: Optional[List[Tensor]] = None, accumulate: bool = False, packed_bf: Optional[Tensor] = None,
                 live: Optional[Tensor] = None, ws: Optional[Tensor] = None) -> List[Tensor]:
    """packed_bf (the three-plane buffer of pack_weights_bf): the dgrad and wgrad run in the opt-in bf16x3 arithmetic.
    live: the forward ran through mlp_forward(live=...) — the backward stops at the same device-side row count (exact fp32).
    ws (mlp_bwd_workspace): run in this workspace, for a caller that reads dZ afterwards (mlp_input_grad)."""
    if grads is None:
        grads = [torch.empty(s, device=packed.device, dtype=torch.float32) for s in spec.tensor_shapes()]
        accumulate = False
    bf = packed_bf is not None
    if live is not None and bf:
        raise CnerfError("mlp_backward(live=...) is an exact-fp32 path")
    _mlp_backward([(spec, packed_bf if bf else packed, d_raw, B, S, stash, grads)], accumulate, bf, live, ws=ws)
    return grads


def mlp_dgrad(spec: NetSpec, packed: Tensor, d_raw: Tensor, B: int, S: int, stash: Tensor, ws: Tensor,
              packed_bf: Optional[Tensor] = None) -> Tensor:
    """cnerf_mlp_dgrad (packed_bf: cnerf_mlp_dgrad_bf) on its own: dZ of every layer into `ws` (mlp_bwd_workspace), no parameter
    gradients — the backward of a frozen network whose inputs take a gradient (mlp_input_grad reads `ws`)."""
    net, d_raw = spec.c(), _chk(d_raw, "d_raw")
    name, profile, pk = ("cnerf_mlp_dgrad_bf", "mlp_dgrad_bf3", packed_bf) if packed_bf is not None else ("cnerf_mlp_dgrad", "mlp_dgrad", packed)
    with _timed(profile, B * S):
        _lib.check(getattr(_lib.load(), name)(C.byref(net), _p(pk), _p(d_raw), B, S, _p(stash), _p(ws), _stream()), name)
    return ws


def mlp_input_grad(spec: NetSpec, packed: Tensor, B: int, S: int, stash: Tensor, ws: Tensor, want_dirs: bool = False):
    """cnerf_mlp_input_grad, behind the dgrad of the same level in `ws` (mlp_backward(ws=...) or mlp_dgrad) ->
    (d_pts [B*S, 3], d_dirs_pt [B*S, 3] | None): the gradient w.r.t. every sample position and, per point, w.r.t. its ray's view
    direction (rays_input_grad sums those per ray).  `packed`: the fp32 panels, also behind a bf16x3 dgrad."""
    net = spec.c()
    d_pts = torch.empty(B * S, 3, device=packed.device, dtype=torch.float32)
    d_dirs = torch.empty(B * S, 3, device=packed.device, dtype=torch.float32) if want_dirs else None
    with _timed("mlp_input_grad", B * S):
        _lib.check(_lib.load().cnerf_mlp_input_grad(C.byref(net), _p(packed), B, S, _p(stash), _p(ws), _p(d_pts), _p(d_dirs), _stream()),
                   "cnerf_mlp_input_grad")
    return d_pts, d_dirs


def rays_input_grad(d_pts: Optional[Tensor], d_dirs_pt: Optional[Tensor], z: Optional[Tensor], B: int, S: int,
                    ray_stride: Optional[int] = None) -> Tensor:
    """cnerf_rays_input_grad.  ray_stride None -> d_viewdirs [B, 3] = the per-ray sum of d_dirs_pt (the points form).  Otherwise ->
    the gradient of the [B, ray_stride] ray rows the level read: columns 0:3 = sum_s d_pts, 3:6 = sum_s z d_pts, and with d_dirs_pt
    the last three columns = its per-ray sum; every other column zero."""
    lib = _lib.load()
    if ray_stride is None:
        out = torch.empty(B, 3, device=d_dirs_pt.device, dtype=torch.float32)
        _lib.check(lib.cnerf_rays_input_grad(None, _p(d_dirs_pt), None, B, S, None, None, _p(out), 3, _stream()), "cnerf_rays_input_grad")
        return out
    z = _chk(z, "z")
    out = torch.zeros(B, ray_stride, device=d_pts.device, dtype=torch.float32)
    _lib.check(lib.cnerf_rays_input_grad(_p(d_pts), _p(d_dirs_pt), _p(z), B, S, _p(out), _p(out[:, 3:]),
                                         _p(out[:, ray_stride - 3:]) if d_dirs_pt is not None else None, ray_stride, _stream()),
               "cnerf_rays_input_grad")
    return out


def composite_norm_grad(d_raw: Tensor, raw: Tensor, noise: Optional[Tensor], rays: Tensor) -> Tensor:
    """cnerf_composite_norm_grad: the gradient of raw2outputs w.r.t. the ray rows, which enter through dists * |rays_d| only (R:283),
    from the d_raw of composite_backward -> [B, ray_stride], columns 3:6 filled."""
    d_raw, raw, noise, rays = _chk(d_raw, "d_raw"), _chk(raw, "raw"), _chk(noise, "noise"), _chk(rays, "rays")
    B, S = raw.shape[0], raw.shape[1]
    out = torch.zeros_like(rays)
    _lib.check(_lib.load().cnerf_composite_norm_grad(_p(d_raw), _p(raw), raw.shape[-1], _p(noise), _p(rays), rays.shape[1], B, S,
                                                     _p(out[:, 3:]), rays.shape[1], _stream()), "cnerf_composite_norm_grad")
    return out


def mlp_backward_pair(spec0: NetSpec, packed0: Tensor, d_raw0: Tensor, B0: int, S0: int, stash0: Tensor, grads0: List[Tensor],
                      spec1: NetSpec, packed1: Tensor, d_raw1: Tensor, B1: int, S1: int, stash1: Tensor, grads1: List[Tensor],
                      accumulate: bool = False, packed_bf0: Optional[Tensor] = None, packed_bf1: Optional[Tensor] = None,
                      live: Optional[Tensor] = None, first0: int = 0, first1: int = 0, ws=None):
    """cnerf_mlp_bwd_pair: the backward of two independent networks (coarse / fine) as one dgrad grid, one wgrad grid and
    one reduction; gradients are written (or accumulated) into grads0 / grads1.  packed_bf0 AND packed_bf1: the dgrad and wgrad
    grids run in the opt-in bf16x3 arithmetic.  live: both levels belong to one ray batch whose live row count sits on the device
    (mlp_forward(live=...)): the halves of cnerf_mlp_bwd_pair_live (exact fp32); first0 / first1: that level's first rays carry
    zero seeds and are left out of its backward.  ws = (ws0, ws1) (mlp_bwd_workspace each): run in these workspaces, which are the
    caller's and hold dZ of both levels afterwards (mlp_input_grad_pair reads them)."""
    if live is not None and (packed_bf0 is not None or packed_bf1 is not None):
        raise CnerfError("mlp_backward_pair(live=...) is an exact-fp32 path")
    bf = packed_bf0 is not None and packed_bf1 is not None
    _mlp_backward([(spec0, packed_bf0 if bf else packed0, d_raw0, B0, S0, stash0, grads0),
                   (spec1, packed_bf1 if bf else packed1, d_raw1, B1, S1, stash1, grads1)],
                  accumulate, bf, live, (first0, first1) if live is not None else (), ws=ws)


def mlp_input_grad_pair(spec0: NetSpec, packed0: Tensor, B0: int, S0: int, stash0: Tensor, ws0: Tensor,
                        spec1: NetSpec, packed1: Tensor, B1: int, S1: int, stash1: Tensor, ws1: Tensor, want_dirs: bool = False):
    """cnerf_mlp_input_grad_pair: mlp_input_grad of two levels as one grid, behind mlp_backward_pair(ws=(ws0, ws1)) ->
    ((d_pts0, d_dirs_pt0 | None), (d_pts1, d_dirs_pt1 | None)), each the bits of the single call.  `packed`: the fp32 panels, also
    behind the bf16x3 pair."""
    n0, n1 = spec0.c(), spec1.c()
    dev = packed0.device
    out = [torch.empty(B * S, 3, device=dev, dtype=torch.float32) if on else None
           for B, S in ((B0, S0), (B1, S1)) for on in (True, want_dirs)]
    with _timed("mlp_input_grad_pair", B0 * S0 + B1 * S1):
        _lib.check(_lib.load().cnerf_mlp_input_grad_pair(C.byref(n0), _p(packed0), B0, S0, _p(stash0), _p(ws0), _p(out[0]), _p(out[1]),
                                                         C.byref(n1), _p(packed1), B1, S1, _p(stash1), _p(ws1), _p(out[2]), _p(out[3]),
                                                         _stream()), "cnerf_mlp_input_grad_pair")
    return (out[0], out[1]), (out[2], out[3])


def rays_input_grad_pair(d_pts0: Tensor, d_dirs_pt0: Optional[Tensor], z0: Tensor, d_pts1: Tensor, d_dirs_pt1: Optional[Tensor],
                         z1: Tensor, ray_stride: int) -> Tensor:
    """cnerf_rays_input_grad_pair: rays_input_grad(level 0) + rays_input_grad(level 1) of one ray batch, bit for bit, as one launch
    that writes every column of the [B, ray_stride] result (no fill in front).  z0 [B, S0], z1 [B, S1]."""
    z0, z1 = _chk(z0, "z0"), _chk(z1, "z1")
    B = z0.shape[0]
    if z1.shape[0] != B:
        raise CnerfError("rays_input_grad_pair: the two levels belong to one ray batch")
    for t, zz, name in ((d_pts0, z0, "d_pts0"), (d_dirs_pt0, z0, "d_dirs_pt0"), (d_pts1, z1, "d_pts1"), (d_dirs_pt1, z1, "d_dirs_pt1")):
        if t is not None and (t.numel() != zz.numel() * 3 or not t.is_contiguous() or t.dtype != torch.float32 or t.device != zz.device):
            raise CnerfError(f"rays_input_grad_pair: {name} must be a contiguous float32 [B * S, 3] on the device of its level's z")
    out = torch.empty(B, ray_stride, device=z0.device, dtype=torch.float32)
    with _timed("rays_input_grad_pair", z0.numel() + z1.numel()):
        _lib.check(_lib.load().cnerf_rays_input_grad_pair(_p(d_pts0), _p(d_dirs_pt0), _p(z0), z0.shape[1], _p(d_pts1), _p(d_dirs_pt1), _p(z1),
                                                          z1.shape[1], B, _p(out), ray_stride, _stream()), "cnerf_rays_input_grad_pair")
    return out


def composite_norm_grad_pair(d_raw0: Tensor, raw0: Tensor, noise0: Optional[Tensor], d_raw1: Tensor, raw1: Tensor,
                             noise1: Optional[Tensor], rays: Tensor) -> Tensor:
    """cnerf_composite_norm_grad_pair: composite_norm_grad(level 0) + composite_norm_grad(level 1) for two levels that read the
    same ray rows, bit for bit, as one launch that writes every column of the result."""
    d_raw0, raw0, noise0 = _chk(d_raw0, "d_raw0"), _chk(raw0, "raw0"), _chk(noise0, "noise0")
    d_raw1, raw1, noise1 = _chk(d_raw1, "d_raw1"), _chk(raw1, "raw1"), _chk(noise1, "noise1")
    rays = _chk(rays, "rays")
    B = rays.shape[0]
    if raw0.shape[0] != B or raw1.shape[0] != B:
        raise CnerfError("composite_norm_grad_pair: the two levels belong to one ray batch")
    for d, r, nz, lv in ((d_raw0, raw0, noise0, 0), (d_raw1, raw1, noise1, 1)):
        if d.shape != r.shape or r.dim() != 3 or (nz is not None and nz.shape != r.shape[:2]):
            raise CnerfError(f"composite_norm_grad_pair: level {lv}: d_raw and raw are [B, S, ch] alike, noise [B, S]")
    out = torch.empty_like(rays)
    with _timed("composite_norm_grad_pair", raw0.shape[0] * (raw0.shape[1] + raw1.shape[1])):
        _lib.check(_lib.load().cnerf_composite_norm_grad_pair(_p(d_raw0), _p(raw0), raw0.shape[-1], _p(noise0), raw0.shape[1],
                                                              _p(d_raw1), _p(raw1), raw1.shape[-1], _p(noise1), raw1.shape[1],
                                                              _p(rays), rays.shape[1], B, _p(out), _stream()),
                   "cnerf_composite_norm_grad_pair")
    return out


# ------------------------------------------------------------------------------------------ render_rays as one call
class RenderState:
    """What cnerf_render_bwd needs from the forward call it follows: the workspace (z, raw, weights, stashes) and the
    call's arguments."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _render_setup(spec_c: NetSpec, spec_f: Optional[NetSpec], B: int, dev, Nc, Nf, lindisp, white_bkgd, ray_stride, train, retraw, u):
    """What cnerf_render_fwd and cnerf_render_fwd_cam take alike -> (lib, config, coarse net, pointer to the fine net | None,
    workspace, the dict of output maps, its struct cnerf_render_out, the row stride of u)."""
    lib = _lib.load()
    cfg = RenderCfg(int(Nc), int(Nf), int(lindisp), int(white_bkgd), int(ray_stride), int(train))
    nc, nf = spec_c.c(), (spec_f.c() if spec_f is not None else None)
    nfp = C.byref(nf) if nf is not None else None
    n = lib.cnerf_render_ws_floats(C.byref(nc), nfp, C.byref(cfg), B)
    if n < 0:
        raise CnerfError("cnerf_render_ws_floats: inconsistent arguments")
    ws = torch.empty(n, device=dev, dtype=torch.float32)
    ch = (spec_f if (spec_f is not None and Nf > 0) else spec_c).raw_ch
    o = {k: torch.empty(B, 3, device=dev) if k.startswith("rgb") else torch.empty(B, device=dev)
         for k in ("rgb_map", "disp_map", "acc_map", "depth_map") + (("rgb0", "disp0", "acc0", "depth0", "z_std") if Nf > 0 else ())}
    if retraw:
        o["raw"] = torch.empty(B, Nc + Nf, ch, device=dev)
    out = RenderOut(**{k: v.data_ptr() for k, v in o.items()})
    stride = 0 if (u is None or u.dim() == 1 or u.shape[0] == 1) else Nf
    return lib, cfg, nc, nfp, ws, o, out, stride


def render_forward(spec_c: NetSpec, packed_c: Tensor, spec_f: Optional[NetSpec], packed_f: Optional[Tensor], rays: Tensor,
                   Nc: int, Nf: int, t_rand: Optional[Tensor] = None, u: Optional[Tensor] = None,
                   noise0: Optional[Tensor] = None, noise1: Optional[Tensor] = None, lindisp: bool = False,
                   white_bkgd: bool = False, train: bool = False, retraw: bool = False):
    """cnerf_render_fwd: render_rays (R:311-421 / V:441-551) of one ray batch in one C call.  Returns (dict with the
    reference's keys + depth maps, RenderState for render_backward)."""
    if train and rays.requires_grad and torch.is_grad_enabled():
        raise CnerfError("render_forward / render_backward (the one-call cnerf_render_fwd / cnerf_render_bwd): gradients w.r.t. rays "
                         "are not implemented (parameter gradients only; run_nerf.render(rays=...) has them)")
    rays, t_rand, u = _chk(rays, "rays"), _chk(t_rand, "t_rand"), _chk(u, "u")
    noise0, noise1 = _chk(noise0, "noise0"), _chk(noise1, "noise1")
    B, dev = rays.shape[0], rays.device
    lib, cfg, nc, nfp, ws, o, out, stride = _render_setup(spec_c, spec_f, B, dev, Nc, Nf, lindisp, white_bkgd, rays.shape[1], train,
                                                          retraw, u)
    _lib.check(lib.cnerf_render_fwd(C.byref(nc), _p(packed_c), nfp, _p(packed_f), _p(rays), B, C.byref(cfg),
                                    _p(_t_vals(Nc, dev)), _p(t_rand), _p(u), stride, _p(noise0), _p(noise1), C.byref(out),
                                    _p(ws), _stream()), "cnerf_render_fwd")
    st = RenderState(spec_c=spec_c, packed_c=packed_c, spec_f=spec_f, packed_f=packed_f, rays=rays, B=B, cfg=cfg,
                     noise0=noise0, noise1=noise1, ws=ws)
    return o, st


def render_forward_cam(spec_c: NetSpec, packed_c: Tensor, spec_f: Optional[NetSpec], packed_f: Optional[Tensor], H: int, W: int,
                       K, c2w, near: float, far: float, use_viewdirs: bool, ndc: bool, ndc_coef, first: int, B: int, Nc: int,
                       Nf: int, t_rand: Optional[Tensor] = None, u: Optional[Tensor] = None, noise0: Optional[Tensor] = None,
                       noise1: Optional[Tensor] = None, lindisp: bool = False, white_bkgd: bool = False, retraw: bool = False):
    """cnerf_render_fwd_cam: render_rays (inference) of the image chunk [first, first + B) of a camera whose rays are
    generated inside the kernels — no [H*W, 11] ray tensor.  Returns the dict of cnerf_render_fwd."""
    t_rand, u, noise0, noise1 = _chk(t_rand, "t_rand"), _chk(u, "u"), _chk(noise0, "noise0"), _chk(noise1, "noise1")
    lib, cfg, nc, nfp, ws, o, out, stride = _render_setup(spec_c, spec_f, B, packed_c.device, Nc, Nf, lindisp, white_bkgd, 11, 0, retraw, u)
    cam = RayGen(int(H), int(W), *_intrinsics(K), _f4(c2w), float(near), float(far), int(use_viewdirs), int(ndc), float(ndc_coef[0]),
                 float(ndc_coef[1]), int(first))
    with _timed("render_fwd_cam", B * (Nc + (Nc + Nf if Nf > 0 else 0))):
        _lib.check(lib.cnerf_render_fwd_cam(C.byref(nc), _p(packed_c), nfp, _p(packed_f), C.byref(cam), B, C.byref(cfg),
                                            _p(_t_vals(Nc, packed_c.device)), _p(t_rand), _p(u), stride, _p(noise0), _p(noise1),
                                            C.byref(out), _p(ws), _stream()), "cnerf_render_fwd_cam")
    return o


def render_backward(st: RenderState, grads_in: dict, grads_c: List[Tensor], grads_f: Optional[List[Tensor]],
                    accumulate: bool = False):
    """cnerf_render_bwd: upstream gradients of the maps (dict with any of rgb_map, disp_map, acc_map, depth_map, rgb0,
    disp0, acc0, depth0) -> parameter gradients of the coarse / fine network, written into the given tensors."""
    lib = _lib.load()
    keep = {k: _chk(v, k) for k, v in grads_in.items() if v is not None}
    g = RenderGrads(**{"g_" + k: v.data_ptr() for k, v in keep.items()})
    nc, nf = st.spec_c.c(), (st.spec_f.c() if st.spec_f is not None else None)
    pc, pf = _ptrs(grads_c), (_ptrs(grads_f) if grads_f is not None else None)
    _lib.check(lib.cnerf_render_bwd(C.byref(nc), _p(st.packed_c), C.byref(nf) if nf is not None else None,
                                    _p(st.packed_f), _p(st.rays), st.B, C.byref(st.cfg), _p(st.noise0), _p(st.noise1),
                                    C.byref(g), _p(st.ws), C.byref(pc), C.byref(pf) if pf is not None else None,
                                    int(accumulate), _stream()), "cnerf_render_bwd")


# ------------------------------------------------------------------------------------------ compositing
def _composite_args(raw, z, rays, noise, white_bkgd):
    """-> (the checked raw, B, S, the nine arguments every compositing entry point starts with, the checked tensors those point
    into: the caller holds them until its launch is enqueued)."""
    keep = raw, z, rays, noise = _chk(raw, "raw"), _chk(z, "z"), _chk(rays, "rays"), _chk(noise, "noise")
    B, S = z.shape
    return raw, B, S, (_p(raw), raw.shape[-1], _p(z), _p(rays), rays.shape[1], _p(noise), B, S, int(white_bkgd)), keep


def _composite_outputs(B, S, dev):
    """(rgb, disp, acc, depth, weights) in the order the compositing entry points take them; the wrappers return weights fourth."""
    return (torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev),
            torch.empty(B, S, device=dev))


def composite_forward(raw: Tensor, z: Tensor, rays: Tensor, noise: Optional[Tensor], white_bkgd: bool):
    raw, B, S, pre, _keep = _composite_args(raw, z, rays, noise, white_bkgd)
    rgb, disp, acc, depth, weights = outs = _composite_outputs(B, S, raw.device)
    _lib.check(_lib.load().cnerf_composite_fwd(*pre, *map(_p, outs), _stream()), "cnerf_composite_fwd")
    return rgb, disp, acc, weights, depth


_MSE_COUNTERS = {}


def _mse_counter(device) -> Tensor:
    """The ticket counters of cnerf_composite_fwd_mse: one zeroed block per (device, stream) — the kernel leaves it zero.  Under a
    hipGraph recording: the block the recorder allocated BEFORE the recording and owns (prepare_capture: one per GraphedStep, so
    two recorded steps replayed concurrently on different streams never share tickets; memory allocated inside a recording
    belongs to that graph's pool and must not be cached); without a recorder, a throw-away zeroed block owned by the graph."""
    if torch.cuda.is_current_stream_capturing():
        t = _MSE_COUNTERS.get((str(device), "graph"))
        return t if t is not None else torch.zeros(_mse_counter_words(), device=device, dtype=torch.int32)
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    if key not in _MSE_COUNTERS:
        _MSE_COUNTERS[key] = torch.zeros(_mse_counter_words(), device=device, dtype=torch.int32)
    return _MSE_COUNTERS[key]


def _mse_counter_words() -> int:
    return int(_lib.load().cnerf_composite_mse_counter_words())


def composite_mse_max_rays() -> int:
    return int(_lib.load().cnerf_composite_mse_max_rays())


def prepare_capture(device) -> Tensor:
    """Allocate, outside the recording, what the kernels of a recorded step keep across replays: a ticket-counter block of the
    recording's OWN (returned: the recorder keeps it alive as long as its graph) — installed as the block launches recorded on this
    device use until end_capture()."""
    t = torch.zeros(_mse_counter_words(), device=device, dtype=torch.int32)
    _MSE_COUNTERS[(str(torch.device(device)), "graph")] = t
    return t


def end_capture(device):
    _MSE_COUNTERS.pop((str(torch.device(device)), "graph"), None)


def composite_forward_mse(raw: Tensor, z: Tensor, rays: Tensor, noise: Optional[Tensor], white_bkgd: bool, target: Tensor,
                          loss_add: Optional[Tensor] = None):
    """cnerf_composite_fwd_mse -> (rgb, disp, acc, weights, depth, loss[1]): raw2outputs + img2mse(rgb_map, target) (+ loss_add)."""
    raw, B, S, pre, _keep = _composite_args(raw, z, rays, noise, white_bkgd)
    target, loss_add = _chk(target, "target"), _chk(loss_add, "loss_add")
    if B == 0 or tuple(target.shape) != (B, 3):
        raise CnerfError(f"composite_forward_mse: target must be [{B}, 3] with B > 0, got {tuple(target.shape)}")
    dev = raw.device
    rgb, disp, acc, depth, weights = outs = _composite_outputs(B, S, dev)
    loss = torch.empty(1, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.cnerf_composite_mse_ws_floats(B) // 2, device=dev, dtype=torch.float64)
    _lib.check(lib.cnerf_composite_fwd_mse(*pre, _p(target), _p(loss_add), *map(_p, outs), _p(loss), _p(ws), _p(_mse_counter(dev)),
                                           _stream()), "cnerf_composite_fwd_mse")
    return rgb, disp, acc, weights, depth, loss


def composite_backward_mse(raw, z, rays, noise, white_bkgd, rgb, target, g_loss) -> Tensor:
    """cnerf_composite_bwd_mse: d_raw of mean((rgb_map - target)^2) * g_loss (a device scalar, or None = 1)."""
    raw, _, _, pre, _keep = _composite_args(raw, z, rays, noise, white_bkgd)
    rgb, target, g_loss = _chk(rgb, "rgb"), _chk(target, "target"), _chk(g_loss, "g_loss")
    d_raw = torch.empty_like(raw)
    _lib.check(_lib.load().cnerf_composite_bwd_mse(*pre, _p(rgb), _p(target), _p(g_loss), _p(d_raw), _stream()), "cnerf_composite_bwd_mse")
    return d_raw


RGB_FORMS = ("hardmask", "softlp", "softmask")                                            # CNERF_RGB_*
DEPTH_FORMS = ("hardmask", "hardmask_coef", "norm", "plain", "softlp", "softmask")        # CNERF_DEPTH_*


# ---- the ConsistentNeRF losses folded into compositing (cnerf_composite_fwd_closs / cnerf_closs_finish / cnerf_composite_bwd_closs)
@dataclass
class ClossSpec:
    """The loss of one ConsistentNeRF training batch (V:1645-1865): masked rgb + depth terms on every level (mask [B] 0/1 floats or
    None; prior [B] or None = no depth term; depths compared after / far), the monocular patch term on the first P * n rays (mono
    [P * n] or None), weights of the three kinds of term in the step's loss, optional GLOBAL (n1, n0) for a sharded batch."""
    target: Tensor
    mask: Optional[Tensor] = None
    prior: Optional[Tensor] = None
    far: float = 1.0
    coef: float = 0.2
    rgb_w: float = 1.0
    depth_w: float = 1.0
    patch_w: float = 0.001
    mono: Optional[Tensor] = None
    P: int = 0
    n: int = 256
    counts: Optional[Tensor] = None
    ss_coins: Optional[tuple] = None      # (rgb, depth, rgb0, depth0) draws of VT:941-969: the in-loop consistency step's primary terms
    seg_row: int = 0                      # > 0 (with ss_coins): the batch is [primary rays | warped rays + padding] cut here (ss_batch)
    counts3: Optional[Tensor] = None      # (with seg_row) GLOBAL (selected, primary, warped) ray counts of a batch sharded over ranks
    ssim_w: float = 0.0                   # V's patch SSIM term (loss -= ssim_w ssim_level per level; 0 = none) over the first
    ssim_P: int = 0                       # ssim_P patches of 16 x 16 rays (cnerf_closs_finish_ssim)
    rgb_form: int = 0                     # RGB_FORMS / DEPTH_FORMS index (cnerf_lossform): any non-zero one takes the *_lossform
    depth_form: int = 0                   # entry points
    lp_coef: float = 0.0                  # the exponent of a softlp form (args.Lp_coef)
    temps: Optional[tuple] = None         # 0-d device tensors (temp_rgb, temp_depth, temp_rgb coarse, temp_depth coarse) or None each
    lpips_w: float = 0.0                  # V's patch LPIPS term (loss += lpips_w lpips_level per level; 0 = none) over the first lpips_P
    lpips_P: int = 0                      # patches of 16 x 16 rays, through ONE batched pass of the packed network lpips_packed
    lpips_packed: Optional[Tensor] = None  # (lpips_pack's blob: cnerf_lpips_pack_patches, cnerf_closs_finish_lpips); default forms only

    @property
    def forms(self) -> bool:
        return bool(self.rgb_form or self.depth_form)

    def form_c(self, level: int) -> LossForm:
        """struct cnerf_lossform of a level (0 = the last / fine one, 1 = coarse)."""
        t = self.temps or (None,) * 4
        return LossForm(int(self.rgb_form), int(self.depth_form), float(self.lp_coef), _addr(t[2 * level]), _addr(t[2 * level + 1]))

    def c(self) -> Closs:
        return Closs(self.target.data_ptr(), _addr(self.mask), _addr(self.prior), float(self.far), int(self.seg_row))

    def checked(self, B: int) -> "ClossSpec":
        t = _chk(self.target.reshape(-1, 3), "target")
        if t.shape[0] != B or B == 0:
            raise CnerfError(f"closs: target must be [{B}, 3] with B > 0, got {tuple(self.target.shape)}")
        m = None if self.mask is None else _chk(self.mask.reshape(-1).to(torch.float32), "mask")
        pr = None if self.prior is None else _chk(self.prior.reshape(-1), "prior")
        mono = None if (self.mono is None or self.P <= 0) else _chk(self.mono.reshape(-1), "mono")
        for x, nme in ((m, "mask"), (pr, "prior")):
            if x is not None and x.numel() != B:
                raise CnerfError(f"closs: {nme} must have {B} elements, got {x.numel()}")
        P = int(self.P) if mono is not None else 0
        if P > 0 and (mono.numel() < P * self.n or P * self.n > B or P > 8):
            raise CnerfError(f"closs: the patch term needs P <= 8 patches of n rays inside the batch (P={P}, n={self.n}, B={B})")
        coins = None if self.ss_coins is None else tuple(int(bool(c)) for c in self.ss_coins)
        if coins is not None and (len(coins) != 4 or P > 0 or self.counts is not None or m is None):
            raise CnerfError("closs: ss_coins takes 4 draws, a selection mask, no patch term and no global counts")
        seg = int(self.seg_row)
        if seg and (coins is None or seg % 8 != 0 or not 0 < seg < B):
            raise CnerfError(f"closs: seg_row {seg} needs ss_coins, a multiple of 8 and 0 < seg_row < B = {B}")
        sP = int(self.ssim_P) if float(self.ssim_w) != 0.0 else 0
        if sP > 0 and (sP > 8 or sP * PATCH_SSIM_RAYS > B or coins is not None):
            raise CnerfError(f"closs: the patch SSIM term needs ssim_P <= 8 patches of {PATCH_SSIM_RAYS} rays inside the batch and no "
                             f"ss_coins (ssim_P={sP}, B={B})")
        rf, df = int(self.rgb_form), int(self.depth_form) if pr is not None else 0
        lP = int(self.lpips_P) if float(self.lpips_w) != 0.0 else 0
        if lP > 0 and (lP > 8 or lP * PATCH_SSIM_RAYS > B or coins is not None or rf or df or self.lpips_packed is None):
            raise CnerfError(f"closs: the patch LPIPS term needs lpips_P <= 8 patches of {PATCH_SSIM_RAYS} rays inside the batch, the packed "
                             f"network, the default loss forms and no ss_coins (lpips_P={lP}, B={B})")
        temps = None
        if rf or df:
            if not (0 <= rf < len(RGB_FORMS) and 0 <= df < len(DEPTH_FORMS)):
                raise CnerfError(f"closs: unknown loss form ({rf}, {df})")
            if coins is not None or (self.counts is not None and (rf or df >= DEPTH_FORMS.index("softlp"))):
                raise CnerfError("closs: a loss form takes no ss_coins, and no global counts with a softlp / softmask form")
            if (rf == RGB_FORMS.index("softlp") or df == DEPTH_FORMS.index("softlp")) and not float(self.lp_coef) > 0:
                raise CnerfError("closs: a softlp form needs lp_coef > 0")
            temps = tuple(None if x is None else _chk(x.reshape(1), "temp") for x in (self.temps or (None,) * 4))
            need = [k for k in (0, 2) if rf == RGB_FORMS.index("softmask")] + [k for k in (1, 3) if df == DEPTH_FORMS.index("softmask")]
            if len(temps) != 4 or any(temps[k] is None for k in need):
                raise CnerfError("closs: a softmask form needs its temperature of both levels as device tensors")
        return dataclasses.replace(
            self, target=t, mask=m, prior=pr, far=float(self.far), coef=float(self.coef), rgb_w=float(self.rgb_w), depth_w=float(self.depth_w),
            patch_w=float(self.patch_w), mono=mono, P=P, n=int(self.n), counts=_chk(self.counts, "counts"), ss_coins=coins, seg_row=seg,
            counts3=_chk(self.counts3, "counts3") if seg else None, ssim_w=float(self.ssim_w) if sP else 0.0, ssim_P=sP, rgb_form=rf,
            depth_form=df, lp_coef=float(self.lp_coef), temps=temps, lpips_w=float(self.lpips_w) if lP else 0.0, lpips_P=lP,
            lpips_packed=_chk(self.lpips_packed, "lpips_packed") if lP else None)


def _closs_args(L: ClossSpec, level: int):
    """struct cnerf_closs of the batch (+ struct cnerf_lossform of the level with a loss form), by reference."""
    return [C.byref(L.c())] + ([C.byref(L.form_c(level))] if L.forms else [])


def composite_forward_closs(raw: Tensor, z: Tensor, rays: Tensor, noise: Optional[Tensor], white_bkgd: bool, L: ClossSpec,
                            level: int = 0):
    """-> (rgb, disp, acc, weights, depth, ws): raw2outputs + the level's five masked-loss partial sums per workgroup in `ws` (with
    a loss form, L.forms: cnerf_composite_fwd_lossform's ten; level 0 = the last level, 1 = coarse: whose temperatures to read)."""
    raw, B, S, pre, _keep = _composite_args(raw, z, rays, noise, white_bkgd)
    rgb, disp, acc, depth, weights = outs = _composite_outputs(B, S, raw.device)
    lib = _lib.load()
    name, floats = ("cnerf_composite_fwd_lossform", lib.cnerf_lossform_ws_floats) if L.forms else ("cnerf_composite_fwd_closs",
                                                                                                   lib.cnerf_closs_ws_floats)
    ws = torch.empty(floats(B) // 2, device=raw.device, dtype=torch.float64)
    _lib.check(getattr(lib, name)(*pre, *_closs_args(L, level), *map(_p, outs), _p(ws), _stream()), name)
    return rgb, disp, acc, weights, depth, ws


class ClossFinish(NamedTuple):
    """What the loss tail of a step leaves (closs_finish); None where the step has no such term.  The sizes per mode:
    terms [8] = loss, then (img, depth, patch) of the last level and of the coarse one, -; [10] with the SSIM term or a loss form
            (+ ssim_level per level); [12] with the LPIPS term (+ lpips_level per level) or L.seg_row (+ the second render's four terms)
    stats   per level the 4 seed weights (w1, w0, wd, wd0: 0 but for a loss form) of the compositing backward; per level 8 with
            L.seg_row ([2 segments][4]) or a loss form (+ 1 / the colour form's normaliser, 3 unused): [8] or [16] floats, both
            levels' room whatever `levels` is"""
    terms: Tensor
    stats: Tensor
    patch_d: Optional[Tensor]     # [levels, P * n]
    ssim_d: Optional[Tensor]      # [levels, ssim_P * 768]
    d_temp: Optional[Tensor]      # [4] = per level (rgb_w dL_rgb / d temp_rgb, depth_w dL_depth / d temp_depth): loss forms only


def lpips_step_forward(L: ClossSpec, B: int, rgb_last: Tensor, rgb_coarse: Optional[Tensor], want_grad: bool = True):
    """The LPIPS forward of the folded step (L.lpips_P > 0) -> (value [levels * lpips_P], kept workspace | None): cnerf_lpips_pack_patches
    writes the patch rays of every level as one batch (the last level's patches first), ONE lpips_forward over it; the values go to
    closs_finish(lpips_v=), the workspace (want_grad) to lpips_step_backward."""
    rgb_last, rgb_coarse = _chk(rgb_last, "rgb"), _chk(rgb_coarse, "rgb0")
    n = (2 if rgb_coarse is not None else 1) * L.lpips_P
    pred, gt = torch.empty(n, 3, 16, 16, device=rgb_last.device), torch.empty(n, 3, 16, 16, device=rgb_last.device)
    _lib.check(_lib.load().cnerf_lpips_pack_patches(_p(rgb_last), _p(rgb_coarse), _p(L.target), int(L.lpips_P), int(B), _p(pred), _p(gt),
                                                    _stream()), "cnerf_lpips_pack_patches")
    value, _, ws, _ = lpips_forward(pred, gt, L.lpips_packed, keep=want_grad)
    return value, ws


def closs_finish(L: ClossSpec, B: int, ws_last: Tensor, ws_coarse: Optional[Tensor], depth_last: Optional[Tensor],
                 depth_coarse: Optional[Tensor], rgb_last: Optional[Tensor] = None, rgb_coarse: Optional[Tensor] = None,
                 want_grad: bool = True, lpips_v: Optional[Tensor] = None) -> ClossFinish:
    """The loss tail of a step whose masked losses rode in the compositing launches, through the entry point L asks for:
    cnerf_lossform_finish (L.forms), cnerf_closs_finish_lpips (L.lpips_P > 0: V's patch LPIPS term of every level from lpips_v, the
    per-image values of lpips_step_forward — with or without the SSIM term),
    cnerf_closs_finish_ssim (L.ssim_P > 0: V's patch SSIM term of every level, from the levels' colour maps), cnerf_closs_finish_ss2 / _ss (L.ss_coins with / without L.seg_row: the in-loop consistency step as one render /
    its primary terms), else cnerf_closs_finish."""
    dev = ws_last.device
    levels = 2 if ws_coarse is not None else 1
    extra = L.forms or L.ssim_P > 0 or L.lpips_P > 0
    terms = torch.empty(12 if (L.seg_row or L.lpips_P > 0) else 10 if extra else 8, device=dev)
    stats = torch.empty(16 if (L.seg_row or L.forms) else 8, device=dev)
    patch_d = torch.empty(levels, L.P * L.n, device=dev) if (L.P > 0 and want_grad) else None
    ssim_d = torch.empty(levels, L.ssim_P * PATCH_SSIM_RAYS * 3, device=dev) if (L.ssim_P > 0 and want_grad) else None
    d_temp = torch.empty(4, device=dev) if L.forms else None
    t = ClossTail(_addr(ws_last), _addr(ws_coarse), int(B), _addr(L.counts), L.coef, L.far, L.rgb_w, L.depth_w, L.patch_w,
                  int(L.prior is not None), _addr(depth_last) if L.P > 0 else None,
                  _addr(depth_coarse) if (L.P > 0 and levels == 2) else None, _addr(L.mono) if L.P > 0 else None, L.P, L.n)
    if extra:
        rgb_last, rgb_coarse = _chk(rgb_last, "rgb"), _chk(rgb_coarse, "rgb0") if levels == 2 else None
    # the argument groups the six entry points share, then (symbol, what follows the tail struct) by what L asks for
    outs, grads = [_p(terms), _p(stats)], [_p(patch_d), _p(ssim_d)]
    ssim = [int(L.ssim_P), float(L.ssim_w), _p(rgb_last), _p(rgb_coarse), _p(L.target)]
    if L.lpips_P > 0:
        if lpips_v is None or lpips_v.numel() != levels * L.lpips_P:
            raise CnerfError(f"closs_finish: the LPIPS term needs lpips_v [{levels * L.lpips_P}] (lpips_step_forward)")
        lpips_v = _chk(lpips_v, "lpips_v")
        name, args = "cnerf_closs_finish_lpips", [*ssim, int(L.lpips_P), float(L.lpips_w), _p(lpips_v), *outs, *grads]
    elif L.forms:
        f0, f1 = L.form_c(0), L.form_c(1)
        name, args = "cnerf_lossform_finish", [C.byref(f0), C.byref(f1), *ssim, *outs, *grads, _p(d_temp)]
    elif L.ssim_P > 0:
        name, args = "cnerf_closs_finish_ssim", [*ssim, *outs, *grads]
    elif L.ss_coins is not None:
        coins = (C.c_int32 * 4)(*L.ss_coins)
        name, args = ("cnerf_closs_finish_ss2", [coins, int(L.seg_row), _p(L.counts3), *outs]) if L.seg_row else ("cnerf_closs_finish_ss",
                                                                                                                 [coins, *outs])
    else:
        name, args = "cnerf_closs_finish", [*outs, _p(patch_d)]
    _lib.check(getattr(_lib.load(), name)(C.byref(t), *args, _stream()), name)
    return ClossFinish(terms, stats, patch_d, ssim_d, d_temp)


lossform_finish = closs_finish    # (the name callers of the loss-form launches use: with L.forms the call above IS cnerf_lossform_finish)


def lpips_step_backward(L: ClossSpec, lpips_ws: Tensor, levels: int, g_loss: Tensor) -> Tensor:
    """The LPIPS backward of the folded step -> dX [levels * lpips_P, 3, 16, 16]: cnerf_lpips_seeds forms the per-image seeds
    (g_loss lpips_w) / 4 on the device, ONE lpips_backward over the kept workspace of lpips_step_forward."""
    n = levels * L.lpips_P
    seeds = torch.empty(n, device=lpips_ws.device)
    _lib.check(_lib.load().cnerf_lpips_seeds(_p(_chk(g_loss.reshape(1), "g_loss")), float(L.lpips_w), n, _p(seeds), _stream()),
               "cnerf_lpips_seeds")
    return lpips_backward(L.lpips_packed, lpips_ws, seeds, (n, 3, 16, 16))


def composite_backward_closs(raw, z, rays, noise, white_bkgd, L: ClossSpec, rgb, depth, stats4, g_loss, patch_d, ssim_d=None,
                             level: int = 0, d_temp2=None, g_temp2=None, lpips_dx=None) -> Tensor:
    raw, _, _, pre, _keep = _composite_args(raw, z, rays, noise, white_bkgd)
    d_raw = torch.empty_like(raw)
    lpips_dx = _chk(lpips_dx, "lpips_dx")
    # what the four entry points take alike, then (symbol, what follows the weights); stats4 = the level's 4 floats, 8 with a loss
    # form, which also puts its struct after the batch's (_closs_args)
    args = [*pre, *_closs_args(L, level), _p(rgb), _p(depth), _p(stats4), _p(g_loss), L.rgb_w, L.depth_w, L.patch_w]
    patch = [_p(patch_d), L.P * L.n if patch_d is not None else 0]
    ssim = [float(L.ssim_w), _p(ssim_d), 0 if ssim_d is None else ssim_d.numel() // 3]      # V's patch SSIM seeds
    if L.forms:
        name, tail = "cnerf_composite_bwd_lossform", [L.coef, *patch, *ssim, _p(d_temp2), _p(g_temp2)]
    elif lpips_dx is not None:  # + V's patch LPIPS seeds, the level's [lpips_P, 3, 16, 16] slice of the gradient (+ the SSIM seeds)
        name, tail = "cnerf_composite_bwd_closs_lpips", [*patch, *ssim, _p(lpips_dx), lpips_dx.shape[0] * PATCH_SSIM_RAYS]
    elif ssim_d is not None:
        name, tail = "cnerf_composite_bwd_closs_ssim", [*patch, *ssim]
    else:
        name, tail = "cnerf_composite_bwd_closs", patch
    _lib.check(getattr(_lib.load(), name)(*args, *tail, _p(d_raw), _stream()), name)
    return d_raw


def composite_backward(raw, z, rays, noise, white_bkgd, g_rgb, g_disp, g_acc, g_depth) -> Tensor:
    raw, _, _, pre, _keep = _composite_args(raw, z, rays, noise, white_bkgd)
    grads = [_chk(g, "grad") for g in (g_rgb, g_disp, g_acc, g_depth)]
    d_raw = torch.empty_like(raw)
    _lib.check(_lib.load().cnerf_composite_bwd(*pre, *map(_p, grads), _p(d_raw), _stream()), "cnerf_composite_bwd")
    return d_raw


# ------------------------------------------------------------------------------------------ rays
def _f4(a) -> "C.Array":
    """The top 3 x 4 of a pose (host array, or a tensor: ONE device-to-host copy) as float[12]."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)[:3, :4]).reshape(-1)
    return (C.c_float * 12)(*a.tolist())


def _intrinsics(K):
    """(fx, fy, cx, cy) of a 3 x 3 camera matrix."""
    return float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])


def gen_rays(H: int, W: int, K, c2w, near: float, far: float, use_viewdirs: bool, ndc: bool, device,
             ndc_coef=(0.0, 0.0)) -> Tensor:
    rays = torch.empty(H * W, 11 if use_viewdirs else 8, device=device, dtype=torch.float32)
    _lib.check(_lib.load().cnerf_gen_rays(H, W, *_intrinsics(K), _f4(c2w), float(near), float(far), int(use_viewdirs), int(ndc),
                                          float(ndc_coef[0]), float(ndc_coef[1]), _p(rays), _stream()), "cnerf_gen_rays")
    return rays


def pack_rays(rays_o: Tensor, rays_d: Tensor, near: float, far: float, use_viewdirs: bool, ndc: bool,
              ndc_coef=(0.0, 0.0)) -> Tensor:
    rays_o, rays_d = _chk(rays_o.reshape(-1, 3), "rays_o"), _chk(rays_d.reshape(-1, 3), "rays_d")
    B = rays_o.shape[0]
    rays = torch.empty(B, 11 if use_viewdirs else 8, device=rays_o.device, dtype=torch.float32)
    _lib.check(_lib.load().cnerf_pack_rays(_p(rays_o), _p(rays_d), B, float(near), float(far), int(use_viewdirs),
                                           int(ndc), float(ndc_coef[0]), float(ndc_coef[1]), _p(rays), _stream()),
               "cnerf_pack_rays")
    return rays


def pack_rays_bwd(g: Tensor, rays_d: Tensor, use_viewdirs: bool):
    """cnerf_pack_rays_bwd: the gradient of the non-NDC pack_rays rows g [B, 8 | 11] -> (d_rays_o [B, 3], d_rays_d [B, 3])."""
    g, rays_d = _chk(g, "g"), _chk(rays_d.reshape(-1, 3), "rays_d")
    B = rays_d.shape[0]
    if g.shape != (B, 11 if use_viewdirs else 8):
        raise CnerfError(f"pack_rays_bwd: g is {tuple(g.shape)}, the pack has {(B, 11 if use_viewdirs else 8)}")
    d_o, d_d = torch.empty_like(rays_d), torch.empty_like(rays_d)
    if B > 0:
        _lib.check(_lib.load().cnerf_pack_rays_bwd(_p(g), _p(rays_d), B, int(use_viewdirs), _p(d_o), _p(d_d), _stream()),
                   "cnerf_pack_rays_bwd")
    return d_o, d_d


def _rays_at_args(who: str, H: int, W: int, n_views: int, coords: Optional[Tensor], view: Optional[Tensor], first: int, B: Optional[int]):
    """(coords, view, B) of a cnerf_gen_rays_at[_bwd] call: int64 device tensors or None, B from coords / view / the caller.  The VALUES
    of coords and view are not checked (a check would be a device-to-host sync): in range is the caller's duty, as for select_inds."""
    coords, view = _chk(coords, "coords", dtype=torch.int64), _chk(view, "view", dtype=torch.int64)
    if coords is not None:
        if coords.dim() != 2 or coords.shape[1] != 2:
            raise CnerfError(f"{who}: coords must be [B, 2] (row, col), got {tuple(coords.shape)}")
        if B is not None and B != coords.shape[0]:
            raise CnerfError(f"{who}: B = {B} but coords has {coords.shape[0]} rows")
        B = coords.shape[0]
    elif B is None:
        B = H * W - first if view is None else view.numel()
    if view is not None and tuple(view.shape) != (B,):
        raise CnerfError(f"{who}: view must be [{B}], got {tuple(view.shape)}")
    if B <= 0 or n_views <= 0 or (coords is None and (first < 0 or first + B > H * W)):
        raise CnerfError(f"{who}: B = {B}, n_views = {n_views}, first = {first} on a {H} x {W} image")
    return coords, view, B


def gen_rays_at(H: int, W: int, K, c2w: Tensor, coords: Optional[Tensor] = None, view: Optional[Tensor] = None, first: int = 0,
                B: Optional[int] = None):
    """cnerf_gen_rays_at: (rays_o [B, 3], rays_d [B, 3]) of H:164-173 from poses c2w [n_views, 12] (row-major 3 x 4 each) that stay
    in device memory.  coords: int64 [B, 2] = (row, col), or None: the B row-major pixels from `first` on; view: int64 [B] or None
    (view 0)."""
    c2w = _chk(c2w, "c2w")
    if c2w.dim() != 2 or c2w.shape[1] != 12:
        raise CnerfError(f"gen_rays_at: c2w must be [n_views, 12], got {tuple(c2w.shape)}")
    coords, view, B = _rays_at_args("gen_rays_at", H, W, c2w.shape[0], coords, view, first, B)
    o, d = torch.empty(B, 3, device=c2w.device), torch.empty(B, 3, device=c2w.device)
    _lib.check(_lib.load().cnerf_gen_rays_at(H, W, *_intrinsics(K), _p(c2w), c2w.shape[0], _p(coords), _p(view), first, B, _p(o), _p(d),
                                             _stream()), "cnerf_gen_rays_at")
    return o, d


def gen_rays_at_bwd(d_rays_o: Tensor, d_rays_d: Tensor, H: int, W: int, K, n_views: int, coords: Optional[Tensor] = None,
                    view: Optional[Tensor] = None, first: int = 0, grid: int = 0) -> Tensor:
    """cnerf_gen_rays_at_bwd: d_c2w [n_views, 12] from (d_rays_o, d_rays_d) [B, 3] of the gen_rays_at call with the same coords, view
    and first.  The same bits call after call and for every `grid` (workgroups of the first launch, 0 = chosen by the library)."""
    d_o, d_d = _chk(d_rays_o.reshape(-1, 3), "d_rays_o"), _chk(d_rays_d.reshape(-1, 3), "d_rays_d")
    if d_o.shape != d_d.shape:
        raise CnerfError(f"gen_rays_at_bwd: d_rays_o is {tuple(d_o.shape)}, d_rays_d {tuple(d_d.shape)}")
    coords, view, B = _rays_at_args("gen_rays_at_bwd", H, W, n_views, coords, view, first, d_o.shape[0])
    lib = _lib.load()
    ws = torch.empty(lib.cnerf_gen_rays_at_bwd_ws_floats(B, n_views) // 2, device=d_o.device, dtype=torch.float64)
    d_c2w = torch.empty(n_views, 12, device=d_o.device)
    _lib.check(lib.cnerf_gen_rays_at_bwd(H, W, *_intrinsics(K), _p(d_o), _p(d_d), n_views, _p(coords), _p(view), first, B, _p(d_c2w),
                                         _p(ws), int(grid), _stream()), "cnerf_gen_rays_at_bwd")
    return d_c2w


def _pose_args(who: str, c2w0: Tensor, rot: Tensor, more: Tensor, more_name: str, more_cols: int):
    c2w0, rot, more = _chk(c2w0, "c2w0"), _chk(rot, "rot"), _chk(more, more_name)
    N = rot.shape[0] if rot.dim() == 2 else -1
    if N <= 0 or rot.shape[1] != 3 or c2w0.numel() != N * 12 or more.numel() != N * more_cols:
        raise CnerfError(f"{who}: c2w0 {tuple(c2w0.shape)}, rot {tuple(rot.shape)}, {more_name} {tuple(more.shape)} are not "
                         f"[N, 3, 4], [N, 3], [N, {more_cols}]")
    return c2w0, rot, more, N


def pose_compose(c2w0: Tensor, rot: Tensor, trans: Tensor) -> Tensor:
    """cnerf_pose_compose: c2w [N, 3, 4] = [Exp(rot[n]) R0_n | t0_n + trans[n]] from c2w0 [N, 3, 4], rot (axis-angle) and trans [N, 3]."""
    c2w0, rot, trans, N = _pose_args("pose_compose", c2w0, rot, trans, "trans", 3)
    c2w = torch.empty(N, 3, 4, device=rot.device)
    _lib.check(_lib.load().cnerf_pose_compose(_p(c2w0), _p(rot), _p(trans), N, _p(c2w), _stream()), "cnerf_pose_compose")
    return c2w


def pose_compose_bwd(c2w0: Tensor, rot: Tensor, d_c2w: Tensor, want_rot: bool = True, want_trans: bool = True):
    """cnerf_pose_compose_bwd: d_c2w [N, 3, 4] (or [N, 12]) -> (d_rot [N, 3] | None, d_trans [N, 3] | None)."""
    c2w0, rot, d_c2w, N = _pose_args("pose_compose_bwd", c2w0, rot, d_c2w, "d_c2w", 12)
    if not (want_rot or want_trans):
        return None, None
    d_rot = torch.empty(N, 3, device=rot.device) if want_rot else None
    d_trans = torch.empty(N, 3, device=rot.device) if want_trans else None
    _lib.check(_lib.load().cnerf_pose_compose_bwd(_p(c2w0), _p(rot), _p(d_c2w), N, _p(d_rot), _p(d_trans), _stream()),
               "cnerf_pose_compose_bwd")
    return d_rot, d_trans


def _camera_intrinsics(who: str, K, ndc_coef):
    """(fx, fy, cx, cy, ax, ay, K_dev) of a cnerf_camera_rows[_bwd] call.  A float32 [3, 3] tensor on the GPU is handed over as a
    pointer and read in the kernel (no copy to the host; the six floats are placeholders it overrides); anything else is a host
    3 x 3 whose floats go in, with the two NDC coefficients the caller formed."""
    if torch.is_tensor(K) and K.is_cuda:
        if K.dtype != torch.float32 or tuple(K.shape) != (3, 3):
            raise CnerfError(f"{who}: a device K must be float32 [3, 3], got {K.dtype} {tuple(K.shape)}")
        return (1.0, 1.0, 0.0, 0.0, 0.0, 0.0), K.detach().contiguous()
    return _intrinsics(K) + (float(ndc_coef[0]), float(ndc_coef[1])), None


def _camera_c2w(who: str, c2w: Tensor) -> Tensor:
    c2w = _chk(c2w, "c2w")
    if c2w.dim() != 2 or c2w.shape[1] != 12:
        raise CnerfError(f"{who}: c2w must be [n_views, 12], got {tuple(c2w.shape)}")
    return c2w


def camera_rows(H: int, W: int, K, c2w: Tensor, coords: Optional[Tensor] = None, view: Optional[Tensor] = None, near: float = 0.,
                far: float = 1., use_viewdirs: bool = False, ndc: bool = True, ndc_coef=(0.0, 0.0), first: int = 0,
                B: Optional[int] = None) -> Tensor:
    """cnerf_camera_rows: the finished rows [B, 8 | 11] = [o, d, near, far (, viewdirs)] of render()'s batch (H:164-173, R:103-116,
    H:186-202) in one launch, from poses c2w [n_views, 12] in device memory; coords / view / first / B as gen_rays_at.  K: a host
    3 x 3 (with ndc_coef = the two coefficients of H:193-199), or a float32 [3, 3] tensor on the GPU, read there (ndc_coef is then
    ignored: the kernel forms the coefficients from K[0][0])."""
    c2w = _camera_c2w("camera_rows", c2w)
    coords, view, B = _rays_at_args("camera_rows", H, W, c2w.shape[0], coords, view, first, B)
    intr, K_dev = _camera_intrinsics("camera_rows", K, ndc_coef)
    rows = torch.empty(B, 11 if use_viewdirs else 8, device=c2w.device)
    _lib.check(_lib.load().cnerf_camera_rows(H, W, *intr, _p(K_dev), _p(c2w), c2w.shape[0], _p(coords), _p(view), first, B, float(near),
                                             float(far), int(use_viewdirs), int(ndc), _p(rows), _stream()), "cnerf_camera_rows")
    return rows


def camera_rows_bwd(g: Tensor, H: int, W: int, K, c2w: Tensor, coords: Optional[Tensor] = None, view: Optional[Tensor] = None,
                    use_viewdirs: bool = False, ndc: bool = True, ndc_coef=(0.0, 0.0), first: int = 0, want_c2w: bool = True,
                    want_K: bool = True, grid: int = 0):
    """cnerf_camera_rows_bwd: the row gradient g [B, 8 | 11] of the camera_rows call with the same arguments -> (d_c2w [n_views, 12]
    | None, d_K [3, 3] | None).  The same bits call after call and for every `grid` (workgroups of the first launch, 0 = chosen by
    the library)."""
    c2w, g = _camera_c2w("camera_rows_bwd", c2w), _chk(g, "g")
    cols = 11 if use_viewdirs else 8
    if g.dim() != 2 or g.shape[1] != cols:
        raise CnerfError(f"camera_rows_bwd: g must be [B, {cols}], got {tuple(g.shape)}")
    n_views = c2w.shape[0]
    coords, view, B = _rays_at_args("camera_rows_bwd", H, W, n_views, coords, view, first, g.shape[0])
    if not (want_c2w or want_K):
        return None, None
    intr, K_dev = _camera_intrinsics("camera_rows_bwd", K, ndc_coef)
    lib = _lib.load()
    ws = torch.empty(lib.cnerf_camera_rows_bwd_ws_floats(B, n_views) // 2, device=g.device, dtype=torch.float64)
    d_c2w = torch.empty(n_views, 12, device=g.device) if want_c2w else None
    d_K = torch.empty(3, 3, device=g.device) if want_K else None
    _lib.check(lib.cnerf_camera_rows_bwd(H, W, *intr, _p(K_dev), _p(c2w), n_views, _p(coords), _p(view), first, B, int(use_viewdirs),
                                         int(ndc), _p(g), _p(d_c2w), _p(d_K), _p(ws), int(grid), _stream()), "cnerf_camera_rows_bwd")
    return d_c2w, d_K


def ndc_rays_bwd(g_o: Tensor, g_d: Tensor, rays_o: Tensor, rays_d: Tensor, ndc_coef):
    """cnerf_ndc_rays_bwd: the gradients (g_o, g_d) [B, 3] of ndc_rays' outputs and its inputs (rays_o, rays_d) [B, 3] ->
    (d_rays_o, d_rays_d) [B, 3]."""
    ts = [_chk(t.reshape(-1, 3), n) for t, n in ((g_o, "g_o"), (g_d, "g_d"), (rays_o, "rays_o"), (rays_d, "rays_d"))]
    B = ts[0].shape[0]
    if B <= 0 or any(t.shape[0] != B for t in ts):
        raise CnerfError(f"ndc_rays_bwd: g_o, g_d, rays_o, rays_d are {[tuple(t.shape) for t in ts]}, not four [B, 3] with B > 0")
    d_o, d_d = torch.empty_like(ts[2]), torch.empty_like(ts[3])
    _lib.check(_lib.load().cnerf_ndc_rays_bwd(*map(_p, ts), B, float(ndc_coef[0]), float(ndc_coef[1]), _p(d_o), _p(d_d), _stream()),
               "cnerf_ndc_rays_bwd")
    return d_o, d_d


def sample_pixels(H: int, W: int, K, c2w, near: float, far: float, use_viewdirs: bool, ndc: bool, ndc_coef, crop, patch_starts,
                  patch_size: int, n_rand: int, select_inds: Optional[Tensor], rng: Optional[RngStream], image: Tensor,
                  extras: Sequence[Tensor] = (), want_rows: bool = True, want_od: bool = True, want_coords: bool = True):
    """cnerf_sample_pixels: the training batch of one image in one launch -> (rays [B, 8|11] | None, rays_od [2, B, 3] | None,
    target [B, 3], extras_out [n_extras, B], coords [B, 2] | None).  crop = (r0, c0, h, w) of the grid the random pixels come
    from; patch_starts [P, 2] host integers (or None); select_inds: device int64 [n_rand] or None (device draw keyed by rng)."""
    image = _chk(image, "image")
    if image.dim() != 3 or image.shape[0] != H or image.shape[1] != W or image.shape[2] < 3:
        raise CnerfError(f"sample_pixels: image must be [{H}, {W}, >=3], got {tuple(image.shape)}")
    dev = image.device
    ex = [_chk(e, "extra") for e in extras]
    for e in ex:
        if tuple(e.shape) != (H, W):
            raise CnerfError(f"sample_pixels: per-pixel maps must be [{H}, {W}], got {tuple(e.shape)}")
    starts = np.zeros((0, 2), np.int64) if patch_starts is None else np.asarray(patch_starts, np.int64).reshape(-1, 2)
    P = starts.shape[0]
    cfg = PixelBatch()
    cfg.H, cfg.W, (cfg.fx, cfg.fy, cfg.cx, cfg.cy) = H, W, _intrinsics(K)
    cfg.c2w = _f4(c2w)
    cfg.near, cfg.far, cfg.use_viewdirs, cfg.ndc = float(near), float(far), int(use_viewdirs), int(ndc)
    cfg.ndc_ax, cfg.ndc_ay = float(ndc_coef[0]), float(ndc_coef[1])
    cfg.crop_r0, cfg.crop_c0, cfg.crop_h, cfg.crop_w = (int(v) for v in crop)
    cfg.n_patches, cfg.patch_size = P, int(patch_size)
    for q in range(P):
        cfg.patch_start[q][0], cfg.patch_start[q][1] = int(starts[q, 0]), int(starts[q, 1])
    cfg.n_rand, cfg.image_ch, cfg.n_extras = int(n_rand), int(image.shape[2]), len(ex)
    B = P * patch_size * patch_size + int(n_rand)
    if select_inds is not None:
        select_inds = _chk(select_inds, "select_inds", dtype=torch.int64)
        if select_inds.numel() != n_rand:
            raise CnerfError(f"sample_pixels: select_inds must have {n_rand} elements")
    rows = torch.empty(B, 11 if use_viewdirs else 8, device=dev) if want_rows else None
    od = torch.empty(2, B, 3, device=dev) if want_od else None
    target = torch.empty(B, 3, device=dev)
    ex_out = torch.empty(len(ex), B, device=dev) if ex else None
    coords = torch.empty(B, 2, device=dev, dtype=torch.int64) if want_coords else None
    ptrs = (C.c_void_p * max(1, len(ex)))(*[e.data_ptr() for e in ex])
    r = rng.c(0) if (rng is not None and select_inds is None) else None
    _lib.check(_lib.load().cnerf_sample_pixels(C.byref(cfg), _p(select_inds), C.byref(r) if r is not None else None, _p(image), ptrs,
                                               _p(rows), _p(od), _p(target), _p(ex_out), _p(coords), _stream()),
               "cnerf_sample_pixels")
    return rows, od, target, ex_out, coords


# ------------------------------------------------------------------------------------------ warp / masks
def warp_points(P: Tensor, w2c, K, H: int, W: int, flip: bool):
    P = _chk(P.reshape(-1, 3), "P")
    N = P.shape[0]
    dev = P.device
    Xc = torch.empty(N, 3, device=dev)
    px, py = torch.empty(N, device=dev), torch.empty(N, device=dev)
    inb = torch.empty(N, device=dev, dtype=torch.uint8)
    _lib.check(_lib.load().cnerf_warp_points(_p(P), N, _f4(w2c), *_intrinsics(K), H, W, int(flip), _p(Xc), _p(px), _p(py), _p(inb),
                                             _stream()), "cnerf_warp_points")
    return Xc, px, py, inb.bool()

_PINNED_META = {}


def _pinned_meta(dev):
    """A small ring of pinned int32[8] buffers per device (pinned allocations cost ~100 us each: never per step)."""
    ring = _PINNED_META.get(dev.index)
    if ring is None:
        ring = _PINNED_META[dev.index] = [[torch.empty(8, dtype=torch.int32).pin_memory() for _ in range(8)], 0]
    ring[1] = (ring[1] + 1) % len(ring[0])
    return ring[0][ring[1]]


def ss_ref_rays(rays_o: Tensor, rays_d: Tensor, depth: Tensor, w2c_ref, c2w_ref, K, H: int, W: int, image: Tensor, depth_ref: Tensor,
                thr0: float, near: float, far: float, use_viewdirs: bool, ndc: bool, ndc_coef=(0.0, 0.0), flip: bool = False,
                want_rows: bool = True):
    """cnerf_ss_ref_rays (VT:905-925): one launch + ONE 32-byte read-back (the ray count M of the second render; the reference
    synchronises at every boolean index and every threshold doubling) -> dict(M, k, thr (python float), rows [M, 8|11] | None,
    rays_od [2, M, 3] (views of a [2, N, 3] buffer), target [M, 3], depth_tgt [M], depth_diff [M], inb [N] uint8, mask [M] uint8,
    sel [N] float, rank [N] int32).  image [H, W, >=3] and depth_ref [H, W] live on the device; w2c_ref / c2w_ref are host 3x4|4x4."""
    rays_o, rays_d, depth = _chk(rays_o.reshape(-1, 3), "rays_o"), _chk(rays_d.reshape(-1, 3), "rays_d"), _chk(depth.reshape(-1), "depth")
    image, depth_ref = _chk(image, "image"), _chk(depth_ref, "depth_ref")
    N, dev = rays_o.shape[0], rays_o.device
    _ss_check("ss_ref_rays", H, W, image, depth_ref, rays_d=rays_d, depth=depth, rays_o=rays_o)
    cfg = _ss_cfg(w2c_ref, c2w_ref, K, H, W, image, thr0, near, far, use_viewdirs, ndc, ndc_coef, flip)
    rows = torch.empty(N, 11 if use_viewdirs else 8, device=dev) if want_rows else None
    od = torch.empty(2, N, 3, device=dev)
    target, dtgt, diff = torch.empty(N, 3, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    inb, mask = torch.empty(N, device=dev, dtype=torch.uint8), torch.empty(N, device=dev, dtype=torch.uint8)
    sel, rank = torch.empty(N, device=dev), torch.empty(N, device=dev, dtype=torch.int32)
    meta = torch.empty(8, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().cnerf_ss_ref_rays(C.byref(cfg), _p(rays_o), _p(rays_d), _p(depth), N, _p(image), _p(depth_ref), _p(rows),
                                             _p(od), _p(target), _p(dtgt), _p(diff), _p(inb), _p(mask), _p(sel), _p(rank), _p(meta),
                                             _stream()), "cnerf_ss_ref_rays")
    host = _pinned_meta(dev)
    host.copy_(meta, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    ev.synchronize()                      # the ONE host wait of the block: the second render's launch dimensions need M
    M, k = int(host[0]), int(host[1])
    thr = float(np.int32(int(host[2])).view(np.float32))
    return dict(M=M, k=k, thr=thr, rows=None if rows is None else rows[:M], rays_od=od[:, :M], target=target[:M], depth_tgt=dtgt[:M],
                depth_diff=diff[:M], inb=inb, mask=mask[:M], sel=sel, rank=rank)


def _ss_check(who, H, W, image, depth_ref, rays_o, **per_ray):
    """The shape rules ss_ref_rays and ss_batch share: the reference view's image and depth, one non-empty batch."""
    if image.dim() != 3 or image.shape[0] != H or image.shape[1] != W or image.shape[2] < 3 or depth_ref.numel() != H * W:
        raise CnerfError(f"{who}: image must be [{H}, {W}, >=3] and depth_ref [{H}, {W}]")
    N = rays_o.shape[0]
    if N == 0 or any(t.shape[0] != N for t in per_ray.values()):
        raise CnerfError(f"{who}: {' / '.join(['rays_o', *per_ray])} must describe the same (non-empty) batch")


def _ss_cfg(w2c_ref, c2w_ref, K, H, W, image, thr0, near, far, use_viewdirs, ndc, ndc_coef, flip) -> "SsWarp":
    cfg = SsWarp()
    r = cfg.ref
    r.H, r.W, (r.fx, r.fy, r.cx, r.cy) = int(H), int(W), _intrinsics(K)
    r.c2w = _f4(c2w_ref)
    r.near, r.far, r.use_viewdirs, r.ndc = float(near), float(far), int(use_viewdirs), int(ndc)
    r.ndc_ax, r.ndc_ay, r.first = float(ndc_coef[0]), float(ndc_coef[1]), 0
    cfg.w2c = _f4(w2c_ref)
    cfg.flip, cfg.image_ch, cfg.thr0 = int(flip), int(image.shape[2]), float(thr0)
    return cfg


def ss_batch(rays_o: Tensor, rays_d: Tensor, depth: Tensor, target_s: Tensor, w2c_ref, c2w_ref, K, H: int, W: int, image: Tensor,
             depth_ref: Tensor, thr0: float, near: float, far: float, use_viewdirs: bool, ndc: bool, ndc_coef=(0.0, 0.0),
             flip: bool = False, amin_global: Optional[Tensor] = None):
    """cnerf_ss_batch (VT:899-925 for the one-render step): ONE launch, NO read-back -> dict of DEVICE tensors:
    rows [2N, 8|11], target [2N, 3], prior [2N], mask [2N] (the combined batch: N primary rays | M warped rays | N - M padding),
    live int32 [1] = N + M, meta int32 [8] (M, k, bits of thr, NaN flag, bits of the local min |diff|, number of selected primary rays),
    rays_od [2, N, 3], depth_diff [N], inb [N] uint8, occ [N] uint8 (the occlusion mask over the first M), sel [N], rank [N] int32 —
    the per-M outputs keep their capacity N (the host does not know M; `ss_host_view` slices them after a synchronisation)."""
    rays_o, rays_d, depth = _chk(rays_o.reshape(-1, 3), "rays_o"), _chk(rays_d.reshape(-1, 3), "rays_d"), _chk(depth.reshape(-1), "depth")
    target_s = _chk(target_s.reshape(-1, 3), "target_s")
    image, depth_ref, amin_global = _chk(image, "image"), _chk(depth_ref, "depth_ref"), _chk(amin_global, "amin_global")
    N, dev = rays_o.shape[0], rays_o.device
    _ss_check("ss_batch", H, W, image, depth_ref, rays_d=rays_d, depth=depth, target_s=target_s, rays_o=rays_o)
    cfg = _ss_cfg(w2c_ref, c2w_ref, K, H, W, image, thr0, near, far, use_viewdirs, ndc, ndc_coef, flip)
    rows = torch.empty(2 * N, 11 if use_viewdirs else 8, device=dev)
    target, prior, mask2 = torch.empty(2 * N, 3, device=dev), torch.empty(2 * N, device=dev), torch.empty(2 * N, device=dev)
    live, meta = torch.empty(1, device=dev, dtype=torch.int32), torch.empty(8, device=dev, dtype=torch.int32)
    od, diff = torch.empty(2, N, 3, device=dev), torch.empty(N, device=dev)
    inb, occ = torch.empty(N, device=dev, dtype=torch.uint8), torch.empty(N, device=dev, dtype=torch.uint8)
    sel, rank = torch.empty(N, device=dev), torch.empty(N, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().cnerf_ss_batch(C.byref(cfg), _p(rays_o), _p(rays_d), _p(depth), _p(target_s), N, _p(image), _p(depth_ref),
                                          _p(amin_global), _p(rows), _p(target), _p(prior), _p(mask2), _p(live), _p(od), _p(diff),
                                          _p(inb), _p(occ), _p(sel), _p(rank), _p(meta), _stream()), "cnerf_ss_batch")
    return dict(N=N, rows=rows, target=target, prior=prior, mask=mask2, live=live, meta=meta, rays_od=od, depth_diff=diff, inb=inb,
                occ=occ, sel=sel, rank=rank)


def hard_mask_pair(H, W, K, c2w_tgt, w2c_ref, depth_tgt: Tensor, depth_ref: Tensor, thr0: float, chunk: int,
                   mask: Tensor, want_thr: bool = False):
    """cnerf_hard_mask_pair: ORs into mask (uint8 [H * W], in place) the pixels of the target view that pass against ONE reference
    view -> the per-chunk thresholds (NaN: no pixel of the chunk can pass) with want_thr, else None.  The kernel indexes all three
    buffers by pixel: their sizes are checked here."""
    depth_tgt, depth_ref = _chk(depth_tgt, "depth_tgt"), _chk(depth_ref, "depth_ref")
    H, W, chunk = int(H), int(W), int(chunk)
    if chunk <= 0:
        raise CnerfError(f"hard_mask_pair: chunk must be positive (got {chunk})")
    if depth_tgt.numel() != H * W or depth_ref.numel() != H * W or mask.numel() != H * W:
        raise CnerfError(f"hard_mask_pair: depth_tgt, depth_ref and mask must hold H * W = {H * W} elements "
                         f"(got {depth_tgt.numel()}, {depth_ref.numel()}, {mask.numel()})")
    if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.device != depth_tgt.device or depth_ref.device != depth_tgt.device:
        raise CnerfError("hard_mask_pair: mask must be a contiguous uint8 tensor on the device of the depths (it is written in place)")
    nchunks = (H * W + chunk - 1) // chunk
    thr = torch.empty(nchunks, device=mask.device) if want_thr else None
    _lib.check(_lib.load().cnerf_hard_mask_pair(H, W, *_intrinsics(K), _f4(c2w_tgt), _f4(w2c_ref), _p(depth_tgt), _p(depth_ref),
                                                float(thr0), chunk, _p(mask), _p(thr), _stream()), "cnerf_hard_mask_pair")
    return thr


# ------------------------------------------------------------------------------------------ loss / optimiser
MASKED_LOSS_SINGLE_WORKGROUP = 16384     # rays up to which cnerf_masked_loss runs as one workgroup


def masked_loss(rgb, target, depth, prior, mask, far: float, coef: float, counts=None, g_scale: float = 1.0,
                want_grads: bool = True):
    rgb, target = _chk(rgb, "rgb"), _chk(target, "target")
    depth, prior, mask, counts = _chk(depth, "depth"), _chk(prior, "prior"), _chk(mask, "mask"), _chk(counts, "counts")
    B = rgb.shape[0]
    dev = rgb.device
    loss = torch.empty(2, device=dev)
    d_rgb = torch.empty_like(rgb) if want_grads else None
    d_depth = torch.empty(B, device=dev) if (want_grads and depth is not None) else None
    lib = _lib.load()
    # beyond one workgroup's comfortable size: one workgroup per 16384 rays + a fixed-order second stage (needs the workspace)
    ws = torch.empty(lib.cnerf_loss_ws_floats() // 2, device=dev, dtype=torch.float64) if B > MASKED_LOSS_SINGLE_WORKGROUP else None
    _lib.check(lib.cnerf_masked_loss(_p(rgb), _p(target), _p(depth), _p(prior), _p(mask), B, float(far), float(coef), _p(counts),
                                     float(g_scale), _p(loss), _p(d_rgb), _p(d_depth), _p(ws), _stream()), "cnerf_masked_loss")
    return loss, d_rgb, d_depth


MSE_SINGLE_WORKGROUP = 65536    # elements up to which cnerf_mse's one workgroup is the faster form (launch-bound)


def mse(x: Tensor, y: Tensor, want_grad: bool = True):
    """cnerf_mse: (mean((x - y)^2) as a 0-d tensor, d loss / d x | None)."""
    x, y = _chk(x, "x"), _chk(y, "y")
    loss = torch.empty(1, device=x.device)
    d_x = torch.empty_like(x) if want_grad else None
    lib, n = _lib.load(), x.numel()
    if n > MSE_SINGLE_WORKGROUP:     # whole images: one workgroup per 16384 elements + a fixed-order second stage
        ws = torch.empty(lib.cnerf_mse_ws_floats(n) // 2, device=x.device, dtype=torch.float64)
        _lib.check(lib.cnerf_mse_ws(_p(x), _p(y), n, _p(loss), _p(d_x), _p(ws), _stream()), "cnerf_mse_ws")
    else:
        _lib.check(lib.cnerf_mse(_p(x), _p(y), n, _p(loss), _p(d_x), _stream()), "cnerf_mse")
    return loss[0], d_x


def soft_lp_loss(x: Tensor, y: Tensor, coef: float, want_grad: bool = True):
    """cnerf_soft_lp_loss (V:58): (sum(w d^2) / sum(w) with w = |d|^coef + 1 and a detached denominator, d loss / d x | None)."""
    x, y = _chk(x, "x"), _chk(y, "y")
    if x.shape != y.shape or x.numel() == 0:
        raise CnerfError("soft_lp_loss: x and y must be non-empty tensors of one shape")
    loss = torch.empty(1, device=x.device)
    d_x = torch.empty_like(x) if want_grad else None
    _lib.check(_lib.load().cnerf_soft_lp_loss(_p(x), _p(y), x.numel(), float(coef), _p(loss), _p(d_x), _stream()), "cnerf_soft_lp_loss")
    return loss[0], d_x


def softmask_loss(x: Tensor, y: Tensor, temp: Tensor, want_grad: bool = True):
    """cnerf_softmask_loss (V:50 / V:55): (sum(w d^2) / sum(w) with w = exp(d^2 / temp), the denominator detached in d but not in
    temp; d loss / d x | None; d loss / d temp [1] | None).  temp: a device tensor of one element."""
    x, y, temp = _chk(x, "x"), _chk(y, "y"), _chk(temp.reshape(1), "temp")
    if x.shape != y.shape or x.numel() == 0:
        raise CnerfError("softmask_loss: x and y must be non-empty tensors of one shape")
    loss = torch.empty(1, device=x.device)
    d_x = torch.empty_like(x) if want_grad else None
    d_t = torch.empty(1, device=x.device) if want_grad else None
    _lib.check(_lib.load().cnerf_softmask_loss(_p(x), _p(y), x.numel(), _p(temp), _p(loss), _p(d_x), _p(d_t), _stream()),
               "cnerf_softmask_loss")
    return loss[0], d_x, d_t


def patch_depth_loss(depth_pred: Tensor, mono: Tensor, P: int, n: int, g_scale: float = 1.0, want_grad: bool = True):
    """f-5 (V:1678-1720): (loss[1], d_depth[P*n] | None) over the first P*n rays."""
    depth_pred, mono = _chk(depth_pred, "depth_pred"), _chk(mono, "mono")
    if depth_pred.numel() < P * n or mono.numel() < P * n:
        raise CnerfError(f"patch_depth_loss: need {P}x{n} values, got {depth_pred.numel()} / {mono.numel()}")
    loss = torch.empty(1, device=depth_pred.device)
    d = torch.empty(P * n, device=depth_pred.device) if want_grad else None
    _lib.check(_lib.load().cnerf_patch_depth_loss(_p(depth_pred), _p(mono), int(P), int(n), float(g_scale), _p(loss),
                                                  _p(d), _stream()), "cnerf_patch_depth_loss")
    return loss, d


# ------------------------------------------------------------------------------------------ SSIM (pytorch-msssim 0.2.1)
PATCH_SSIM_RAYS = 256       # rays of one of V's 16 x 16 patches


def _ssim_args(X: Tensor, Y: Tensor, win_size: int):
    for t, n in ((X, "X"), (Y, "Y")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise CnerfError(f"ssim: {n} must be a float32 GPU tensor (consistentnerf_amd has no CPU path), got "
                             f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '-')}")
    if X.dim() != 4 or X.shape != Y.shape or X.numel() == 0:
        raise CnerfError(f"ssim: X and Y must be non-empty [N, C, H, W] tensors of one shape, got {tuple(X.shape)} / {tuple(Y.shape)}")
    return X.contiguous(), Y.contiguous()


def ssim_forward(X: Tensor, Y: Tensor, win_size: int, win_sigma: float, C1: float, C2: float, want_cs: bool = True):
    """cnerf_ssim_fwd: (ssim [N, C], cs [N, C] | None) = the per-channel means of the SSIM / contrast-structure maps."""
    X, Y = _ssim_args(X, Y, win_size)
    N, Cc, H, W = X.shape
    lib = _lib.load()
    ws = torch.empty(max(1, lib.cnerf_ssim_ws_floats(N, Cc, H, W, int(win_size)) // 2), device=X.device, dtype=torch.float64)
    s = torch.empty(N, Cc, device=X.device)
    cs = torch.empty(N, Cc, device=X.device) if want_cs else None
    _lib.check(lib.cnerf_ssim_fwd(_p(X), _p(Y), N, Cc, H, W, int(win_size), float(win_sigma), float(C1), float(C2), _p(s), _p(cs),
                                  _p(ws), _stream()), "cnerf_ssim_fwd")
    return s, cs


def ssim_backward(X: Tensor, Y: Tensor, win_size: int, win_sigma: float, C1: float, C2: float, g_ssim: Tensor, want_dY: bool = True):
    """cnerf_ssim_bwd: (dX, dY | None), the gradient of sum(g_ssim * ssim) (g_ssim [N, C])."""
    X, Y = _ssim_args(X, Y, win_size)
    N, Cc, H, W = X.shape
    g = _chk(g_ssim.reshape(N, Cc), "g_ssim")
    lib = _lib.load()
    ws = torch.empty(lib.cnerf_ssim_bwd_ws_floats(N, Cc, H, W, int(win_size)), device=X.device)
    dX = torch.empty_like(X)
    dY = torch.empty_like(Y) if want_dY else None
    _lib.check(lib.cnerf_ssim_bwd(_p(X), _p(Y), N, Cc, H, W, int(win_size), float(win_sigma), float(C1), float(C2), _p(g), _p(dX),
                                  _p(dY), _p(ws), _stream()), "cnerf_ssim_bwd")
    return dX, dY


def avg_pool2(X: Tensor) -> Tensor:
    """cnerf_avg_pool2: avg_pool2d(X, 2, stride=2, padding=[H % 2, W % 2]) with the padding counted (MS-SSIM's level step)."""
    X = _chk(X, "X")
    N, Cc, H, W = X.shape
    out = torch.empty(N, Cc, H // 2 + H % 2, W // 2 + W % 2, device=X.device)
    _lib.check(_lib.load().cnerf_avg_pool2(_p(X), N, Cc, H, W, _p(out), _stream()), "cnerf_avg_pool2")
    return out


def _msssim_pyr_floats(N: int, Cc: int, H: int, W: int, levels: int) -> int:
    """Floats of the pooled levels 2 .. `levels` of X and of Y (include/cnerf.h: pyr)."""
    n = 0
    for _ in range(int(levels) - 1):
        H, W = H // 2 + H % 2, W // 2 + W % 2
        n += N * Cc * H * W
    return 2 * n


def msssim_forward(X: Tensor, Y: Tensor, win_size: int, win_sigma: float, C1: float, C2: float, levels: int):
    """cnerf_msssim_fwd: (v [levels, N, C], pyr) — v = per plane the mean of cs at the levels below the last and of SSIM at the
    last; pyr = the pooled levels of X and Y, what msssim_backward needs besides X and Y."""
    X, Y = _ssim_args(X, Y, win_size)
    N, Cc, H, W = X.shape
    lib = _lib.load()
    ws = torch.empty(max(1, lib.cnerf_msssim_ws_floats(N, Cc, H, W, int(win_size), int(levels)) // 2), device=X.device,
                     dtype=torch.float64)
    v = torch.empty(int(levels), N, Cc, device=X.device)
    pyr = torch.empty(max(1, _msssim_pyr_floats(N, Cc, H, W, levels)), device=X.device)
    _lib.check(lib.cnerf_msssim_fwd(_p(X), _p(Y), N, Cc, H, W, int(win_size), float(win_sigma), float(C1), float(C2), int(levels),
                                    _p(v), _p(pyr), _p(ws), _stream()), "cnerf_msssim_fwd")
    return v, pyr


def msssim_backward(X: Tensor, Y: Tensor, win_size: int, win_sigma: float, C1: float, C2: float, pyr: Tensor, g_v: Tensor,
                    want_dY: bool = True):
    """cnerf_msssim_bwd: (dX, dY | None), the gradient of sum(g_v * v) (g_v [levels, N, C]; pyr from msssim_forward)."""
    X, Y = _ssim_args(X, Y, win_size)
    N, Cc, H, W = X.shape
    levels = g_v.shape[0]
    g = _chk(g_v.reshape(levels, N, Cc), "g_v")
    pyr = _chk(pyr, "pyr")
    if pyr.numel() < _msssim_pyr_floats(N, Cc, H, W, levels):
        raise CnerfError(f"msssim_backward: pyr holds {pyr.numel()} floats, {levels} levels of {tuple(X.shape)} need more")
    lib = _lib.load()
    ws = torch.empty(max(1, lib.cnerf_msssim_bwd_ws_floats(N, Cc, H, W, int(win_size), levels)), device=X.device)
    dX = torch.empty_like(X)
    dY = torch.empty_like(Y) if want_dY else None
    _lib.check(lib.cnerf_msssim_bwd(_p(X), _p(Y), N, Cc, H, W, int(win_size), float(win_sigma), float(C1), float(C2), levels, _p(pyr),
                                    _p(g), _p(dX), _p(dY), _p(ws), _stream()), "cnerf_msssim_bwd")
    return dX, dY


def patch_ssim_loss(rgb: Tensor, target: Tensor, P: int, want_grad: bool = True):
    """V:1696-1720's SSIM lines (cnerf_patch_ssim_loss): (value[1] = sum_p ssim_p / 4, d value / d rgb [P * 256, 3] | None) over
    the first P * 256 rays."""
    rgb, target = _chk(rgb.reshape(-1, 3), "rgb"), _chk(target.reshape(-1, 3), "target")
    n = int(P) * PATCH_SSIM_RAYS
    if rgb.shape[0] < n or target.shape[0] < n:
        raise CnerfError(f"patch_ssim_loss: need {P} x {PATCH_SSIM_RAYS} rays, got {rgb.shape[0]} / {target.shape[0]}")
    value = torch.empty(1, device=rgb.device)
    d = torch.empty(n, 3, device=rgb.device) if want_grad else None
    _lib.check(_lib.load().cnerf_patch_ssim_loss(_p(rgb), _p(target), int(P), _p(value), _p(d), _stream()), "cnerf_patch_ssim_loss")
    return value, d


# ---- LPIPS (csrc/lpips.hip) --------------------------------------------------------------------------------------------------------
LPIPS_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                  (512, 512), (512, 512), (512, 512))          # (Cin, Cout) of the 13 convolutions
LPIPS_POOL_BEFORE = (2, 4, 7, 10)                              # a 2x2 max pool feeds these layers
LPIPS_TAPS = (1, 3, 6, 9, 12)                                  # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3


def _nchw(t: Tensor, name: str, channels: Optional[int] = None) -> Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise CnerfError(f"{name} must be a float32 GPU tensor (consistentnerf_amd has no CPU path), got "
                         f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '-')}")
    if t.dim() != 4 or t.numel() == 0 or (channels is not None and t.shape[1] != channels):
        raise CnerfError(f"{name} must be a non-empty [N, {channels or 'C'}, H, W] tensor, got {tuple(t.shape)}")
    return t.contiguous()


def conv3x3_pack(w: Tensor, transposed: bool = False) -> Tensor:
    """cnerf_conv3x3_pack: w [Cout, Cin, 3, 3] -> the MFMA panels of the forward (or, transposed, of the input gradient)."""
    w = _nchw(w, "w")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3):
        raise CnerfError(f"conv3x3_pack: w must be [Cout, Cin, 3, 3], got {tuple(w.shape)}")
    lib = _lib.load()
    panel = torch.empty(lib.cnerf_conv3x3_packed_floats(Cin, Cout, int(transposed)), device=w.device)
    _lib.check(lib.cnerf_conv3x3_pack(_p(w), Cin, Cout, int(transposed), _p(panel), _stream()), "cnerf_conv3x3_pack")
    return panel


def _conv_ws(lib, N, Cin, Cout, H, W, device):
    n = lib.cnerf_conv3x3_ws_floats(N, Cin, Cout, H, W)
    return torch.empty(n, device=device) if n else None


def conv3x3_forward(x: Tensor, panel: Tensor, bias: Optional[Tensor], Cout: int, relu: bool = True) -> Tensor:
    """cnerf_conv3x3_fwd: conv2d(x, w, bias, padding=1) (then ReLU) with w packed by conv3x3_pack(w)."""
    x = _nchw(x, "x")
    N, Cin, H, W = x.shape
    lib = _lib.load()
    out = torch.empty(N, Cout, H, W, device=x.device)
    ws = _conv_ws(lib, N, Cin, Cout, H, W, x.device)
    _lib.check(lib.cnerf_conv3x3_fwd(_p(x), _p(panel), _p(_chk(bias, "bias")), N, Cin, Cout, H, W, int(relu), _p(out), _p(ws), _stream()),
               "cnerf_conv3x3_fwd")
    return out


def conv3x3_dgrad(g: Tensor, panel_t: Tensor, Cin: int, gate: Optional[Tensor] = None) -> Tensor:
    """cnerf_conv3x3_dgrad: the input gradient of conv2d(., w, padding=1) for the output gradient g [N, Cout, H, W], w packed by
    conv3x3_pack(w, transposed=True); gate (the layer's post-ReLU output) zeroes g where gate <= 0."""
    g = _nchw(g, "g")
    N, Cout, H, W = g.shape
    gate = None if gate is None else _nchw(gate, "gate", Cout)
    lib = _lib.load()
    d = torch.empty(N, Cin, H, W, device=g.device)
    ws = _conv_ws(lib, N, Cin, Cout, H, W, g.device)
    _lib.check(lib.cnerf_conv3x3_dgrad(_p(g), _p(gate), _p(panel_t), N, Cin, Cout, H, W, _p(d), _p(ws), _stream()), "cnerf_conv3x3_dgrad")
    return d


def maxpool2_forward(x: Tensor) -> Tensor:
    """cnerf_maxpool2_fwd: max_pool2d(x, 2, 2)."""
    x = _nchw(x, "x")
    N, Cc, H, W = x.shape
    out = torch.empty(N, Cc, H // 2, W // 2, device=x.device)
    _lib.check(_lib.load().cnerf_maxpool2_fwd(_p(x), N, Cc, H, W, _p(out), _stream()), "cnerf_maxpool2_fwd")
    return out


def maxpool2_backward(x: Tensor, g: Tensor, add: Optional[Tensor] = None) -> Tensor:
    """cnerf_maxpool2_bwd: the gradient of max_pool2d(x, 2, 2) w.r.t. x for the output gradient g (+ add)."""
    x = _nchw(x, "x")
    N, Cc, H, W = x.shape
    g = _nchw(g, "g", Cc)
    add = None if add is None else _nchw(add, "add", Cc)
    d = torch.empty_like(x)
    _lib.check(_lib.load().cnerf_maxpool2_bwd(_p(x), _p(g), _p(add), N, Cc, H, W, _p(d), _stream()), "cnerf_maxpool2_bwd")
    return d


def lpips_head_forward(F0: Tensor, F1: Tensor, lin: Tensor) -> Tensor:
    """cnerf_lpips_head_fwd: one tap's value [N] for the feature sets F0, F1 [N, C, H, W] and the lin weight [C]."""
    F0, F1 = _nchw(F0, "F0"), _nchw(F1, "F1")
    N, Cc, H, W = F0.shape
    lib = _lib.load()
    ws = torch.empty(max(1, lib.cnerf_lpips_head_ws_floats(N, H, W) // 2), device=F0.device, dtype=torch.float64)
    v = torch.empty(N, device=F0.device)
    _lib.check(lib.cnerf_lpips_head_fwd(_p(F0), _p(F1), _p(_chk(lin.reshape(-1), "lin")), N, Cc, H, W, _p(v), _p(ws), _stream()),
               "cnerf_lpips_head_fwd")
    return v


def lpips_head_backward(F0: Tensor, F1: Tensor, lin: Tensor, g: Tensor) -> Tensor:
    """cnerf_lpips_head_bwd: the gradient of sum(g * value) w.r.t. F0."""
    F0, F1 = _nchw(F0, "F0"), _nchw(F1, "F1")
    N, Cc, H, W = F0.shape
    d = torch.empty_like(F0)
    _lib.check(_lib.load().cnerf_lpips_head_bwd(_p(F0), _p(F1), _p(_chk(lin.reshape(-1), "lin")), _p(_chk(g.reshape(N), "g")), N, Cc, H, W,
                                                _p(d), _stream()), "cnerf_lpips_head_bwd")
    return d


def lpips_pack(convs: Sequence[Tensor], lins: Sequence[Tensor], shift: Tensor, scale: Tensor) -> Tensor:
    """cnerf_lpips_pack: convs = weight, bias of the 13 convolutions in order (26 tensors), lins = the five [C] weights."""
    ts = [_chk(t, "lpips weight") for t in list(convs) + [w.reshape(-1) for w in lins] + [shift.reshape(-1), scale.reshape(-1)]]
    want = [s for ci, co in LPIPS_CHANNELS for s in ((co, ci, 3, 3), (co,))] + [(LPIPS_CHANNELS[l][1],) for l in LPIPS_TAPS] + [(3,), (3,)]
    if [tuple(t.shape) for t in ts] != want:
        raise CnerfError("lpips_pack: tensor shapes do not match VGG16 + lin + scaling layer")
    lib = _lib.load()
    packed = torch.empty(lib.cnerf_lpips_packed_floats(), device=ts[0].device)
    _lib.check(lib.cnerf_lpips_pack(C.byref(_ptrs(ts)), _p(packed), _stream()), "cnerf_lpips_pack")
    return packed


def lpips_forward(X: Tensor, Y: Tensor, packed: Tensor, keep: bool = False, want_taps: bool = False, want_acts: bool = False):
    """cnerf_lpips_fwd: (value [N], per-tap [5, N] | None, workspace | None, activations | None).  keep holds the activations in the
    returned workspace for lpips_backward; want_acts (with keep) also returns the 13 post-ReLU activations [2 N, C, h, w] (X's images
    first) as copies."""
    X, Y = _nchw(X, "X", 3), _nchw(Y, "Y", 3)
    if X.shape != Y.shape:
        raise CnerfError(f"lpips: X and Y must have one shape, got {tuple(X.shape)} / {tuple(Y.shape)}")
    N, _, H, W = X.shape
    lib = _lib.load()
    n = lib.cnerf_lpips_ws_floats(N, H, W, int(keep))
    if n <= 0:
        raise CnerfError(f"lpips: unsupported shape {tuple(X.shape)} (sides >= 16)")
    ws = torch.empty(n, device=X.device)
    value = torch.empty(N, device=X.device)
    taps = torch.empty(5, N, device=X.device) if want_taps else None
    _lib.check(lib.cnerf_lpips_fwd(_p(X), _p(Y), _p(packed), N, H, W, int(keep), _p(value), _p(taps), _p(ws), _stream()), "cnerf_lpips_fwd")
    acts = None
    if want_acts:
        if not keep:
            raise CnerfError("lpips_forward: want_acts needs keep=True")
        acts, h, w = [], H, W
        for l, (_, co) in enumerate(LPIPS_CHANNELS):
            if l in LPIPS_POOL_BEFORE:
                h, w = h // 2, w // 2
            off = lib.cnerf_lpips_act_offset(N, H, W, l)
            acts.append(ws[off:off + 2 * N * co * h * w].view(2 * N, co, h, w).clone())
    return value, taps, (ws if keep else None), acts


def lpips_backward(packed: Tensor, ws: Tensor, g: Tensor, shape) -> Tensor:
    """cnerf_lpips_bwd: the gradient of sum(g * value) w.r.t. X after lpips_forward(X, Y, packed, keep=True) returned ws."""
    N, _, H, W = shape
    dX = torch.empty(N, 3, H, W, device=ws.device)
    _lib.check(_lib.load().cnerf_lpips_bwd(_p(packed), _p(_chk(g.reshape(N), "g")), N, H, W, _p(dX), _p(ws), _stream()), "cnerf_lpips_bwd")
    return dX


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8,
              clip: float = 0.0, grad_scale: float = 1.0):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise CnerfError(f"adam_step: {n} must be a contiguous fp32 GPU tensor")
    _lib.check(_lib.load().cnerf_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), int(step), float(lr), float(beta1),
                                           float(beta2), float(eps), float(clip), float(grad_scale), _stream()),
               "cnerf_adam_step")


def adam_hyper(out_host: Tensor, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, clip: float = 0.0,
               grad_scale: float = 1.0):
    """cnerf_adam_hyper: the 8 scalars of step `step` into a (pinned) HOST float tensor."""
    if out_host.is_cuda or out_host.dtype != torch.float32 or out_host.numel() < 8 or not out_host.is_contiguous():
        raise CnerfError("adam_hyper: need a contiguous fp32 host tensor of 8 floats")
    _lib.check(_lib.load().cnerf_adam_hyper(int(step), float(lr), float(beta1), float(beta2), float(eps), float(clip),
                                            float(grad_scale), C.c_void_p(out_host.data_ptr())), "cnerf_adam_hyper")


def adam_step_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyp_dev: Tensor):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (hyp_dev, "hyp")):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise CnerfError(f"adam_step_dev: {n} must be a contiguous fp32 GPU tensor")
    _lib.check(_lib.load().cnerf_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyp_dev), _stream()),
               "cnerf_adam_step_dev")


# ---- the test-set pass (V:2034-2087): depth-map images and the metric inputs ---------------------------------------------------------
def _frames(t: Tensor, name: str, dims: int) -> Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise CnerfError(f"{name} must be a float32 GPU tensor (consistentnerf_amd has no CPU path), got "
                         f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '-')}")
    if t.dim() != dims or t.numel() == 0:
        raise CnerfError(f"{name} must be a non-empty {dims}-d tensor, got {tuple(t.shape)}")
    return t.contiguous()


def depthvis(disp: Tensor, acc: Tensor, lo: Optional[float] = None, hi: Optional[float] = None, want_f32: bool = True,
             want_u8: bool = True):
    """cnerf_depthvis: disp, acc [N, H, W] -> (img_f32 [N, H, W, 3] | None, img_u8 [N, H, W, 3] uint8 | None, bounds [N, 2]) =
    lky_visualize_depth(1 / disp, acc, lo, hi), its save_img_u8 bytes, and the automatic (lo_auto, hi_auto) of every frame."""
    disp, acc = _frames(disp, "disp", 3), _frames(acc, "acc", 3)
    if disp.shape != acc.shape:
        raise CnerfError(f"depthvis: disp and acc must have one shape, got {tuple(disp.shape)} / {tuple(acc.shape)}")
    N, H, W = disp.shape
    lib = _lib.load()
    n = lib.cnerf_depthvis_ws_bytes(N, H, W)
    if n <= 0:
        raise CnerfError(f"depthvis: unsupported shape {tuple(disp.shape)}")
    ws = torch.empty((n + 7) // 8, device=disp.device, dtype=torch.float64)
    f32 = torch.empty(N, H, W, 3, device=disp.device) if want_f32 else None
    u8 = torch.empty(N, H, W, 3, device=disp.device, dtype=torch.uint8) if want_u8 else None
    bounds = torch.empty(N, 2, device=disp.device)
    _lib.check(lib.cnerf_depthvis(_p(disp), _p(acc), N, H, W, float(lo or 0.), float(hi or 0.), int(lo is not None), int(hi is not None),
                                  _p(f32), _p(u8), _p(bounds), _p(ws), _stream()), "cnerf_depthvis")
    return f32, u8, bounds


def eval_prep(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None, want_ssim: bool = True, want_lpips: bool = True,
              want_sums: bool = True):
    """cnerf_eval_prep: pred, gt [N, H, W, 3] in [0, 1], mask [N, H, W] | None -> ((ssim_pred, ssim_gt) | None, (lpips_pred, lpips_gt)
    | None, sums [1 + 2 N] float64 | None): the [N, 3, H, W] inputs of img2ssim's and img2lpips' kernels and the PSNR partial sums
    (include/cnerf.h)."""
    pred, gt = _frames(pred, "pred", 4), _frames(gt, "gt", 4)
    if pred.shape != gt.shape or pred.shape[-1] != 3:
        raise CnerfError(f"eval_prep: pred and gt must be [N, H, W, 3] of one shape, got {tuple(pred.shape)} / {tuple(gt.shape)}")
    N, H, W, _ = pred.shape
    if mask is not None:
        mask = _frames(mask, "mask", 3)
        if mask.shape != pred.shape[:3]:
            raise CnerfError(f"eval_prep: mask must be {tuple(pred.shape[:3])}, got {tuple(mask.shape)}")
    lib = _lib.load()
    n = lib.cnerf_eval_prep_ws_bytes(N, H, W)
    if n <= 0:
        raise CnerfError(f"eval_prep: unsupported shape {tuple(pred.shape)}")
    new = lambda: torch.empty(N, 3, H, W, device=pred.device)  # noqa: E731
    ssim = (new(), new()) if want_ssim else None
    lp = (new(), new()) if want_lpips else None
    sums = torch.empty(1 + 2 * N, device=pred.device, dtype=torch.float64) if want_sums else None
    ws = torch.empty((n + 7) // 8, device=pred.device, dtype=torch.float64) if want_sums else None
    _lib.check(lib.cnerf_eval_prep(_p(pred), _p(gt), _p(mask), N, H, W, _p(ssim[0] if ssim else None), _p(ssim[1] if ssim else None),
                                   _p(lp[0] if lp else None), _p(lp[1] if lp else None), _p(sums), _p(ws), _stream()), "cnerf_eval_prep")
    return ssim, lp, sums
