"""Drop-in for the render / model-construction surface of the reference's run_nerf.py (R):

  batchify R:27 | run_network R:37 | batchify_rays R:55 | render R:70 | render_path R:140 |
  create_nerf R:181 | raw2outputs R:265 | render_rays R:311

Same signatures, kwargs dictionaries and return structures; the bodies launch the gfx950 kernels of
libcnerf_hip.so (include/cnerf.h).  Autograd is wired with two torch.autograd.Function nodes (fused
encoding+MLP, compositing); sampling carries no gradient, exactly like the reference (R:397).  Sample points, view directions
and the rays of render(rays=(rays_o, rays_d), ndc=False) take gradients too (csrc/mlp_igrad.hip, behind the same backward), and so do
the finished ray rows of render_loss(rows=...), on the folded training step (both levels in one grid per launch).

`run_nerf_view.py` of this package layers the ConsistentNeRF additions (depth outputs, warp, hard masks,
masked losses) on top of this module.
"""
import os
import time
import weakref

import numpy as np
import torch

from . import ops
from .optim import FusedAdam
from .run_nerf_helpers import (NeRF, get_embedder, get_rays, get_rays_at, img2mse, mse2psnr, ndc_coefficients,  # noqa: F401
                               get_rays_np, ndc_rays, pytest_uniform, sample_pdf, sample_u, to8b)

DEBUG = False


# ----------------------------------------------------------------------------- autograd nodes
class RayPoints:
    """Lazy stand-in for the [N_rays, N_samples, 3] point tensor of R:384: the fused kernel evaluates
    o + d*z itself, so the 9.4 MB/step point cloud is never written.  `.materialize()` gives the tensor."""

    def __init__(self, rays, z_vals, live=None, skip=0):
        self.rays, self.z_vals = rays, z_vals
        self.live = live          # device int32 [1]: only the first live[0] rays are real (a batch padded to a fixed capacity)
        self.skip = skip          # (with live) the first `skip` rays get zero seeds: the backward of this query may leave them out
        self.shape = torch.Size([z_vals.shape[0], z_vals.shape[1], 3])
        self.device = z_vals.device

    def materialize(self):
        return self.rays[:, None, 0:3] + self.rays[:, None, 3:6] * self.z_vals[..., None]


class _PanelCache:
    """The kernel-layout copy of one model's weights, one object per model and kind (NeRF.invalidate_packed drops both): the fp32
    panels (`planes` None) and the bf16- / fp16-plane panels of the opt-in reduced-precision forward and the bf16x3 training kernels
    (`planes` = the mode's value in ops.PRECISION_PLANES, distinct per mode).  Re-packed only when a parameter changed (optimizer
    step / load) or the mode did.  Two buffers alternate, so the copy a forward pass used stays intact for its backward without a
    per-step clone (forward A, step, forward B, backward A is legal): it is overwritten by the SECOND re-pack after it — two
    parameter updates between a forward and its backward, where the reference itself fails (autograd's version check)."""
    __slots__ = ("key", "bufs", "gen", "buf", "planes")
    SLOT = {False: "_cnerf_packed", True: "_cnerf_packed_bf"}       # where a model keeps it, by `planes is not None`

    def __init__(self):
        self.key, self.bufs, self.gen, self.buf, self.planes = None, [None, None], -1, None, None

    @staticmethod
    def probe(model, planes=None):
        """(the model's cache of this kind or None, its kernel tensors, their identity / version key now)"""
        ts = model.kernel_tensors()
        key = tuple((t.data_ptr(), t._version, getattr(t, "_cnerf_epoch", 0)) for t in ts)
        return model.__dict__.get(_PanelCache.SLOT[planes is not None]), ts, key if planes is None else (planes,) + key

    def next_out(self, planes=None):
        """The buffer the next re-pack overwrites (None: the packer allocates it; always after a change of `planes`)."""
        return self.bufs[(self.gen + 1) & 1] if planes == self.planes else None

    def commit(self, model, key, buf, planes=None):
        """`buf` holds the panels of `key`: the next generation (monotonic also across a change of `planes`, which drops both buffers)."""
        if planes != self.planes:
            self.bufs, self.planes = [None, None], planes
        self.gen += 1
        self.bufs[self.gen & 1] = self.buf = buf
        self.key = key
        model.__dict__[self.SLOT[planes is not None]] = self

    @staticmethod
    def get(model, planes=None):
        """-> (buffer, generation) of the current panels of `model`, re-packed first when stale."""
        c, ts, key = _PanelCache.probe(model, planes)
        if c is None or c.key != key:
            c = _PanelCache() if c is None else c
            out = c.next_out(planes)
            with torch.no_grad():
                buf = ops.pack_weights(model.spec(), ts, out) if planes is None else ops.pack_weights_bf(model.spec(), ts, planes, out)
            c.commit(model, key, buf, planes)
        return c.buf, c.gen

    def still_valid(self, gen, buf):
        """May a backward still read `buf`, packed as generation `gen`?  Not after a second re-pack.  The plane panels also insist on
        `buf` being one of the two buffers: after invalidate_packed() + a new forward they refuse, the fp32 panels accept."""
        return self.gen - gen <= 1 and (self.planes is None or any(b is buf for b in self.bufs))


def _packed(model):
    return _PanelCache.get(model)[0]


def _packed_bf(model, planes):
    return _PanelCache.get(model, planes)[0]


def _still_valid(model, gen, buf, planes=None):
    c = model.__dict__.get(_PanelCache.SLOT[planes is not None])
    return c is not None and c.still_valid(gen, buf)


def _prepack_pair(model_a, model_b):
    """render_rays is about to query both networks: when BOTH kernel-layout copies are stale (every training step: the optimizer
    just wrote both) re-pack them with one launch instead of one each."""
    if model_a is None or model_b is None or model_a is model_b:
        return
    st = []
    for m in (model_a, model_b):
        if not hasattr(m, "kernel_tensors"):
            return
        c, ts, key = _PanelCache.probe(m)
        if c is not None and c.key == key:
            return                               # (at most one is stale: its own query re-packs it)
        st.append((m, ts, key, _PanelCache() if c is None else c))
    (ma, tsa, ka, ca), (mb, tsb, kb, cb) = st
    if tsa[0].device != tsb[0].device or not tsa[0].is_cuda:
        return
    with torch.no_grad():
        pa, pb = ops.pack_weights_pair(ma.spec(), tsa, ca.next_out(), mb.spec(), tsb, cb.next_out())
    ca.commit(ma, ka, pa)
    cb.commit(mb, kb, pb)


# Training arithmetic: "fp32" (default: exact fp32 MFMA, the arithmetic every parity statement and the headline bench line are
# made in) or "bf16x3" (opt-in: bf16 matrix cores, three planes per operand, fp32 accumulation — reported as a SECOND bench line
# only).  Per model (`NeRF.training_precision`), or for the whole process with CNERF_TRAIN_PRECISION (what the GPU suite uses to
# run every test in that arithmetic as well).
DEFAULT_TRAINING_PRECISION = os.environ.get("CNERF_TRAIN_PRECISION", "fp32")


def training_precision(model):
    """An explicit `model.training_precision` is obeyed (an architecture the bf16x3 kernels are not compiled for then fails
    loudly in the launch); the process-wide default only applies to architectures they cover (view directions, W = 128 | 256,
    the 10 / 4-frequency encodings) and leaves every other network on the exact-fp32 path."""
    prec = getattr(model, "training_precision", None)
    if prec is None:
        prec = DEFAULT_TRAINING_PRECISION
        if prec == "bf16x3":
            sp = model.spec()
            if not (sp.use_viewdirs and sp.W in (128, 256) and sp.multires == 10 and sp.multires_views == 4):
                prec = "fp32"
    if prec not in ("fp32", "bf16x3"):
        raise ValueError("training_precision must be 'fp32' or 'bf16x3'")
    return prec


def _probe_engine_query():
    """The direct-accumulate route and the merged coarse+fine backward ask the autograd engine, from inside a backward node,
    whether another node is going to run in the same pass: `torch._C._will_engine_execute_node` — a PRIVATE symbol.  This
    probe runs once at import, on the CPU: the symbol must exist, answer True for a leaf's AccumulateGrad node under
    .backward(), and refuse (RuntimeError) or answer False under torch.autograd.grad().  Anything else -> (None, reason) and
    the module selects the plain route explicitly: per-tensor gradients handed back to autograd, one backward per level."""
    fn = getattr(torch._C, "_will_engine_execute_node", None)
    if fn is None:
        return None, "torch._C._will_engine_execute_node does not exist in this torch"
    seen = []

    class _Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            ctx.w = w
            return x * 1.0

        @staticmethod
        def backward(ctx, g):
            with torch.enable_grad():
                acc = ctx.w.view_as(ctx.w).grad_fn.next_functions[0][0]
            try:
                seen.append(bool(fn(acc)))
            except RuntimeError:
                seen.append("refused")
            return g, None

    try:
        w = torch.ones(2, requires_grad=True)
        _Probe.apply(w * 2.0, w).sum().backward()
        torch.autograd.grad(_Probe.apply(w * 2.0, w).sum(), [w])
    except Exception as e:   # noqa: BLE001 — any failure of the probe selects the plain route
        return None, f"probing torch._C._will_engine_execute_node raised {type(e).__name__}: {e}"
    if len(seen) != 2 or seen[0] is not True or seen[1] not in (False, "refused"):
        return None, f"torch._C._will_engine_execute_node answered {seen} (expected [True, False | refused])"
    return fn, None


_ENGINE_QUERY, _ENGINE_QUERY_WHY = _probe_engine_query()
if _ENGINE_QUERY is None:
    import warnings
    warnings.warn("consistentnerf_amd: " + _ENGINE_QUERY_WHY + " — training falls back to the plain autograd route "
                  "(per-tensor gradients returned to autograd, coarse and fine backward launched separately); results are "
                  "identical, the step is ~2 % slower", RuntimeWarning)


def _engine_accumulates(p):
    """True when the running backward pass will ACCUMULATE into p.grad (loss.backward(), also with inputs=[...]); False
    under torch.autograd.grad(), where the engine captures the gradient of a leaf instead (it refuses the query for a
    leaf's AccumulateGrad node in that mode — that refusal is the signal), and False when the engine query is unusable in
    this torch (_probe_engine_query)."""
    if _ENGINE_QUERY is None:
        return False
    with torch.enable_grad():
        acc = p.view_as(p).grad_fn.next_functions[0][0]
    try:
        return bool(_ENGINE_QUERY(acc))
    except RuntimeError:
        return False


# The coarse and the fine network's backward passes share nothing once the forward is done (z is detached at R:397): when
# both are FusedAdam-owned they run as ONE dgrad grid + ONE wgrad grid (cnerf_mlp_bwd_pair) instead of two of each — the
# 8-round coarse launches otherwise pay their own ramp and tail.  CNERF_MERGE_BWD=0 keeps them separate.
MERGE_BWD = os.environ.get("CNERF_MERGE_BWD", "1") != "0"


class _LevelJob:
    """What the MLP backward of one level launches with, taken from its node (`ctx`) and the gradient of its output.  `d_raw` is
    made contiguous here: when the fine node parks, in ITS backward."""
    __slots__ = ("spec", "packed", "packed_bf", "d_raw", "B", "S", "stash", "params", "model", "live", "skip", "needs", "z",
                 "ray_stride", "dirs_given")

    def __init__(self, ctx, g_raw):
        self.spec, self.packed, self.packed_bf, self.d_raw = ctx.spec, ctx.packed, ctx.packed_bf, g_raw.contiguous()
        self.B, self.S, self.stash, self.params, self.model = ctx.B, ctx.S, ctx.stash, ctx.params, ctx.model
        self.live, self.skip, self.needs = ctx.live, ctx.skip, ctx.needs_input_grad
        # a level whose inputs take a gradient: the sample depths and the form of the inputs (_MlpFn.forward)
        self.z, self.ray_stride, self.dirs_given = (ctx.z, ctx.ray_stride, ctx.dirs_given) if ctx.igrad else (None, None, False)


class _LevelPair:
    """Links the coarse and the fine _MlpFn node of one render_rays call.  The fine node runs first in the backward pass
    (it was created last); if the engine is going to run the coarse node too, it parks its _LevelJob here and the coarse node
    launches both."""
    __slots__ = ("coarse", "fine", "parked")

    def __init__(self, coarse_node, fine_node):
        self.coarse, self.fine, self.parked = weakref.ref(coarse_node), weakref.ref(fine_node), None


def _link_levels(raw_coarse, raw_fine):
    nc, nf = raw_coarse.grad_fn, raw_fine.grad_fn
    if not MERGE_BWD or _ENGINE_QUERY is None or nc is None or nf is None:
        return
    if getattr(nc, "stash", None) is None or getattr(nf, "stash", None) is None or nc.model is nf.model:
        return
    if getattr(nc, "igrad", False) or getattr(nf, "igrad", False):
        # a level whose inputs take a gradient runs on its own (_MlpFn._input_grads) — except the two levels of one batch of ray rows
        # that both hand a gradient to those rows and to their parameters (the camera chain): those pair up (_run_pair_rows)
        if not (_rows_level(nc) and _rows_level(nf) and nc.B == nf.B and nc.ray_stride == nf.ray_stride
                and bool(nc.spec.use_viewdirs) == bool(nf.spec.use_viewdirs)):
            return
    nc.pair = nf.pair = _LevelPair(nc, nf)


def _rows_level(n):
    """A level that _link_levels may pair although its inputs take a gradient: the gradient goes to the ray rows alone (no points or
    view directions given, so the view directions sit in the rows), the parameters take theirs, and the batch is not `live`."""
    needs = n.needs_input_grad
    return (n.igrad and needs[4] and not needs[3] and not needs[6] and n.ray_stride is not None and not n.dirs_given
            and n.live is None and any(needs[10:]))


def _direct_ok(needs, params):
    # .grad must BE FusedAdam's view of the flat gradient: after `p.grad = None` autograd attaches a tensor of its own, and a
    # direct write into that one would bypass (and, on the overwrite route, destroy) what the optimiser steps on
    return all(needs) and all(getattr(p, "_cnerf_direct_grad", False) and p.grad is not None
                              and p.grad.data_ptr() == p._cnerf_view_ptr and p.grad.is_contiguous() for p in params)


def _take_dropped(*param_lists):
    """The direct route is about to write these parameters' views of FusedAdam's flat gradient.  True when none of them holds a
    live gradient (all dropped by zero_grad(), or still zero): the wgrad reduction then OVERWRITES (accumulate=0) and the fill
    launch of an eager zero_grad never happens.  In a mixed state the dropped views are zeroed here and the reduction adds."""
    from .optim import GRAD_DETACHED, GRAD_DROPPED, GRAD_LIVE
    ps = [p for params in param_lists for p in params]
    fresh = all(p._cnerf_grad_state not in (GRAD_LIVE, GRAD_DETACHED) for p in ps)
    for p in ps:
        if not fresh and p._cnerf_grad_state == GRAD_DROPPED:
            p.grad.zero_()
        p._cnerf_grad_state = GRAD_LIVE
    return fresh


def _report_ready(models, direct):
    """One backward node of each of `models` has run: on the direct route (it accumulated into the flat gradient) tell the
    GradReducer of those it was the last node of.  The merged backward finishes BOTH networks at once: reported together, so that a
    reducer that owns both sends their (adjacent) slices of the flat gradient as ONE message instead of two back-to-back ones."""
    ready = []
    for m in models:
        if hasattr(m, "_cnerf_pending"):
            m._cnerf_pending -= 1
            if direct and m._cnerf_pending <= 0:
                ready.append(m)
    if len(ready) == 2 and ready[0]._cnerf_reducer is ready[1]._cnerf_reducer:
        ready[0]._cnerf_reducer.networks_ready(ready)
    else:
        for m in ready:
            m._cnerf_reducer.network_ready(m)


def _run_single(job, direct):
    """One level on its own -> its gradients (on the direct route: the parameters' views of the flat gradient, written in place)."""
    out = [p.grad for p in job.params] if direct else None
    grads = ops.mlp_backward(job.spec, job.packed, job.d_raw, job.B, job.S, job.stash, grads=out,
                             accumulate=direct and not _take_dropped(job.params), packed_bf=job.packed_bf, live=job.live)
    _report_ready([job.model], direct)
    return grads


def _run_pair(fine, coarse):
    """Both levels as one launch, on the direct route (bf16x3 only when both carry a plane buffer: ops.mlp_backward_pair)."""
    live = coarse.live
    ops.mlp_backward_pair(fine.spec, fine.packed, fine.d_raw, fine.B, fine.S, fine.stash, [p.grad for p in fine.params],
                          coarse.spec, coarse.packed, coarse.d_raw, coarse.B, coarse.S, coarse.stash, [p.grad for p in coarse.params],
                          accumulate=not _take_dropped(fine.params, coarse.params), packed_bf0=fine.packed_bf,
                          packed_bf1=coarse.packed_bf, live=live, first0=fine.skip if live is not None else 0,
                          first1=coarse.skip if live is not None else 0)
    _report_ready([fine.model, coarse.model], True)


def _run_pair_rows(fine, coarse):
    """_run_pair for two levels whose ray rows take a gradient too -> the [B, ray_stride] row gradient of BOTH levels: the paired
    backward in workspaces kept here, then cnerf_mlp_input_grad_pair on them and cnerf_rays_input_grad_pair (every column written)."""
    dev = fine.packed.device
    ws = (ops.mlp_bwd_workspace(fine.spec, fine.B, fine.S, dev), ops.mlp_bwd_workspace(coarse.spec, coarse.B, coarse.S, dev))
    ops.mlp_backward_pair(fine.spec, fine.packed, fine.d_raw, fine.B, fine.S, fine.stash, [p.grad for p in fine.params],
                          coarse.spec, coarse.packed, coarse.d_raw, coarse.B, coarse.S, coarse.stash, [p.grad for p in coarse.params],
                          accumulate=not _take_dropped(fine.params, coarse.params), packed_bf0=fine.packed_bf,
                          packed_bf1=coarse.packed_bf, ws=ws)
    _report_ready([fine.model, coarse.model], True)
    (pts_f, dirs_f), (pts_c, dirs_c) = ops.mlp_input_grad_pair(fine.spec, fine.packed, fine.B, fine.S, fine.stash, ws[0],
                                                                coarse.spec, coarse.packed, coarse.B, coarse.S, coarse.stash, ws[1],
                                                                want_dirs=bool(fine.spec.use_viewdirs))
    return ops.rays_input_grad_pair(pts_f, dirs_f, fine.z, pts_c, dirs_c, coarse.z, fine.ray_stride)


class _MlpFn(torch.autograd.Function):
    """Fused gamma(x), gamma(d) + MLP (replaces R:37-52 + H:44-45 + H:107-130 and their autograd)."""

    @staticmethod
    def forward(ctx, model, B, S, pts, rays, z, dirs, emb, live, skip, *params):
        spec = model.spec()
        packed, gen = _PanelCache.get(model)
        need_pts, need_rays, need_z, need_dirs, need_emb = ctx.needs_input_grad[3:8]
        # fail loudly rather than return silently-missing gradients
        if need_emb:
            raise ops.CnerfError("gradients w.r.t. pre-embedded inputs (NeRF.forward(x) with x.requires_grad) are not implemented: "
                                 "run_network(pts, viewdirs, ...) differentiates w.r.t. the points and view directions themselves")
        if need_z:
            raise ops.CnerfError("gradients w.r.t. z_vals are not implemented (the sample depths are detached, R:397)")
        # gradients w.r.t. sample positions / ray rows / view directions: the stash is kept and the backward runs this level alone,
        # dgrad (+ wgrad when parameters take gradients too), then cnerf_mlp_input_grad on the same workspace
        igrad = need_pts or need_rays or need_dirs
        if igrad and live is not None:
            raise ops.CnerfError("input gradients of a `live` batch (a batch padded to a fixed capacity) are not implemented")
        train = any(ctx.needs_input_grad[10:]) or igrad
        packed_bf = bf_gen = use_live = None
        if emb is not None:      # NeRF.forward(x) on pre-embedded inputs
            raw, stash = ops.mlp_forward_embedded(spec, packed, emb, want_stash=train)
        elif train and training_precision(model) == "bf16x3":
            # OPT-IN second training arithmetic (never the default): the forward GEMMs on the bf16 matrix cores at three planes
            # per operand; same stash, so the backward below is unchanged.  `packed` (fp32 panels) still feeds the dgrad.
            packed_bf, bf_gen = _PanelCache.get(model, 3)
            raw, stash = ops.mlp_forward_bf_train(spec, packed_bf, B, S, pts=pts, rays=rays, z=z, dirs=dirs)
        else:
            # `live` (device int32 [1]; RayPoints.live): the batch is padded to its capacity B and only the first live[0] rays are
            # real — the training kernels stop there (run_nerf_view.ss_step_loss: the one-render in-loop consistency step).  Every
            # other route simply processes the padding rays too (they are valid rays whose loss weight is 0: same result, more work).
            use_live = live if (train and pts is None and dirs is None and S % 32 == 0) else None
            raw, stash = ops.mlp_forward(spec, packed, B, S, pts=pts, rays=rays, z=z, dirs=dirs, want_stash=train, live=use_live)
        if train:
            ctx.spec, ctx.B, ctx.S, ctx.stash, ctx.packed, ctx.packed_gen = spec, B, S, stash, packed, gen
            ctx.params, ctx.model = params, model
            ctx.packed_bf, ctx.packed_bf_gen, ctx.live, ctx.pair = packed_bf, bf_gen, use_live, None    # (pair: _link_levels sets it)
            # `skip` (with live): this level's first `skip` rays will get zero seeds — the merged backward leaves them out
            ctx.skip = int(skip) if (use_live is not None and skip) else 0
            ctx.igrad = igrad
            if igrad:       # what the input-gradient launches need beside the stash: the sample depths and the form of the inputs
                ctx.z, ctx.ray_stride, ctx.dirs_given = z, (rays.shape[1] if rays is not None else None), dirs is not None
            # distributed.GradReducer counts this network's backward nodes (those that produce parameter gradients)
            if hasattr(model, "_cnerf_pending") and any(ctx.needs_input_grad[10:]):
                model._cnerf_pending += 1
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        params, pair = ctx.params, ctx.pair
        if not _still_valid(ctx.model, ctx.packed_gen, ctx.packed):
            raise ops.CnerfError("the network's weights were updated twice between this forward pass and its backward "
                                 "(the kernel-layout copy it used has been re-packed)")
        if ctx.packed_bf is not None and not _still_valid(ctx.model, ctx.packed_bf_gen, ctx.packed_bf, planes=3):
            raise ops.CnerfError("the network's weights were updated twice between this bf16x3 forward pass and its backward "
                                 "(the bf16-plane copy it used has been re-packed)")
        if ctx.igrad:
            return _MlpFn._input_grads(ctx, g_raw) if pair is None else _MlpFn._rows_pair_backward(ctx, g_raw)
        # Parameters owned by FusedAdam carry their .grad as a view into the flat gradient buffer: under loss.backward()
        # the wgrad reduction accumulates straight into it (what AccumulateGrad would do with ~50 add/copy launches per
        # step) and autograd gets no per-tensor gradients back.  Anything else — plain nn.Parameters, and
        # torch.autograd.grad() on FusedAdam-owned ones, where the engine captures gradients instead of accumulating them
        # — takes the tensor route and leaves the flat buffer untouched.
        direct = _direct_ok(ctx.needs_input_grad[10:], params) and _engine_accumulates(params[0])
        nret = (None,) * (10 + len(params))
        job = _LevelJob(ctx, g_raw)
        parked = grads = None
        if direct and pair is not None and pair.fine() is ctx and pair.parked is None:
            c = pair.coarse()
            # park only when the coarse node is certain to run in this very pass, on the direct route as well
            if (c is not None and c.stash is not None and _direct_ok(c.needs_input_grad[10:], c.params)
                    and _ENGINE_QUERY(c)):
                pair.parked = job
                ctx.stash = ctx.packed = ctx.params = ctx.model = None
                return nret
        if pair is not None and pair.coarse() is ctx and pair.parked is not None:
            parked, pair.parked = pair.parked, None
        if parked is not None and direct and parked.live is job.live and (job.live is None or parked.B == job.B):
            _run_pair(parked, job)
        else:
            if parked is not None:    # (cannot happen — the fine node checked this node's route — but never drop a gradient)
                _run_single(parked, True)
            grads = _run_single(job, direct)
        ctx.stash = ctx.packed = ctx.params = ctx.model = None
        return nret if direct else (None,) * 10 + tuple(grads)

    @staticmethod
    def _rows_pair_backward(ctx, g_raw):
        """The backward of a level that _link_levels paired although its ray rows take a gradient (_rows_level).  The fine node parks
        under the conditions of the plain pair (both levels on the direct route, the coarse node certain to run in this pass) and
        hands no row gradient back; the coarse node then launches both levels (_run_pair_rows) and returns the row gradient of both.
        Anything else (the tensor route, torch.autograd.grad, a coarse node that does not run): each level alone, as unpaired."""
        params, pair = ctx.params, ctx.pair
        if pair.fine() is ctx:
            c = pair.coarse()
            if (pair.parked is None and _direct_ok(ctx.needs_input_grad[10:], params) and _engine_accumulates(params[0])
                    and c is not None and c.stash is not None and _direct_ok(c.needs_input_grad[10:], c.params) and _ENGINE_QUERY(c)
                    and _engine_accumulates(c.params[0])):
                pair.parked = _LevelJob(ctx, g_raw)
                ctx.stash = ctx.packed = ctx.params = ctx.model = ctx.z = None
                return (None,) * (10 + len(params))
            return _MlpFn._input_grads(ctx, g_raw)
        parked, pair.parked = pair.parked, None
        if parked is None:
            return _MlpFn._input_grads(ctx, g_raw)
        if _direct_ok(ctx.needs_input_grad[10:], params) and _engine_accumulates(params[0]):
            g_rays = _run_pair_rows(parked, _LevelJob(ctx, g_raw))
            ctx.stash = ctx.packed = ctx.params = ctx.model = ctx.z = None
            return (None,) * 4 + (g_rays,) + (None,) * (5 + len(params))
        # (cannot happen — the fine node checked this node's route — but never drop a gradient: the parked level alone, on the direct
        # route it chose, and its row gradient added to this level's)
        g_fine = _MlpFn._level_input_grads(parked)[1]
        own = list(_MlpFn._input_grads(ctx, g_raw))
        own[4] = own[4] + g_fine
        return tuple(own)

    @staticmethod
    def _input_grads(ctx, g_raw):
        """The backward of a level whose sample positions / ray rows / view directions take a gradient, this level alone."""
        g_pts, g_rays, g_dirs, grads = _MlpFn._level_input_grads(_LevelJob(ctx, g_raw))
        n = len(ctx.params)
        ctx.stash = ctx.packed = ctx.params = ctx.model = ctx.z = None
        return (None, None, None, g_pts, g_rays, None, g_dirs, None, None, None) + (tuple(grads) if grads is not None else (None,) * n)

    @staticmethod
    def _level_input_grads(job):
        """One level whose inputs take a gradient -> (g_pts, g_rays, g_dirs, the parameter gradients for autograd | None): the full
        backward when parameters take gradients too and the dgrad alone when they do not, then cnerf_mlp_input_grad on the workspace
        the dgrad wrote and the per-ray sums."""
        params, needs = job.params, job.needs
        ws = ops.mlp_bwd_workspace(job.spec, job.B, job.S, job.packed.device)
        grads, direct = None, False
        if any(needs[10:]):
            direct = _direct_ok(needs[10:], params) and _engine_accumulates(params[0])
            grads = ops.mlp_backward(job.spec, job.packed, job.d_raw, job.B, job.S, job.stash, grads=[p.grad for p in params] if direct else None,
                                     accumulate=direct and not _take_dropped(params), packed_bf=job.packed_bf, ws=ws)
            _report_ready([job.model], direct)
        else:
            ops.mlp_dgrad(job.spec, job.packed, job.d_raw, job.B, job.S, job.stash, ws, packed_bf=job.packed_bf)
        need_pts, need_rays, _, need_dirs = needs[3:7]
        vd = bool(job.spec.use_viewdirs)
        dirs_in_rows = vd and not job.dirs_given          # the view directions are the last three columns of the ray rows (R:350)
        d_pts, d_dirs_pt = ops.mlp_input_grad(job.spec, job.packed, job.B, job.S, job.stash, ws,
                                              want_dirs=vd and (need_dirs or (need_rays and dirs_in_rows)))
        g_pts = d_pts if need_pts else None
        g_rays = g_dirs = None
        if need_rays:
            g_rays = ops.rays_input_grad(d_pts, d_dirs_pt if dirs_in_rows else None, job.z, job.B, job.S, ray_stride=job.ray_stride)
        if need_dirs and vd:
            g_dirs = ops.rays_input_grad(None, d_dirs_pt, None, job.B, job.S)
        return g_pts, g_rays, g_dirs, (grads if grads is not None and not direct else None)


class _CompositeFn(torch.autograd.Function):
    """raw2outputs (R:265-308) and its backward."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays, noise, white_bkgd):
        if ctx.needs_input_grad[1]:   # (z is detached in the reference, R:397)
            raise ops.CnerfError("raw2outputs: gradients w.r.t. z_vals are not implemented (only w.r.t. raw and rays_d)")
        rgb, disp, acc, weights, depth = ops.composite_forward(raw, z_vals, rays, noise, white_bkgd)
        ctx.save_for_backward(raw, z_vals, rays)
        ctx.noise, ctx.white = noise, white_bkgd
        ctx.mark_non_differentiable(weights)
        ctx.set_materialize_grads(False)
        return rgb, disp, acc, weights, depth

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_weights, g_depth):
        raw, z_vals, rays = ctx.saved_tensors
        d_raw = ops.composite_backward(raw, z_vals, rays, ctx.noise, ctx.white, g_rgb, g_disp, g_acc, g_depth)
        # the rays enter through dists * |rays_d| only (R:283): that gradient follows from d_raw
        g_rays = ops.composite_norm_grad(d_raw, raw, ctx.noise, rays) if ctx.needs_input_grad[2] else None
        return d_raw, None, g_rays, None, None


class _PackRaysFn(torch.autograd.Function):
    """The non-NDC [B, 8|11] pack of render(rays=(rays_o, rays_d)) (R:97-125) when the rays take a gradient (a learnable pose):
    rows [o, d, near, far (, d / |d|)]; near and far are Python floats there and take none."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, near, far, use_viewdirs):
        ctx.save_for_backward(rays_d)
        ctx.use_viewdirs, ctx.shape_o = use_viewdirs, rays_o.shape
        return ops.pack_rays(rays_o, rays_d, near, far, use_viewdirs, False)

    @staticmethod
    def backward(ctx, g):
        rays_d, = ctx.saved_tensors
        d_o, d_d = ops.pack_rays_bwd(g, rays_d, ctx.use_viewdirs)
        return (d_o.reshape(ctx.shape_o) if ctx.needs_input_grad[0] else None,
                d_d.reshape(rays_d.shape) if ctx.needs_input_grad[1] else None, None, None, None)


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in ts)


def _norm_grad_levels(d_raw, raws, noises, rays):
    """The gradient of a folded loss w.r.t. the ray rows, which raw2outputs reads through dists * |rays_d| only (R:283): it follows
    from the d_raw the compositing-backward launches just produced, whatever the loss form.  Both levels: one launch that adds them
    (cnerf_composite_norm_grad_pair); one level with a d_raw: the single kernel; none: no gradient."""
    if d_raw[0] is not None and d_raw[1] is not None:
        return ops.composite_norm_grad_pair(d_raw[0], raws[0], noises[0], d_raw[1], raws[1], noises[1], rays)
    for lv in (0, 1):
        if d_raw[lv] is not None:
            return ops.composite_norm_grad(d_raw[lv], raws[lv], noises[lv], rays)
    return None


class _RenderLossFn(torch.autograd.Function):
    """raw2outputs of the LAST level (R:265-308) with the photometric loss of the training loop folded in (R:769-775):
    loss = img2mse(rgb_map, target) [+ img2mse(rgb0, target)] as ONE autograd node from (raw, raw_coarse) to the scalar.  Forward:
    the last level's compositing kernel also reduces the squared error and adds the coarse level's term (computed by ITS compositing
    launch, render_rays); backward: the two compositing-backward kernels form their seed (2 / n) (rgb - target) * g in registers.
    Gone from the step: two loss launches, their `+`, the two `d_x * g` of their backward.  The maps come back detached (values for
    logging, R:776): a caller that differentiates anything else of a map uses render() + img2mse()."""

    @staticmethod
    def forward(ctx, raw, raw_c, z, z_c, rays, noise, noise_c, white, target, rgb_c, loss_c):
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3] or ctx.needs_input_grad[8]:
            raise ops.CnerfError("render_loss: gradients w.r.t. z_vals / target are not implemented (only w.r.t. raw and the ray rows)")
        rgb, disp, acc, weights, depth, loss = ops.composite_forward_mse(raw, z, rays, noise, white, target, loss_add=loss_c)
        ctx.save_for_backward(raw, raw_c, z, z_c, rays, target, rgb, rgb_c)
        ctx.noise, ctx.noise_c, ctx.white = noise, noise_c, white
        ctx.mark_non_differentiable(rgb, disp, acc, weights, depth)
        ctx.set_materialize_grads(False)
        return loss.view(()), rgb, disp, acc, weights, depth

    @staticmethod
    def backward(ctx, g_loss, *_maps):
        raw, raw_c, z, z_c, rays, target, rgb, rgb_c = ctx.saved_tensors
        d_raw = [None, None]
        if g_loss is not None:
            for lv, (r, zv, nz, c) in enumerate(((raw, z, ctx.noise, rgb), (raw_c, z_c, ctx.noise_c, rgb_c))):      # fine, then coarse
                if r is not None and ctx.needs_input_grad[lv]:
                    d_raw[lv] = ops.composite_backward_mse(r, zv, rays, nz, ctx.white, c, target, g_loss)
        g_rays = _norm_grad_levels(d_raw, (raw, raw_c), (ctx.noise, ctx.noise_c), rays) if ctx.needs_input_grad[4] else None
        return tuple(d_raw) + (None, None, g_rays) + (None,) * 6


class _RenderClossFn(torch.autograd.Function):
    """raw2outputs of the LAST level with ConsistentNeRF's whole step loss folded in (V:1645-1865; ops.ClossSpec): ONE autograd node
    from (raw, raw_coarse) to the scalar.  Forward: the last level's compositing launch leaves its masked-loss partial sums (the
    coarse level's launch left its own, render_rays), cnerf_closs_finish sums both, evaluates the patch term of both levels and
    assembles the loss; backward: the two compositing-backward launches form their rgb / depth / patch seeds in registers.  Gone from
    the step: 2 masked-loss + 2 patch-term launches and the ~25 ATen kernels between them (adds, muls, index copies, fills).
    With a loss form (L.forms: the other live branches of V / VC, cnerf_lossform) the same three kinds of launch through the *_lossform
    entry points; `temps` = L.temps as autograd inputs: the softmask temperatures (temp_rgb, temp_depth, coarse temp_rgb, coarse
    temp_depth; None each), whose gradients the compositing-backward launches leave next to d_raw.
    With V's patch LPIPS term (L.lpips_P > 0): forward, the patches of BOTH levels packed into one batch, one LPIPS forward and the
    per-image values into the tail (ops.lpips_step_forward, ops.closs_finish); backward, the per-image seeds from g_loss, ONE LPIPS backward over the kept
    activations (here, with the real seeds: the arithmetic of lpips._LpipsFn under autograd), and the levels' compositing-backward
    launches read their slice of its NCHW gradient in place."""

    @staticmethod
    def forward(ctx, raw, raw_c, z, z_c, rays, noise, noise_c, white, L, rgb_c, depth_c, ws_c, *temps):
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            raise ops.CnerfError("render_loss: gradients w.r.t. z_vals are not implemented (only w.r.t. raw and the ray rows)")
        rgb, disp, acc, weights, depth, ws = ops.composite_forward_closs(raw, z, rays, noise, white, L)
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or (L.forms and any(ctx.needs_input_grad[12:]))
        ctx.n_temps = len(temps)
        lpips_v = lpips_ws = None
        if L.lpips_P > 0:
            lpips_v, lpips_ws = ops.lpips_step_forward(L, z.shape[0], rgb, rgb_c, want_grad=want)
        terms, stats, patch_d, ssim_d, d_temp = ops.closs_finish(L, z.shape[0], ws, ws_c, depth, depth_c, rgb, rgb_c, want_grad=want,
                                                                 lpips_v=lpips_v)
        ctx.save_for_backward(raw, raw_c, z, z_c, rays, rgb, rgb_c, depth, depth_c, stats, patch_d, ssim_d, d_temp, lpips_ws)
        ctx.noise, ctx.noise_c, ctx.white, ctx.L = noise, noise_c, white, L
        ctx.temp_shapes = [None if t is None else t.shape for t in temps]
        ctx.mark_non_differentiable(terms, rgb, disp, acc, weights, depth)
        ctx.set_materialize_grads(False)
        return terms[0], terms, rgb, disp, acc, weights, depth

    @staticmethod
    def backward(ctx, g_loss, *_rest):
        raw, raw_c, z, z_c, rays, rgb, rgb_c, depth, depth_c, stats, patch_d, ssim_d, d_temp, lpips_ws = ctx.saved_tensors
        d_raw = [None, None]
        g_temps = (None,) * ctx.n_temps
        if g_loss is not None:
            L = ctx.L
            w = stats.numel() // 2                   # the level's seed weights: 4, or 8 (two segments / a loss form), ops.ClossFinish
            want_t = L.forms and any(ctx.needs_input_grad[12:])
            g_temp = torch.empty(4, device=raw.device) if want_t else None   # written by the levels' backward launches
            pair = lambda x, lv: x[2 * lv:2 * lv + 2] if want_t else None  # noqa: E731   (the level's two temperatures)
            row = lambda x, lv: None if x is None else x[lv]  # noqa: E731                 (the level's row of a [levels, ..] tensor)
            ran = [False, False]
            lp = (None, None)
            if lpips_ws is not None and (ctx.needs_input_grad[0] or (raw_c is not None and ctx.needs_input_grad[1])):
                dX = ops.lpips_step_backward(L, lpips_ws, 2 if raw_c is not None else 1, g_loss)
                lp = (dX[:L.lpips_P], dX[L.lpips_P:] if raw_c is not None else None)
            levels = ((raw, z, ctx.noise, rgb, depth), (raw_c, z_c, ctx.noise_c, rgb_c, depth_c))      # the fine level's launch first
            for lv, (r, zv, nz, c, dp) in enumerate(levels):
                if r is not None and ctx.needs_input_grad[lv]:
                    d_raw[lv] = ops.composite_backward_closs(r, zv, rays, nz, ctx.white, L, c, dp, stats[lv * w:(lv + 1) * w], g_loss,
                                                             row(patch_d, lv), row(ssim_d, lv), lv, pair(d_temp, lv), pair(g_temp, lv),
                                                             lpips_dx=lp[lv])
                    ran[lv] = True
            if want_t:
                for lv in (0, 1):       # (a level whose raw takes no gradient had no launch to ride in)
                    if not ran[lv]:
                        g_temp[2 * lv:2 * lv + 2] = d_temp[2 * lv:2 * lv + 2] * g_loss
                g_temps = tuple(g_temp[k].reshape(ctx.temp_shapes[k]) if ctx.needs_input_grad[12 + k] else None
                                for k in range(ctx.n_temps))
        g_rays = _norm_grad_levels(d_raw, (raw, raw_c), (ctx.noise, ctx.noise_c), rays) if ctx.needs_input_grad[4] else None
        return tuple(d_raw) + (None, None, g_rays) + (None,) * 7 + g_temps


_ONES = {}


def backward(loss):
    """`loss.backward()` without the fill launch of its implicit ones_like seed: the seed is a cached device constant."""
    key = (str(loss.device), loss.dtype)
    one = _ONES.get(key)
    if one is None:
        one = torch.ones((), device=loss.device, dtype=loss.dtype)
        if not torch.cuda.is_current_stream_capturing():     # (a tensor allocated inside a recording belongs to the graph's pool)
            _ONES[key] = one
    torch.autograd.backward(loss, grad_tensors=one)


# ----------------------------------------------------------------------------- reference surface
def batchify(fn, chunk):
    """R:27-34.  Kept for API parity; the fused kernel tiles internally so chunking is a no-op."""
    if chunk is None:
        return fn

    def ret(inputs):
        return torch.cat([fn(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)
    return ret


def run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk=1024 * 64):
    """R:37-52.  inputs: [N_rays, N_samples, 3] tensor (or the lazy RayPoints render_rays passes);
    viewdirs: [N_rays, 3] or None.  embed_fn / embeddirs_fn only have to agree with the widths `fn` was
    built with (the encodings are generated inside the kernel); netchunk is advisory (results are
    chunk-invariant, R:79-80)."""
    if not isinstance(fn, NeRF):
        raise TypeError("run_network needs a consistentnerf_amd NeRF module")
    spec = fn.spec()
    if getattr(embed_fn, "out_dim", 3) != fn.input_ch:
        raise ValueError("embed_fn width does not match the network input_ch")
    if spec.use_viewdirs:
        if viewdirs is None:
            raise ValueError("network was built with use_viewdirs=True but viewdirs is None")
        if embeddirs_fn is not None and getattr(embeddirs_fn, "out_dim", 3) != fn.input_ch_views:
            raise ValueError("embeddirs_fn width does not match the network input_ch_views")
    B, S = inputs.shape[0], inputs.shape[1]
    dirs = viewdirs if (viewdirs is not None and spec.use_viewdirs) else None
    if dirs is not None and isinstance(inputs, RayPoints) and _is_viewdir_columns(dirs, inputs.rays):
        dirs = None      # the kernel reads the view directions from the last three columns of the ray rows (R:350): no copy
    elif dirs is not None:
        dirs = dirs.contiguous()
    params = fn.kernel_tensors()
    prec = getattr(fn, "inference_precision", "fp32")
    if prec != "fp32" and not (torch.is_grad_enabled() and any(p.requires_grad for p in params)):
        # OPT-IN reduced-precision inference (NeRF.inference_precision = "bf16" | "bf16x2" | "bf16x3" | "fp16x2"): bf16 / f16
        # matrix cores, fp32 accumulation; never taken when a gradient could be asked for.  `planes` is the mode's code in the
        # C ABI (fp16x2 has one of its own), which is also what keys the packed-panel cache: a change of mode re-packs
        if prec not in ops.PRECISION_PLANES:
            raise ValueError(f"inference_precision must be fp32 or one of {sorted(ops.PRECISION_PLANES)}")
        planes = ops.PRECISION_PLANES[prec]
        pk = _packed_bf(fn, planes)
        if isinstance(inputs, RayPoints):
            return ops.mlp_forward_bf(spec, pk, planes, B, S, rays=inputs.rays, z=inputs.z_vals, dirs=dirs)
        return ops.mlp_forward_bf(spec, pk, planes, B, S, pts=inputs.reshape(-1, 3).contiguous(), dirs=dirs)
    if not torch.is_grad_enabled():
        # under torch.no_grad() a Function still sees needs_input_grad = True for the parameters: detach them, or the
        # inference pass would run the training kernel and write a 10 KB-per-point stash nobody reads
        params = [p.detach() for p in params]
    if isinstance(inputs, RayPoints):
        return _MlpFn.apply(fn, B, S, None, inputs.rays, inputs.z_vals, dirs, None, getattr(inputs, "live", None),
                            getattr(inputs, "skip", 0), *params)
    pts = inputs.reshape(-1, 3).contiguous()
    return _MlpFn.apply(fn, B, S, pts, None, None, dirs, None, None, 0, *params)


def _is_viewdir_columns(viewdirs, rays):
    """True when `viewdirs` IS rays[:, -3:] (same storage): what render_rays passes (R:350)."""
    return (rays.dim() == 2 and rays.shape[1] >= 11 and viewdirs.dim() == 2 and viewdirs.shape == (rays.shape[0], 3)
            and viewdirs.dtype == rays.dtype and rays.is_contiguous() and viewdirs.stride() == (rays.shape[1], 1)
            and viewdirs.data_ptr() == rays.data_ptr() + 4 * (rays.shape[1] - 3))


def _jitter_and_u(rows, Nc, Nf, dev, global_rows):
    """The stratified-jitter stream t_rand [rows, Nc] (R:376) and the resampling stream u [rows, Nf] (H:227) of one render_rays
    call from ONE generator call: a flat draw cut into two contiguous blocks (one launch instead of two; with `global_rows` the
    draw is for the whole batch and this call's rows are sliced, _rows_of_global)."""
    off, total = (0, rows) if global_rows is None else (int(global_rows[0]), int(global_rows[1]))
    r = torch.rand(total * (Nc + Nf), device=dev)
    t_rand = r[:total * Nc].view(total, Nc)[off:off + rows]
    u = r[total * Nc:].view(total, Nf)[off:off + rows] if Nf > 0 else None
    return t_rand, u


def _in_kernel_rng():
    """The jitter / resampling streams are generated inside coarse_z_k / resample_k and the density noise by normal_rng_k
    (ops.rng_draw) — unless switched off, or a hipGraph is being recorded by something other than graph.GraphedStep (torch.rand /
    torch.randn are the graph-safe generators then)."""
    return ops.IN_KERNEL_RNG and (ops.RngCapture.active is not None or not torch.cuda.is_current_stream_capturing())


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False):
    """R:265-308 -> (rgb_map, disp_map, acc_map, weights, depth_map)."""
    B = z_vals.shape[0]
    rays = torch.cat([torch.zeros_like(rays_d), rays_d], -1).contiguous()
    if raw_noise_std > 0. and not pytest and _in_kernel_rng():     # its own block of offsets, the coarse level's stream (+2)
        noise = ops.density_noise(ops.rng_draw(raw.device), raw.shape[0], raw.shape[1], 0, raw_noise_std, raw.device)[0]
    else:
        noise = _density_noise(raw.shape[:2], raw_noise_std, pytest, raw.device)
    return _CompositeFn.apply(raw.contiguous(), z_vals.contiguous(), rays, noise, bool(white_bkgd))


def _rows_of_global(draw, rows, cols, global_rows):
    """`draw(n, cols)` for this call's `rows` rays — or, when the rays are rows [offset, offset + rows) of a GLOBAL batch of
    `total` rays sharded over ranks (`global_rows = (offset, total)`), the matching rows of the draw for the whole batch: every
    rank consumes the identical generator state for the identical global stream, so an N-rank step sees exactly the random
    numbers the 1-rank step on the whole batch sees ("t_rand / u generated from the global batch and sliced")."""
    if global_rows is None:
        return draw(rows, cols)
    off, total = global_rows
    return draw(int(total), cols)[int(off):int(off) + rows].contiguous()


def _pytest_rows(rows, cols, device, global_rows):
    """The reference's deterministic stream (np.random.seed(0); np.random.rand) for this call's rows — of the WHOLE batch when the
    rays are a shard of it, so that the shards see the rows the unsharded call sees."""
    if global_rows is None:
        return pytest_uniform((rows, cols), device)
    off, total = global_rows
    return pytest_uniform((int(total), cols), device)[int(off):int(off) + rows].contiguous()


def _density_noise(shape, raw_noise_std, pytest, device, global_rows=None):
    """The host-side density noise: the reference's uniform stream in pytest mode, torch.randn when the in-kernel streams are
    off (otherwise ops.density_noise draws both levels in one launch, render_rays)."""
    if not raw_noise_std > 0.:
        return None
    if pytest:   # R:290-294: uniform in pytest mode
        return _pytest_rows(shape[0], shape[1], device, global_rows) * raw_noise_std
    return _rows_of_global(lambda n, c: torch.randn(n, c, device=device), shape[0], shape[1], global_rows) * raw_noise_std


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """R:55-67."""
    all_ret = {}
    gr = kwargs.pop("_global_rows", None)
    if kwargs.get("_live") is not None and rays_flat.shape[0] > chunk:
        raise ops.CnerfError(f"_live needs the padded batch ({rays_flat.shape[0]} rows) to fit one chunk ({chunk})")
    if gr is not None and rays_flat.shape[0] > chunk:
        # every chunk would draw the whole batch's stream afresh, while the unsharded call draws one stream PER CHUNK: the
        # "N-rank step sees the 1-rank step's random numbers row for row" guarantee holds for shards that fit one chunk
        # (the training case: N_rand <= chunk)
        raise ops.CnerfError(f"_global_rows needs the shard ({rays_flat.shape[0]} rays) to fit one chunk ({chunk})")
    for i in range(0, rays_flat.shape[0], chunk):
        if gr is not None:     # this chunk's rows of the global batch
            kwargs["_global_rows"] = (gr[0] + i, gr[1])
        ret = render_rays(rays_flat[i:i + chunk], **kwargs)
        for k in ret:
            all_ret.setdefault(k, []).append(ret[k])
    return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}


def _rows_kwargs(rows, rays, kwargs, who="render_loss"):
    """render_loss(rows=...): the checked call -> the kwargs render() takes instead, with the rows as `_rows` (_render renders them
    as they are) and without ndc / near / far, which are baked into the rows."""
    if rays is not None or kwargs.get('c2w') is not None:
        raise ops.CnerfError(f"{who}: rows= is mutually exclusive with rays= and c2w= (the rows ARE the finished ray batch)")
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] not in (8, 11):
        raise ops.CnerfError(f"{who}: rows must be a [B, 8 | 11] tensor in batchify_rays' row format (pose.camera_rows)")
    vd = bool(kwargs.get('use_viewdirs', False))
    if rows.shape[1] != (11 if vd else 8):
        raise ops.CnerfError(f"{who}: rows of width {rows.shape[1]} with use_viewdirs={vd}: the rows carry the view directions in "
                             "three more columns (width 11) exactly when the networks read them")
    kw = {k: v for k, v in kwargs.items() if k not in ('ndc', 'near', 'far', 'c2w')}
    kw['_rows'] = rows
    return kw


def render_loss(H, W, K, target_s, chunk=1024 * 32, rays=None, rows=None, **kwargs):
    """R:764-775 as one call — `rgb, disp, acc, extras = render(H, W, K, chunk=, rays=batch_rays, retraw=True, **render_kwargs_train);
    img_loss = img2mse(rgb, target_s); loss = img_loss (+ img2mse(extras['rgb0'], target_s))` — with the loss folded into the
    compositing launches (_RenderLossFn).  -> (loss, rgb, disp, acc, extras); the same values and, after loss.backward() (or
    run_nerf.backward(loss): no seed fill), the same parameter gradients bit for bit as the lines above, from 6 launches fewer.
    The maps are detached.  Batches larger than `chunk`, or an empty one, take the lines above literally.
    rows= [B, 8 | 11] (instead of rays= / c2w=): the finished ray batch in batchify_rays' row format, normally pose.camera_rows(...)
    of learnable cameras; the width agrees with use_viewdirs.  `ndc` / `near` / `far` of the kwargs are already baked into the rows
    and are dropped.  Rows that require grad take their gradient on the same folded route: the two compositing-backward launches, one
    cnerf_composite_norm_grad_pair, the paired MLP backward, cnerf_mlp_input_grad_pair and cnerf_rays_input_grad_pair; parameter
    gradients do not depend on whether the rows require grad.  Batches beyond one chunk, empty ones and a target that is not on the
    device: batchify_rays(rows) + the lines above.  Not covered: all-reducing camera gradients across ranks, hipGraph capture of
    the pose step."""
    if rows is not None:
        kwargs = _rows_kwargs(rows, rays, kwargs)
    if rays is not None and _needs_grad(rays[0], rays[1]):
        raise ops.CnerfError("render_loss: gradients w.r.t. rays=(rays_o, rays_d) are not implemented on the folded-loss route; pass "
                             "the finished rows instead, render_loss(rows=pose.camera_rows(...)), or use render(rays=...) + img2mse")
    n = rows.shape[0] if rows is not None else rays[0].reshape(-1, 3).shape[0] if rays is not None else 0
    tgt = target_s.reshape(-1, 3) if torch.is_tensor(target_s) else None
    if ((rays is None and rows is None) or n == 0 or n > min(chunk, ops.composite_mse_max_rays()) or tgt is None or not tgt.is_cuda or tgt.dtype != torch.float32 or tgt.shape[0] != n
            or kwargs.get('c2w') is not None):
        rgb, disp, acc, extras = render(H, W, K, chunk=chunk, rays=rays, **kwargs)
        loss = img2mse(rgb, target_s)
        if 'rgb0' in extras:
            loss = loss + img2mse(extras['rgb0'], target_s)
        return loss, rgb, disp, acc, extras
    rgb, disp, acc, extras = render(H, W, K, chunk=chunk, rays=rays, _target=tgt.contiguous(), **kwargs)
    return extras.pop('loss'), rgb, disp, acc, extras


def _ray_batch(H, W, K, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, device):
    """R:97-125 -> (rays [B, 8|11], output leading shape)."""
    coef = ndc_coefficients(H, W, K[0][0]) if ndc else (0., 0.)
    # per-ray tensor bounds are written after the pack (R:111 `near * ones` takes any mix of scalars and tensors)
    near_s = 0. if torch.is_tensor(near) else near
    far_s = 1. if torch.is_tensor(far) else far
    if c2w is not None:
        sh = (H, W)
        if c2w_staticcam is not None and use_viewdirs:
            # viewdirs from c2w, geometry from the static camera (R:104-108)
            vd = ops.gen_rays(H, W, K, c2w, near_s, far_s, True, False, device)[:, 8:11]
            batch = ops.gen_rays(H, W, K, c2w_staticcam, near_s, far_s, True, ndc, device, coef)
            batch[:, 8:11] = vd
        else:
            batch = ops.gen_rays(H, W, K, c2w, near_s, far_s, use_viewdirs, ndc, device, coef)
    else:
        pk = getattr(rays, "_cnerf_packed", None)
        if pk is not None and pk.matches(H, W, K, near, far, use_viewdirs, ndc, device, src=rays if torch.is_tensor(rays) else None):
            # raybank's one-launch sampler already wrote the [B, 8|11] rows this call would assemble (same arithmetic: raygen.hpp)
            return pk.rows, (pk.rows.shape[0],)
        rays_o, rays_d = rays
        sh = tuple(rays_d.shape[:-1])
        if _needs_grad(rays_o, rays_d):      # rays of a learnable pose: the pack as an autograd node
            if ndc:
                raise ops.CnerfError("render(rays=..., ndc=True): gradients w.r.t. rays through the NDC warp are not implemented "
                                     "here (ndc=False has them) — build the NDC rows from the pose with pose.camera_rows(..., "
                                     "ndc=True) and pass them to batchify_rays")
            batch = _PackRaysFn.apply(rays_o.to(device=device, dtype=torch.float32), rays_d.to(device=device, dtype=torch.float32),
                                      near_s, far_s, bool(use_viewdirs))
        else:
            batch = ops.pack_rays(rays_o.to(device), rays_d.to(device), near_s, far_s, use_viewdirs, ndc, coef)
    if torch.is_tensor(near):
        batch[:, 6] = near.reshape(-1).to(batch)
    if torch.is_tensor(far):
        batch[:, 7] = far.reshape(-1).to(batch)
    return batch, sh


def _default_device():
    if not torch.cuda.is_available():
        raise ops.CnerfError("consistentnerf_amd needs an MI355X (no CPU execution path)")
    return torch.device("cuda", torch.cuda.current_device())


def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, **kwargs):
    """R:70-137 -> [rgb_map, disp_map, acc_map, extras]."""
    return _render(H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, False, kwargs)


def _camera_path_ok(rays, c2w, near, far, use_viewdirs, c2w_staticcam, kwargs):
    """render(c2w=...) of a whole image for inference can generate its rays inside the kernels (cnerf_render_fwd_cam):
    that needs the stock network_query_fn of create_nerf (the kernels ARE that query), scalar near / far, no static
    camera, and no autograd graph to build."""
    net, fine = kwargs.get("network_fn"), kwargs.get("network_fine")
    if rays is not None or c2w is None or c2w_staticcam is not None or torch.is_tensor(near) or torch.is_tensor(far):
        return False
    if not getattr(kwargs.get("network_query_fn"), "_cnerf_stock", False) or not isinstance(net, NeRF):
        return False
    if fine is not None and not isinstance(fine, NeRF):
        return False
    if DEBUG:            # the ray-tensor path carries render_rays' NaN / Inf report (R:417-419)
        return False
    nets = [net] + ([fine] if fine is not None else [])
    if any(bool(n.use_viewdirs) != bool(use_viewdirs) for n in nets):
        return False
    if any(getattr(n, "inference_precision", "fp32") != "fp32" for n in nets):   # the camera path is the exact-fp32 one
        return False
    return not (torch.is_grad_enabled() and any(p.requires_grad for n in nets for p in n.parameters()))


def camera_path_ok(c2w, render_kwargs):
    """True when render(c2w=..., **render_kwargs) would take the in-kernel camera path (distributed.render_image_sharded asks
    before calling render_pixels)."""
    kw = dict(render_kwargs)
    near, far = kw.pop("near", 0.), kw.pop("far", 1.)
    return _camera_path_ok(None, c2w, near, far, kw.pop("use_viewdirs", False), kw.pop("c2w_staticcam", None), kw)


def render_pixels(H, W, K, chunk, c2w, first, count, ndc=True, near=0., far=1., use_viewdirs=False, with_depth=False, **kwargs):
    """The pixels [first, first + count) (row-major) of the image render(H, W, K, c2w=c2w, ...) would produce, as flat
    per-ray maps {rgb_map [count, 3], disp_map [count], acc_map [count], ...}: the row block of one rank of a sharded frame
    (distributed.render_image_sharded).  Inference only, stock network_query_fn only (camera_path_ok); the rays are generated
    inside the kernels, and every pixel equals the one of the full-frame render bit for bit (rays are independent; chunk
    boundaries do not matter, R:79-80) as long as no per-call random stream is involved (perturb = 0, raw_noise_std = 0)."""
    if isinstance(c2w, torch.Tensor):
        c2w = c2w[:3, :4]
    if not _camera_path_ok(None, c2w, near, far, use_viewdirs, None, kwargs):
        raise ops.CnerfError("render_pixels needs the in-kernel camera path (stock network_query_fn, scalar near / far, "
                             "no autograd graph)")
    return _render_camera(H, W, K, chunk, c2w, ndc, near, far, use_viewdirs, with_depth, kwargs, int(first), int(count))


def _render_camera(H, W, K, chunk, c2w, ndc, near, far, use_viewdirs, with_depth, kwargs, first0=0, count=None):
    """batchify_rays (R:55-67) + render_rays (R:311-421) over the image of one camera (or its pixels [first0, first0 +
    count)), rays generated in-kernel: one C call per chunk, the same random streams in the same order as the ray-tensor
    path (bit-identical results)."""
    net, fine = kwargs["network_fn"], kwargs.get("network_fine")
    Nc, Nf = kwargs["N_samples"], kwargs.get("N_importance", 0)
    perturb, pytest = kwargs.get("perturb", 0.), kwargs.get("pytest", False)
    std, dev = kwargs.get("raw_noise_std", 0.), next(net.parameters()).device
    coef = ndc_coefficients(H, W, K[0][0]) if ndc else (0., 0.)
    two_nets = fine is not None and Nf > 0
    if isinstance(c2w, torch.Tensor):     # ONE device-to-host copy of the 12 pose floats per frame, not one per chunk
        c2w = c2w.detach().cpu().numpy()
    all_ret = {}
    end = H * W if count is None else min(H * W, first0 + count)
    for first in range(first0, end, chunk):
        B = min(chunk, end - first)
        t_rand = u = rng = None
        ik_noise = std > 0. and not pytest and _in_kernel_rng()
        if perturb > 0.:
            if pytest:
                t_rand = pytest_uniform((B, Nc), dev)
            elif _in_kernel_rng():
                # the streams render_rays' kernels generate for the same generator state, materialised (this C call takes tensors)
                rng = ops.rng_draw(dev)
                t_rand = ops.uniform_rng(rng, B, Nc, dev, 0)
                u = ops.uniform_rng(rng, B, Nf, dev, 1) if Nf > 0 else None
            else:
                t_rand, u = _jitter_and_u(B, Nc, Nf, dev, None)     # (the same draw as render_rays: bit-identical paths)
        if ik_noise:   # both levels from one launch, on the block of the jitter (render_rays does the same)
            noise0, noise1 = ops.density_noise(rng if rng is not None else ops.rng_draw(dev), B, Nc, Nc + Nf if Nf > 0 else 0, std, dev)
        else:
            noise0 = _density_noise((B, Nc), std, pytest, dev)
        if u is None:
            u = sample_u(B, Nf, perturb == 0., pytest, dev) if Nf > 0 else None
        if not ik_noise:
            noise1 = _density_noise((B, Nc + Nf), std, pytest, dev) if Nf > 0 else None
        if two_nets:
            _prepack_pair(net, fine)
        o = ops.render_forward_cam(net.spec(), _packed(net), fine.spec() if two_nets else None,
                                   _packed(fine) if two_nets else None, H, W, K, c2w, near, far, use_viewdirs, ndc, coef, first,
                                   B, Nc, Nf, t_rand, u, noise0, noise1, bool(kwargs.get("lindisp", False)),
                                   bool(kwargs.get("white_bkgd", False)), bool(kwargs.get("retraw", False)))
        if not with_depth:
            o.pop("depth_map", None)
            o.pop("depth0", None)
        for k, v in o.items():
            all_ret.setdefault(k, []).append(v)
    return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}


def _render(H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, with_depth, kwargs):
    net = kwargs.get("network_fn")
    device = next(net.parameters()).device if net is not None else _default_device()
    rows = kwargs.get("_rows")
    if rows is not None:       # render_loss(rows=...): the finished [B, 8 | 11] batch, rendered as it is (_rows_kwargs checked it)
        kwargs = {k: v for k, v in kwargs.items() if k != "_rows"}
        if rows.device != device or rows.dtype != torch.float32:
            rows = rows.to(device=device, dtype=torch.float32)
        return _render_batch(rows, (rows.shape[0],), chunk, with_depth, kwargs)
    if _needs_grad(c2w):
        raise ops.CnerfError("render(c2w=...) with c2w requiring grad: gradients w.r.t. a camera pose are not implemented — build "
                             "the rays from the pose with get_rays and pass render(rays=(rays_o, rays_d), ndc=False), or, with "
                             "ndc=True or a learnable K, the rows with pose.camera_rows and pass them to batchify_rays")
    if _needs_grad(c2w_staticcam):
        raise ops.CnerfError("render(c2w_staticcam=...) requiring grad: gradients w.r.t. the static camera are not implemented — "
                             "pose.camera_rows + batchify_rays take a pose that requires grad")
    if _camera_path_ok(rays, c2w, near, far, use_viewdirs, c2w_staticcam, kwargs):
        kw = {k: v for k, v in kwargs.items()}
        all_ret = _render_camera(H, W, K, chunk, c2w, ndc, near, far, use_viewdirs, with_depth, kw)
        for k in all_ret:
            all_ret[k] = torch.reshape(all_ret[k], [H, W] + list(all_ret[k].shape[1:]))
        k_extract = ['rgb_map', 'disp_map', 'acc_map'] + (['depth_map'] if with_depth else [])
        return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]
    batch, sh = _ray_batch(H, W, K, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, device)
    return _render_batch(batch, sh, chunk, with_depth, kwargs)


def _render_batch(batch, sh, chunk, with_depth, kwargs):
    """batchify_rays over the [B, 8 | 11] rows and render()'s result structure (R:127-137)."""
    all_ret = batchify_rays(batch, chunk, _with_depth=with_depth, **kwargs)
    for k in all_ret:
        if k not in ('loss', 'loss_terms'):          # (the scalars of render_loss pass through)
            all_ret[k] = torch.reshape(all_ret[k], list(sh) + list(all_ret[k].shape[1:]))
    k_extract = ['rgb_map', 'disp_map', 'acc_map'] + (['depth_map'] if with_depth else [])
    ret_list = [all_ret[k] for k in k_extract]
    ret_dict = {k: all_ret[k] for k in all_ret if k not in k_extract}
    return ret_list + [ret_dict]


def render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0):
    """R:140-178 -> (rgbs, disps) numpy."""
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    rgbs, disps = [], []
    t = time.time()
    for i, c2w in enumerate(render_poses):
        print(i, time.time() - t)
        t = time.time()
        with torch.no_grad():
            rgb, disp, acc, _ = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)
        rgbs.append(rgb.cpu().numpy())
        disps.append(disp.cpu().numpy())
        if i == 0:
            print(rgb.shape, disp.shape)
        if savedir is not None:
            _save_png(os.path.join(savedir, '{:03d}.png'.format(i)), to8b(rgbs[-1]))
    return np.stack(rgbs, 0), np.stack(disps, 0)


def _save_png(path, img8):
    try:
        import imageio
        imageio.imwrite(path, img8)
    except ImportError:   # image IO is outside the hot path; keep the render usable without imageio
        np.save(path + ".npy", img8)


def save_checkpoint(basedir, expname, global_step, render_kwargs_train, optimizer):
    """The checkpoint write of train() (R:836-845): `{basedir}/{expname}/{global_step:06d}.tar` with the reference's
    keys, loadable by the reference and by create_nerf() here."""
    path = os.path.join(basedir, expname, '{:06d}.tar'.format(global_step))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    fine = render_kwargs_train.get('network_fine')
    ckpt = {'global_step': global_step,
            'network_fn_state_dict': render_kwargs_train['network_fn'].state_dict(),
            'optimizer_state_dict': optimizer.state_dict()}
    if fine is not None:
        ckpt['network_fine_state_dict'] = fine.state_dict()
    torch.save(ckpt, path)
    print('Saved checkpoints at', path)
    return path


def create_nerf(args):
    """R:181-262 -> (render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer)."""
    return _create_nerf(args, NeRF, False)


def _create_nerf(args, model_cls, view_variant):
    device = _default_device()
    embed_fn, input_ch = get_embedder(args.multires, args.i_embed)
    input_ch_views, embeddirs_fn = 0, None
    if args.use_viewdirs:
        embeddirs_fn, input_ch_views = get_embedder(args.multires_views, args.i_embed)
    output_ch = 5 if args.N_importance > 0 else 4
    skips = [4]
    extra = dict(coarse=True, stable_init=getattr(args, "stable_init", False)) if view_variant else {}
    model = model_cls(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=skips,
                      input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs, **extra).to(device)
    grad_vars = list(model.parameters())
    model_fine = None
    if args.N_importance > 0:
        extra_f = dict(stable_init=getattr(args, "stable_init", False)) if view_variant else {}
        model_fine = model_cls(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch,
                               skips=skips, input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs,
                               **extra_f).to(device)
        grad_vars += list(model_fine.parameters())
    if view_variant:   # V:321: the coarse net starts as a copy of the fine net
        model.load_state_dict(model_fine.state_dict())

    def network_query_fn(inputs, viewdirs, network_fn):
        return run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn,
                           netchunk=args.netchunk)

    network_query_fn._cnerf_stock = True     # render(c2w=...) may replace it by the single-call camera path
    optimizer = FusedAdam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start = 0
    basedir, expname = args.basedir, args.expname
    if args.ft_path is not None and args.ft_path != 'None':
        ckpts = [args.ft_path]
    else:
        d = os.path.join(basedir, expname)
        ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if 'tar' in f] if os.path.isdir(d) else []
    print('Found ckpts', ckpts)
    if len(ckpts) > 0 and not args.no_reload:
        ckpt_path = ckpts[-1]
        print('Reloading from', ckpt_path)
        ckpt = torch.load(ckpt_path, map_location=device, weights_only=False)
        start = ckpt['global_step']
        if not view_variant:      # V:351 skips the optimizer reload
            optimizer.load_state_dict(ckpt['optimizer_state_dict'])
        sd_c, sd_f = ckpt['network_fn_state_dict'], ckpt.get('network_fine_state_dict')
        if view_variant:          # V:353-358 resets the three scalars
            for sd in (sd_c, sd_f):
                if sd is not None:
                    for k in ('temp_rgb', 'temp_depth', 'depth_scale'):
                        sd[k] = torch.full((1,), 0.1, device=device)
        model.load_state_dict(sd_c)
        if model_fine is not None and sd_f is not None:
            model_fine.load_state_dict(sd_f)
    render_kwargs_train = {
        'network_query_fn': network_query_fn, 'perturb': args.perturb, 'N_importance': args.N_importance,
        'network_fine': model_fine, 'N_samples': args.N_samples, 'network_fn': model,
        'use_viewdirs': args.use_viewdirs, 'white_bkgd': args.white_bkgd, 'raw_noise_std': args.raw_noise_std,
    }
    if args.dataset_type != 'llff' or args.no_ndc:
        print('Not ndc!')
        render_kwargs_train['ndc'] = False
        render_kwargs_train['lindisp'] = args.lindisp
    render_kwargs_test = {k: render_kwargs_train[k] for k in render_kwargs_train}
    render_kwargs_test['perturb'] = False
    render_kwargs_test['raw_noise_std'] = 0.
    return render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer


def _random_streams(rows, Nc, Nf, perturb, raw_noise_std, pytest, dev, global_rows):
    """Every random stream of one render_rays call, decided in one place -> (t_rand | None, rng | None, u(), noise(level)).
    t_rand: the jitter as a tensor (pytest; torch.rand when the in-kernel streams are off) and rng: the block of in-kernel stream
    offsets (ops.rng_draw: jitter +0, u +1, noise +2 / +3) are taken here.  u() -> the resampling stream (None: generated inside
    resample_k) and noise(level) -> the density noise of level 0 (coarse) / 1 (fine) or None draw where render_rays calls them — u()
    after the coarse level, noise() once per level, coarse first — so the calls on torch's generator keep the reference's order."""
    in_kernel = _in_kernel_rng()
    row0 = 0 if global_rows is None else int(global_rows[0])
    t_rand = u_drawn = rng = rng_noise = None
    if perturb > 0.:
        if pytest:
            t_rand = _pytest_rows(rows, Nc, dev, global_rows)
        elif in_kernel:
            # no generator launch: both streams are generated where they are consumed, indexed by the GLOBAL row (a shard of a
            # batch sees the rows the unsharded call sees without drawing the whole batch's stream)
            rng = ops.rng_draw(dev, row0)
        else:
            t_rand, u_drawn = _jitter_and_u(rows, Nc, Nf, dev, global_rows)
    if raw_noise_std > 0. and not pytest and in_kernel:
        # the density noise of both levels: one launch on the SAME block of offsets (+2, +3), so the call still advances the
        # generator by RNG_STRIDE; without jitter the block is reserved for the noise alone
        rng_noise = rng if rng is not None else ops.rng_draw(dev, row0)
    both = []

    def noise(level):
        if rng_noise is None:
            return _density_noise((rows, Nc + Nf if level else Nc), raw_noise_std, pytest, dev, global_rows)
        if not both:
            both.extend(ops.density_noise(rng_noise, rows, Nc, Nc + Nf if Nf > 0 else 0, raw_noise_std, dev))
        return both[level]

    def u():
        if rng is not None or u_drawn is not None:     # inside resample_k / drawn together with the jitter (one generator call)
            return u_drawn
        if perturb == 0.:                              # H:221 det = perturb == 0
            return sample_u(rows, Nf, True, pytest, dev)
        if pytest:
            return _pytest_rows(rows, Nf, dev, global_rows)
        return _rows_of_global(lambda n, c: torch.rand(n, c, device=dev), rows, Nf, global_rows)    # (perturb < 0 too: no jitter)
    return t_rand, rng, u, noise


def _coarse_coins_off(L):
    """VT:959 / VT:966 with both coarse coins 0: no primary term depends on the coarse network (its colour term falls back to the
    FINE rgb, its depth term is absent)."""
    return L.ss_coins is not None and not (L.ss_coins[2] or (L.prior is not None and L.ss_coins[3]))


def _composite_level(raw, z, rays, noise, white, target, coarse_of_two, below=(None,) * 6, temps=()):
    """raw2outputs of one level under the call's loss fold (target: None, the MSE target or a checked ops.ClossSpec) ->
    (loss, terms, (rgb, disp, acc, depth), weights, carry).  The coarse level of two: its loss term (MSE) / partial sums (ClossSpec)
    ride in its compositing launch and come back as `carry`; the autograd node comes with the last level, which takes
    below = (raw, z, noise, rgb, depth, carry) of that coarse level."""
    loss = terms = carry = None
    closs = isinstance(target, ops.ClossSpec)
    if target is None:
        rgb, disp, acc, weights, depth = _CompositeFn.apply(raw, z, rays, noise, white)
    elif coarse_of_two and closs:
        rgb, disp, acc, weights, depth, carry = ops.composite_forward_closs(raw, z, rays, noise, white, target, level=1)
    elif coarse_of_two:
        rgb, disp, acc, weights, depth, carry = ops.composite_forward_mse(raw, z, rays, noise, white, target)
    else:
        raw_c, z_c, noise_c, rgb_c, depth_c, carry_c = below
        if closs:
            loss, terms, rgb, disp, acc, weights, depth = _RenderClossFn.apply(raw, raw_c, z, z_c, rays, noise, noise_c, white, target,
                                                                               rgb_c, depth_c, carry_c, *temps)
        else:
            loss, rgb, disp, acc, weights, depth = _RenderLossFn.apply(raw, raw_c, z, z_c, rays, noise, noise_c, white, target, rgb_c,
                                                                       carry_c)
    return loss, terms, (rgb, disp, acc, depth), weights, carry


def _ray_results(last, coarse, z_std, raw, retraw, with_depth, loss=None, terms=None):
    """render_rays' dict from (rgb, disp, acc, depth) of the last level and of the coarse level of two (None: one level)."""
    ret = {'rgb_map': last[0], 'disp_map': last[1], 'acc_map': last[2]}
    if loss is not None:
        ret['loss'] = loss
    if terms is not None:
        ret['loss_terms'] = terms
    if with_depth:
        ret['depth_map'] = last[3]
    if retraw:
        ret['raw'] = raw
    if coarse is not None:
        ret['rgb0'], ret['disp0'], ret['acc0'] = coarse[:3]
        if with_depth:
            ret['depth0'] = coarse[3]
        ret['z_std'] = z_std
    return ret


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, retraw=False, lindisp=False, perturb=0.,
                N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0., verbose=False, pytest=False,
                _with_depth=False, _debug=False, _global_rows=None, _target=None, _live=None):
    """R:311-421 (V:441-551 when _with_depth).  Returns the same dict (+ the sample depths when _debug).
    `_global_rows = (offset, total)`: `ray_batch` is rows [offset, offset + N_rays) of a global batch of `total` rays sharded over
    ranks — the in-kernel jitter / resampling / noise streams are indexed by the global row (a shard draws its own rows only); the
    host-side streams (pytest, ops.IN_KERNEL_RNG off) are drawn for the whole batch and sliced (_rows_of_global).
    `_target` [N_rays, 3] (render_loss): the compositing launches also produce ret['loss'] = img2mse(rgb_map, _target)
    (+ img2mse(rgb0, _target) with two levels) through _RenderLossFn; the maps are then detached values.
    `_live` (device int32 [1]): `ray_batch` is padded to a fixed capacity, only its first _live[0] rows are real rays (the rest are
    valid dummy rays whose loss weight is 0): the MLP training kernels stop at the count, which never visits the host."""
    rays = ray_batch if ray_batch.is_contiguous() else ray_batch.contiguous()
    N_rays, dev = rays.shape[0], rays.device
    if _needs_grad(rays) and _live is not None:
        raise ops.CnerfError("render_rays: gradients w.r.t. rays are not implemented for a `live` batch (ss_step_loss); use "
                             "render_loss(rows=...) or render(rays=...) and form the loss from its maps")
    two = N_importance > 0
    if N_rays == 0:   # nothing to launch (the reference's batchify_rays raises on an empty batch; here: empty maps)
        last = network_fn if (network_fine is None or not two) else network_fine
        maps = lambda: tuple(torch.empty(*sh, device=dev) for sh in ((0, 3), (0,), (0,), (0,)))  # noqa: E731
        return _ray_results(maps(), maps() if two else None, torch.empty(0, device=dev),
                            torch.empty(0, N_samples + N_importance, last.spec().raw_ch, device=dev) if retraw else None, retraw, _with_depth)
    viewdirs = rays[:, -3:] if rays.shape[-1] > 8 else None
    t_rand, rng, draw_u, draw_noise = _random_streams(N_rays, N_samples, N_importance, perturb, raw_noise_std, pytest, dev, _global_rows)
    z_vals = ops.coarse_z(rays, N_samples, t_rand, lindisp, rng=rng)
    if two:
        _prepack_pair(network_fn, network_fine)
    # the loss fold of the call: none (_target None), the MSE target, or the whole ConsistentNeRF step loss (ops.ClossSpec)
    closs = isinstance(_target, ops.ClossSpec)
    skip_c, form_temps = 0, ()
    if closs:
        if _live is not None and _target.seg_row and two and _coarse_coins_off(_target):
            skip_c = int(_target.seg_row)        # the coarse level's backward covers the second segment only
        form_temps = (_target.temps or ()) if _target.forms else ()    # autograd inputs: checked() below detaches nothing, but
        _target = _target.checked(N_rays)                              # the node must see the caller's own tensors
    white = bool(white_bkgd)
    raw = network_query_fn(RayPoints(rays, z_vals, _live, skip_c), viewdirs, network_fn)
    noise = draw_noise(0)
    loss, terms, maps, weights, carry = _composite_level(raw, z_vals, rays, noise, white, _target, two, temps=form_temps)
    z_coarse, maps_0, z_std = z_vals, None, None
    if two:
        maps_0, raw_coarse, noise_coarse = maps, raw, noise
        z_vals, z_std = ops.resample(z_coarse, weights, draw_u(), rng=rng, Nf=N_importance)   # R:395-399 + R:415, no gradient (R:397)
        raw = network_query_fn(RayPoints(rays, z_vals, _live), viewdirs, network_fn if network_fine is None else network_fine)
        _link_levels(raw_coarse, raw)
        noise = draw_noise(1)
        # as in the reference's graph, a coarse level that no term of this render reaches has no backward at all (left attached, its
        # dgrad + wgrad would run on zero seeds: 16 % of the step for nothing).  (Not in the one-render form of the step, seg_row > 0:
        # the second render's coarse terms always reach the coarse network.)
        detach = closs and not _target.seg_row and _coarse_coins_off(_target)
        loss, terms, maps, weights, _ = _composite_level(
            raw, z_vals, rays, noise, white, _target, False,
            (raw_coarse.detach() if detach else raw_coarse, z_coarse, noise_coarse, maps_0[0], maps_0[3], carry), form_temps)
    ret = _ray_results(maps, maps_0, z_std, raw, retraw, _with_depth, loss, terms)
    if _debug:
        ret['_z_coarse'], ret['_z_vals'], ret['_weights'] = z_coarse, z_vals, weights
        if two:
            ret['_raw_coarse'] = raw_coarse
    if DEBUG:
        for k in ret:
            if torch.isnan(ret[k]).any() or torch.isinf(ret[k]).any():
                print(f"! [Numerical Error] {k} contains nan or inf.")
    return ret
