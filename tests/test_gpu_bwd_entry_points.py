"""The 14 exported forms of the MLP backward (include/cnerf.h: cnerf_mlp_{bwd,dgrad,wgrad} x {"", _pair, _live, _pair_live, _bf,
_bf_pair}), called through the C ABI.  They are one host path behind different argument lists, so the forms must agree with each
other BIT FOR BIT (torch.equal, no tolerance anywhere in this file):

  combined = halves      cnerf_mlp_bwd* equals its dgrad + wgrad halves, overwriting and accumulating
  pair = two singles     the bf16x3 pair forms equal two single bf16x3 calls
  rows outside a launch  with a device-side live count and first_ray, every d_raw / stash row the launch leaves out may hold NaN:
                         this pins the operand offsets (a wrong one reads a poisoned row, or memory that is not the caller's)
  merged = separate      cnerf_mlp_bwd_live per network equals cnerf_mlp_bwd_pair_live with first_ray = 0 (the wgrad range count
                         depends on the network's own point count only, csrc/wgrad.hip plan_ranges)

Live is never compared with non-live on a truncated batch: those differ by the association of the point ranges.
Workspaces are handed over full of NaN: no form may read a workspace word it did not write."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import T, dev, make_model  # noqa: F401  (dev: the module's device fixture)

pytestmark = pytest.mark.gpu

VD64, VD128, NOVD64, VD256 = (2, 64, True), (4, 128, True), (2, 64, False), (2, 256, True)


class _Level:
    """One network with a training stash of M points and a seed gradient d_raw[M, raw_ch]."""

    def __init__(self, dev, arch, seed, M):
        from consistentnerf_amd import ops
        D, W, vd = arch
        model, _ = make_model(D, W, vd, 5, seed, dev)
        self.spec, self.M, self.dev = model.spec(), M, dev
        self.net = self.spec.c()
        self.params = model.kernel_tensors()
        self.packed = ops.pack_weights(self.spec, self.params)
        rs = np.random.RandomState(seed)
        pts = T(rs.uniform(-2, 2, size=(M, 3)).astype(np.float32), dev)
        dirs = T(rs.normal(size=(M, 3)).astype(np.float32), dev) if vd else None
        raw, self.stash = ops.mlp_forward(self.spec, self.packed, M, 1, pts=pts, dirs=dirs, want_stash=True)
        self.d_raw = T(rs.normal(size=(M, self.spec.raw_ch)).astype(np.float32), dev)
        self.s_rows = self.stash.numel() // ((M + 31) // 32 * 32)

    @functools.cached_property
    def packed_bf(self):
        from consistentnerf_amd import ops
        return ops.pack_weights_bf(self.spec, self.params, 3)


@functools.lru_cache(maxsize=None)
def _level(dev, arch, seed, M):
    return _Level(dev, arch, seed, M)


def _backward(levels, shapes, halves, accumulate, live=None, first=None, bf=False, d_raw=None, stash=None):
    """Runs one form over `levels` (one or two _Level) at shapes [(B, S)] and returns the gradients, one list per level.
    halves: the dgrad + wgrad entry points instead of the combined one.  live: device int32 count (the _live forms); first: the
    pair-live first_ray pair.  d_raw / stash: per-level replacements of the level's own."""
    from consistentnerf_amd import _lib, ops
    lib, n = _lib.load(), len(levels)
    d_raw = d_raw or [lv.d_raw for lv in levels]
    stash = stash or [lv.stash for lv in levels]
    grads = [[torch.full(s, 7.0, device=lv.dev) for s in lv.spec.tensor_shapes()] for lv in levels]
    ptrs = [ops._ptrs(g) for g in grads]
    ws = [torch.full((lib.cnerf_mlp_bwd_ws_floats(C.byref(lv.net), B * S),), float("nan"), device=lv.dev)
          for lv, (B, S) in zip(levels, shapes)]
    p = ops._p
    dg = [[C.byref(lv.net), p(lv.packed_bf if bf else lv.packed), p(d_raw[i]), B, S, p(stash[i]), p(ws[i])]
          for i, (lv, (B, S)) in enumerate(zip(levels, shapes))]
    wg = [[C.byref(lv.net), B, S, p(stash[i]), p(ws[i]), C.byref(ptrs[i])] for i, (lv, (B, S)) in enumerate(zip(levels, shapes))]
    tail = ([p(live)] if live is not None else []) + (list(first) if first is not None else [])
    sfx = ("_bf" if bf else "") + ("_pair" if n == 2 else "") + ("_live" if live is not None else "")

    def call(name, per_level, extra):
        rc = getattr(lib, name)(*[a for lv in per_level for a in lv], *extra, ops._stream())
        assert rc == 0, (name, rc)

    if halves:
        call("cnerf_mlp_dgrad" + sfx, dg, tail)
        call("cnerf_mlp_wgrad" + sfx, wg, [int(accumulate)] + tail)
    else:
        call("cnerf_mlp_bwd" + sfx, [d + [w[-1]] for d, w in zip(dg, wg)], [int(accumulate)] + tail)
    return grads


def _same(a, b):
    for ga, gb in zip(a, b):
        assert len(ga) == len(gb)
        for i, (x, y) in enumerate(zip(ga, gb)):
            assert torch.isfinite(x).all(), f"tensor {i} is not finite"
            assert torch.equal(x, y), f"tensor {i} differs"


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M", [33, 128])
@pytest.mark.parametrize("arch", [VD64, VD128, NOVD64])
def test_bwd_equals_dgrad_plus_wgrad(dev, arch, M, accumulate):
    lv = [_level(dev, arch, 71, M)]
    _same(_backward(lv, [(M, 1)], False, accumulate), _backward(lv, [(M, 1)], True, accumulate))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("arch0,arch1", [(VD64, VD64), (VD64, VD128), (NOVD64, NOVD64)])
def test_bwd_pair_equals_dgrad_pair_plus_wgrad_pair(dev, arch0, arch1, accumulate):
    lv, sh = [_level(dev, arch0, 71, 33), _level(dev, arch1, 72, 128)], [(33, 1), (128, 1)]
    _same(_backward(lv, sh, False, accumulate), _backward(lv, sh, True, accumulate))


LIVE_B, LIVE_S, LIVE_N = 4, (32, 64), 3      # capacity in rays, points per ray of level 0 / 1, live rays


def _live_pair(dev, arch0, arch1):
    lv = [_level(dev, arch0, 71, LIVE_B * LIVE_S[0]), _level(dev, arch1, 72, LIVE_B * LIVE_S[1])]
    return lv, [(LIVE_B, LIVE_S[0]), (LIVE_B, LIVE_S[1])], torch.tensor([LIVE_N], device=dev, dtype=torch.int32)


def _poisoned(lv, S, first=0):
    """The level's d_raw and stash with every row the launch leaves out set to NaN: rows at or beyond live * S of both (the stash
    is stored in tiles of 32 points, S is a multiple of 32), and d_raw rows in front of first * S."""
    d, st = lv.d_raw.clone(), lv.stash.clone()
    d[LIVE_N * S:] = float("nan")
    d[:first * S] = float("nan")
    st[LIVE_N * S * lv.s_rows:] = float("nan")
    return d, st


@pytest.mark.parametrize("first", [(0, 0), (1, 0)])
@pytest.mark.parametrize("arch0,arch1", [(VD64, VD64), (VD64, VD128), (NOVD64, NOVD64)])
def test_bwd_pair_live_equals_its_halves_and_ignores_rows_outside_the_launch(dev, arch0, arch1, first):
    lv, sh, live = _live_pair(dev, arch0, arch1)
    for accumulate in (False, True):
        want = _backward(lv, sh, False, accumulate, live=live, first=first)
        _same(want, _backward(lv, sh, True, accumulate, live=live, first=first))
    want = _backward(lv, sh, False, False, live=live, first=first)
    pz = [_poisoned(lv[0], LIVE_S[0], first[0]), _poisoned(lv[1], LIVE_S[1], first[1])]
    for halves in (False, True):
        _same(want, _backward(lv, sh, halves, False, live=live, first=first, d_raw=[d for d, _ in pz], stash=[s for _, s in pz]))


@pytest.mark.parametrize("arch0,arch1", [(VD64, VD64), (VD64, VD128), (NOVD64, NOVD64)])
def test_bwd_live_equals_the_pair_with_first_ray_0_and_ignores_rows_outside_the_launch(dev, arch0, arch1):
    lv, sh, live = _live_pair(dev, arch0, arch1)
    pair = _backward(lv, sh, False, False, live=live, first=(0, 0))
    for i in range(2):
        one = _backward([lv[i]], [sh[i]], False, False, live=live)
        _same(one, [pair[i]])
        d, st = _poisoned(lv[i], LIVE_S[i])
        _same(one, _backward([lv[i]], [sh[i]], False, False, live=live, d_raw=[d], stash=[st]))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("arch0,arch1,M0,M1", [(VD128, VD128, 33, 128), (VD128, VD128, 300, 130),
                                               # W = 256: the only width whose wgrad plan has wide jobs, i.e. where the bf16x3 body of
                                               # wgrad_mixed_k runs (csrc/wgrad.hip add_net_jobs) — as one merged dgrad grid, and as
                                               # two dgrad launches behind one wgrad grid (architectures differ)
                                               (VD256, VD256, 129, 33), (VD256, VD128, 129, 33)],
                         ids=["33-128", "300-130", "D2W256-D2W256-129-33", "D2W256-D4W128-129-33"])
def test_bf16x3_pair_forms_equal_two_single_calls(dev, arch0, arch1, M0, M1, accumulate):
    lv, sh = [_level(dev, arch0, 71, M0), _level(dev, arch1, 72, M1)], [(M0, 1), (M1, 1)]
    pair = _backward(lv, sh, True, accumulate, bf=True)
    _same(pair, [_backward([lv[i]], [sh[i]], True, accumulate, bf=True)[0] for i in range(2)])
