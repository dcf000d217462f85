"""The entry points of the folded step loss (include/cnerf.h: cnerf_composite_fwd_{closs,lossform}, the cnerf_closs_finish* tails and
cnerf_lossform_finish, cnerf_composite_bwd_{closs,closs_ssim,closs_lpips,lossform}), called through the C ABI.  They are one host
path behind different argument lists, so a form that adds a term must equal the form without it when the term is switched off — BIT
FOR BIT (torch.equal, no tolerance anywhere in this file):

  finish_lpips, lpips_w = 0, ssim_P = 2   = finish_ssim     on terms[:10], stats, patch_d, ssim_d
  finish_lpips, lpips_w = 0, ssim_P = 0   = finish          on terms[:8], stats, patch_d
  bwd_closs_lpips, lpips_dx = 0           = bwd_closs_ssim
  bwd_closs_ssim, ssim_d = 0              = bwd_closs
  the hardmask / hardmask form chain      = the closs chain on the maps, terms[:8] and d_raw

B = 520 rays (two 16 x 16 patches + 8: 65 compositing workgroups of the loss form), S = 33 (one sample past a 32-sample tile), two
levels, a random mask, a prior and monocular depths.  Workspaces and outputs are handed over full of NaN: no form may leave a word
it is compared on unwritten."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import T, dev  # noqa: F401  (dev: the module's device fixture)

pytestmark = pytest.mark.gpu

B, S, P, N, FAR = 520, 33, 2, 256, 6.0
W = dict(rgb_w=1.0, depth_w=0.5, patch_w=0.001, coef=0.2, ssim_w=0.3)


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def call(name, *args):
    from consistentnerf_amd import _lib, ops
    rc = getattr(_lib.load(), name)(*args, ops._stream())
    assert rc == 0, (name, rc)


class _Step:
    """The inputs of one two-level batch, and each stage of the step through a named entry point."""

    def __init__(self, dev):
        from consistentnerf_amd import _lib
        rs = np.random.RandomState(11)
        f = lambda *s: rs.uniform(0.05, 1.0, size=s).astype(np.float32)  # noqa: E731
        self.dev = dev
        self.raw = [T(rs.normal(size=(B, S, 4)).astype(np.float32), dev) for _ in range(2)]
        self.z = [T(np.sort(2.0 + 4.0 * f(B, S), axis=1), dev) for _ in range(2)]
        self.rays = T(rs.normal(size=(B, 8)).astype(np.float32), dev)
        self.target, self.prior, self.mono = T(f(B, 3), dev), T(2.0 + 4.0 * f(B), dev), T(f(P * N), dev)
        self.mask = T((rs.uniform(size=B) < 0.6).astype(np.float32), dev)
        self.g_loss = T(np.array([0.7], np.float32), dev)
        self.lpips_v = T(f(2 * P), dev)
        self.closs = _lib.Closs(self.target.data_ptr(), self.mask.data_ptr(), self.prior.data_ptr(), FAR, 0)
        self.form = _lib.LossForm(0, 0, 0.0, None, None)      # hardmask / hardmask

    def nine(self, lv):
        from consistentnerf_amd.ops import _p
        return [_p(self.raw[lv]), 4, _p(self.z[lv]), _p(self.rays), 8, None, B, S, 0]

    @functools.lru_cache(maxsize=None)
    def forward(self, forms):
        """-> per level (rgb, disp, acc, depth, weights, ws)."""
        from consistentnerf_amd import _lib
        from consistentnerf_amd.ops import _p
        lib = _lib.load()
        name, floats = ("cnerf_composite_fwd_lossform", lib.cnerf_lossform_ws_floats) if forms else ("cnerf_composite_fwd_closs",
                                                                                                     lib.cnerf_closs_ws_floats)
        out = []
        for lv in (0, 1):
            maps = [nan(self.dev, B, 3), nan(self.dev, B), nan(self.dev, B), nan(self.dev, B), nan(self.dev, B, S)]
            ws = torch.full((floats(B) // 2,), float("nan"), device=self.dev, dtype=torch.float64)
            call(name, *self.nine(lv), C.byref(self.closs), *([C.byref(self.form)] if forms else []), *map(_p, maps), _p(ws))
            out.append((*maps, ws))
        return out

    @functools.lru_cache(maxsize=None)
    def finish(self, name, ssim_P=0, lpips_w=None):
        """-> (terms, stats, patch_d, ssim_d) of the tail `name` over the forward it belongs to."""
        from consistentnerf_amd import _lib
        from consistentnerf_amd.ops import _p
        forms = name == "cnerf_lossform_finish"
        (rgb, _, _, depth, _, ws), (rgb_c, _, _, depth_c, _, ws_c) = self.forward(forms)
        t = _lib.ClossTail(ws.data_ptr(), ws_c.data_ptr(), B, None, W["coef"], FAR, W["rgb_w"], W["depth_w"], W["patch_w"], 1,
                           depth.data_ptr(), depth_c.data_ptr(), self.mono.data_ptr(), P, N)
        terms, stats = nan(self.dev, 12), nan(self.dev, 16 if forms else 8)
        patch_d, ssim_d, d_temp = nan(self.dev, 2, P * N), nan(self.dev, 2, max(ssim_P, 1) * 768), nan(self.dev, 4)
        ssim = [ssim_P, W["ssim_w"], _p(rgb), _p(rgb_c), _p(self.target)]
        outs, grads = [_p(terms), _p(stats)], [_p(patch_d), _p(ssim_d)]
        args = {"cnerf_closs_finish": [*outs, _p(patch_d)],
                "cnerf_closs_finish_ssim": [*ssim, *outs, *grads],
                "cnerf_closs_finish_lpips": [*ssim, P, lpips_w, _p(self.lpips_v), *outs, *grads],
                "cnerf_lossform_finish": [C.byref(self.form), C.byref(self.form), *ssim, *outs, *grads, _p(d_temp)]}[name]
        call(name, C.byref(t), *args)
        return terms, stats, patch_d, ssim_d

    def backward(self, name, lv, fwd, stats, patch_d, ssim_d=None, lpips_dx=None):
        """-> d_raw of level lv through the backward `name`, seeded by the given tail outputs."""
        from consistentnerf_amd.ops import _p
        forms = name == "cnerf_composite_bwd_lossform"
        rgb, _, _, depth, _, _ = fwd[lv]
        w = stats.numel() // 2
        d_raw = nan(self.dev, B, S, 4)
        args = [*self.nine(lv), C.byref(self.closs), *([C.byref(self.form)] if forms else []), _p(rgb), _p(depth),
                _p(stats[lv * w:(lv + 1) * w]), _p(self.g_loss), W["rgb_w"], W["depth_w"], W["patch_w"], *([W["coef"]] if forms else []),
                _p(patch_d[lv]), P * N]
        if name != "cnerf_composite_bwd_closs":
            args += [W["ssim_w"], _p(ssim_d), 0 if ssim_d is None else ssim_d.numel() // 3]
        if lpips_dx is not None:
            args += [_p(lpips_dx), lpips_dx.shape[0] * 256]
        if forms:
            args += [None, None]
        call(name, *args, _p(d_raw))
        return d_raw


@functools.lru_cache(maxsize=None)
def _step(dev):
    return _Step(dev)


def written(*tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def test_finish_lpips_with_zero_weight_equals_finish_ssim(dev):
    s = _step(dev)
    a, b = s.finish("cnerf_closs_finish_lpips", 2, 0.0), s.finish("cnerf_closs_finish_ssim", 2)
    assert written(b[0][:10], *b[1:])
    assert torch.equal(a[0][:10], b[0][:10])
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


def test_finish_lpips_with_zero_weight_and_no_ssim_equals_finish(dev):
    s = _step(dev)
    a, b = s.finish("cnerf_closs_finish_lpips", 0, 0.0), s.finish("cnerf_closs_finish")
    assert written(b[0][:8], b[1], b[2])
    assert torch.equal(a[0][:8], b[0][:8]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("lv", [0, 1])
def test_bwd_lpips_with_zero_seeds_equals_bwd_ssim(dev, lv):
    s = _step(dev)
    fwd, (_, stats, patch_d, ssim_d) = s.forward(False), s.finish("cnerf_closs_finish_ssim", 2)
    zero = torch.zeros(P, 3, 16, 16, device=dev)
    a = s.backward("cnerf_composite_bwd_closs_lpips", lv, fwd, stats, patch_d, ssim_d[lv], zero)
    b = s.backward("cnerf_composite_bwd_closs_ssim", lv, fwd, stats, patch_d, ssim_d[lv])
    assert written(b) and torch.equal(a, b)


@pytest.mark.parametrize("lv", [0, 1])
def test_bwd_ssim_with_zero_seeds_equals_bwd_closs(dev, lv):
    s = _step(dev)
    fwd, (_, stats, patch_d, _) = s.forward(False), s.finish("cnerf_closs_finish")
    a = s.backward("cnerf_composite_bwd_closs_ssim", lv, fwd, stats, patch_d, torch.zeros(P * 768, device=dev))
    b = s.backward("cnerf_composite_bwd_closs", lv, fwd, stats, patch_d)
    assert written(b) and torch.equal(a, b)


def test_hardmask_form_chain_equals_closs_chain(dev):
    s = _step(dev)
    fa, fb = s.forward(True), s.forward(False)
    for lv in (0, 1):
        for x, y in zip(fa[lv][:5], fb[lv][:5]):
            assert written(y) and torch.equal(x, y)
    ta, tb = s.finish("cnerf_lossform_finish"), s.finish("cnerf_closs_finish")
    assert written(tb[0][:8]) and torch.equal(ta[0][:8], tb[0][:8])
    for lv in (0, 1):
        a = s.backward("cnerf_composite_bwd_lossform", lv, fa, ta[1], ta[2], None)
        b = s.backward("cnerf_composite_bwd_closs", lv, fb, tb[1], tb[2])
        assert written(b) and torch.equal(a, b)
