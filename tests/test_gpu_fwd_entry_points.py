"""The forward entry points of the MLP (include/cnerf.h: cnerf_mlp_fwd, _live, _embedded, _bf, _bf_train), called through the C ABI.
They are one host path behind different argument lists; this file pins what that path decides — which pointer, which stride, which
rows — BIT FOR BIT (torch.equal, no tolerance anywhere in this file):

  operand selection      ray rows at stride 11 == stride 8 + dirs == stride 13 with NaN in the two columns nobody may read
  rows outside a launch  raw rows past M keep the caller's bytes, the stash rows of the padding points M .. Mp are zero
  live count             cnerf_mlp_fwd_live leaves zero raw past the device-side count and, below it, what cnerf_mlp_fwd leaves on a
                         batch of exactly that many rays ("one render == two renders")
  embedded form          cnerf_mlp_fwd_embedded on ops.embed's rows == the points form (the shapes here are the ones
                         tests/test_gpu_geometry_envelope.py::test_fused_encoding_equals_embed does not run)

Networks: D=2/W=64 with and without view directions, D=2/W=128 for the plane kernels.  Shapes (B, S): (5, 7) = 35 points, a ragged
last tile; (4, 8) exactly one tile; (1, 1)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _inputs as I
from test_gpu_parity import T, dev, make_model  # noqa: F401  (dev: the module's device fixture)

pytestmark = pytest.mark.gpu

VD64, NOVD64, VD128 = (2, 64, True), (2, 64, False), (2, 128, True)
SHAPES = [(5, 7), (4, 8), (1, 1)]
SENTINEL = -7.5


class _Net:
    def __init__(self, dev, arch):
        from consistentnerf_amd import ops
        D, W, self.vd = arch
        model, _ = make_model(D, W, self.vd, 5, 71, dev)
        self.spec, self.dev = model.spec(), dev
        self.net = self.spec.c()
        self.params = model.kernel_tensors()
        self.packed = ops.pack_weights(self.spec, self.params)

    @functools.cached_property
    def packed_bf(self):
        from consistentnerf_amd import ops
        return ops.pack_weights_bf(self.spec, self.params, 3)

    def stash_floats(self, M):
        from consistentnerf_amd import _lib
        return _lib.load().cnerf_mlp_stash_floats(C.byref(self.net), M)


@functools.lru_cache(maxsize=None)
def _net(dev, arch):
    return _Net(dev, arch)


@functools.lru_cache(maxsize=None)
def _batch(dev, B, S):
    """Ray rows [B, 11] and ascending depths [B, S]."""
    rs = np.random.RandomState(100 * B + S)
    return T(I.ray_batch(B, seed=B + S), dev), T(np.sort(rs.uniform(2.0, 6.0, size=(B, S)).astype(np.float32), -1), dev)


def _forward(nt, entry, B, S, *, pts=None, rays=None, dirs=None, z=None, train=False, live=None, extra_rows=0, fill=None):
    """One call of `entry` on buffers this allocates (full of `fill` where given) -> (raw[B * S + extra_rows, raw_ch], stash or None)."""
    from consistentnerf_amd import _lib, ops
    lib, p, M = _lib.load(), ops._p, B * S
    new = (lambda n: torch.full((n,), fill, device=nt.dev)) if fill is not None else (lambda n: torch.empty(n, device=nt.dev))
    raw = new((M + extra_rows) * nt.spec.raw_ch).view(M + extra_rows, nt.spec.raw_ch)
    stash = new(nt.stash_floats(M)) if train else None
    rs = rays.shape[1] if rays is not None else 0
    rows = [p(pts), p(rays), rs, p(dirs), p(z), B, S, p(raw)]
    args = {"cnerf_mlp_fwd": lambda: [p(nt.packed)] + rows + [p(stash)],
            "cnerf_mlp_fwd_live": lambda: [p(nt.packed), p(rays), rs, p(z), B, S, p(raw), p(stash), p(live)],
            "cnerf_mlp_fwd_bf": lambda: [p(nt.packed_bf), 3] + rows,
            "cnerf_mlp_fwd_bf_train": lambda: [p(nt.packed_bf)] + rows + [p(stash)]}[entry]()
    rc = getattr(lib, entry)(C.byref(nt.net), *args, ops._stream())
    assert rc == 0, (entry, rc)
    return raw, stash


def _bits(x):
    """The words of a tensor: a stash holds ReLU sign-bit words next to its activations, which read as floats may be NaN."""
    return x.view(torch.int32)


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y))


def _three_layouts(dev, B, S, vd):
    """The same rays as (rows, dirs): stride 11; stride 8 + explicit directions; stride 13 whose columns 8, 9 hold NaN (the directions
    are a row's LAST three columns)."""
    r11, z = _batch(dev, B, S)
    nan = torch.full((B, 2), float("nan"), device=dev)
    return z, [(r11, None), (r11[:, :8].contiguous(), r11[:, 8:].contiguous() if vd else None), (torch.cat([r11[:, :8], nan, r11[:, 8:]], 1), None)]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B,S", SHAPES)
@pytest.mark.parametrize("arch", [VD64, NOVD64])
def test_fp32_operand_selection(dev, arch, B, S, train):
    nt = _net(dev, arch)
    z, layouts = _three_layouts(dev, B, S, nt.vd)
    got = [_forward(nt, "cnerf_mlp_fwd", B, S, rays=r, dirs=d, z=z, train=train, fill=0.0) for r, d in layouts]
    assert torch.isfinite(got[0][0]).all()
    _same(got[0], got[1])
    _same(got[0], got[2])


@pytest.mark.parametrize("perwave", [False, True])
@pytest.mark.parametrize("B,S", SHAPES)
def test_planes_operand_selection(dev, monkeypatch, B, S, perwave):
    nt = _net(dev, VD128)
    if perwave:
        monkeypatch.setenv("CNERF_BF_PERWAVE", "1")
    z, layouts = _three_layouts(dev, B, S, True)
    got = [_forward(nt, "cnerf_mlp_fwd_bf", B, S, rays=r, dirs=d, z=z) for r, d in layouts]
    assert torch.isfinite(got[0][0]).all()
    _same(got[0], got[1])
    _same(got[0], got[2])


@pytest.mark.parametrize("B,S", SHAPES)
@pytest.mark.parametrize("arch,entry", [(VD64, "cnerf_mlp_fwd"), (NOVD64, "cnerf_mlp_fwd"), (VD128, "cnerf_mlp_fwd_bf_train")])
def test_rows_outside_the_launch(dev, arch, entry, B, S):
    nt = _net(dev, arch)
    rays, z = _batch(dev, B, S)
    M, Mp = B * S, (B * S + 31) // 32 * 32
    raw, stash = _forward(nt, entry, B, S, rays=rays, z=z, train=True, extra_rows=32, fill=SENTINEL)
    assert torch.isfinite(raw[:M]).all() and (raw[:M] != SENTINEL).any()
    assert (raw[M:] == SENTINEL).all(), "the launch wrote raw rows past M"
    # tile-major (csrc/mlp_common.hpp): column c of point m of a 32-point tile row sits at octet c >> 3, [m][c & 7]
    st = stash.view(Mp // 32, -1, 32, 8).permute(0, 2, 1, 3).reshape(Mp, -1)
    assert (st[M:] == 0).all(), "stash rows of the padding points are not zero"
    if entry == "cnerf_mlp_fwd":      # (not asserted of the bf16x3 stash: at (5, 7) its sign-bit words read as floats are not all finite)
        assert torch.isfinite(st[:M]).all()


@pytest.mark.parametrize("count", [0, 1, 3, 4])
@pytest.mark.parametrize("arch", [VD64, NOVD64])
def test_live_count(dev, arch, count):
    nt, B, S = _net(dev, arch), 4, 32
    rays, z = _batch(dev, B, S)
    live = torch.tensor([count], device=dev, dtype=torch.int32)
    raw, stash = _forward(nt, "cnerf_mlp_fwd_live", B, S, rays=rays, z=z, train=True, live=live, fill=SENTINEL)
    assert (raw[count * S:] == 0).all(), "raw rows at or past the live count are not zero"
    if count:
        want_raw, want_stash = _forward(nt, "cnerf_mlp_fwd", count, S, rays=rays[:count].contiguous(), z=z[:count].contiguous(), train=True,
                                       fill=SENTINEL)
        assert torch.equal(raw[:count * S], want_raw)
        assert torch.equal(_bits(stash[:want_stash.numel()]), _bits(want_stash))      # (whole 32-point tile rows: S = 32)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("M", [1, 32, 35])
@pytest.mark.parametrize("arch", [VD64, NOVD64])
def test_embedded_equals_points(dev, arch, M, train):
    from consistentnerf_amd import _lib, ops
    nt = _net(dev, arch)
    rs = np.random.RandomState(M)
    pts = T(rs.uniform(-2, 2, size=(M, 3)).astype(np.float32), dev)
    dirs = rs.normal(size=(M, 3)).astype(np.float32)
    dirs = T(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True), dev)
    xe = torch.cat([ops.embed(pts, 10)] + ([ops.embed(dirs, 4)] if nt.vd else []), -1).contiguous()
    raw = torch.zeros(M, nt.spec.raw_ch, device=dev)
    stash = torch.zeros(nt.stash_floats(M), device=dev) if train else None
    rc = _lib.load().cnerf_mlp_fwd_embedded(C.byref(nt.net), ops._p(nt.packed), ops._p(xe), M, ops._p(raw), ops._p(stash), ops._stream())
    assert rc == 0, rc
    want = _forward(nt, "cnerf_mlp_fwd", M, 1, pts=pts, dirs=dirs if nt.vd else None, train=train, fill=0.0)
    assert torch.isfinite(raw).all()
    _same((raw, stash), want)
