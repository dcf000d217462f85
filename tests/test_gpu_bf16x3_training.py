"""The opt-in "bf16x3" training kernels against float64, in the DEFAULT run (`pytest -m gpu`, no CNERF_TRAIN_PRECISION): the training
forward mlp_fwd_bfs_k<NT, 3, TRAIN> (csrc/mlp_fwd_bf.hip), the dgrad mlp_dgrad_bfs_k (csrc/mlp_bwd_bf.hip), the wgrad_body_bf3 body
of wgrad_mixed_k (csrc/wgrad.hip) and the ring / split machinery they share (csrc/mlp_bf_common.hpp).  Every call opts in by
itself: `ops.mlp_forward_bf_train`, `packed_bf=`, the `_bf` entry points of the C ABI, or `model.training_precision = "bf16x3"`.

Tolerances — each one the suite's own or derived from the arithmetic, none read off what these kernels produce:
  raw                      |d| <= 3e-5 * max(1, max|raw|) against a float64 forward of the same weights and inputs (the suite's
                           forward bound, header of test_gpu_parity.py)
  each GEMM on its own     |stored - act(in @ W.T + b)| <= C_GEMM * (|in| @ |W|.T + |b|) elementwise, the layer's input taken from
                           the stash, the product in float64.  C_GEMM = 5e-7 + 4 * 2^-24:
                             5e-7      fp32 accumulation on the matrix cores (the constant of tests/test_gpu_lpips.py: 0.75-1.5e-7 of
                                       sum|ab| measured at K <= 1024, 3.5e-7 at K = 4096 for an fp32 fmaf chain)
                             3 * 2^-24 the three cross terms the three-plane product drops (w1 x2, w2 x1, w2 x2: plane i is below
                                       2^-8i of the operand, so each is at most 2^-24 |w||x|)
                             1 * 2^-24 the last bit of the plane split
                           A dropped or mis-paired FIRST-order term (w0 x1, w1 x0) leaves 2^-8 * 2^-8 = 2^-16 |w||x| per product:
                           20x this bound, yet small enough to hide in the chained 3e-5 of raw.  The same bound, C_GEMM * sum|a||b|
                           with the operands as the kernel read them, holds every GEMM of the dgrad (from its own workspace)
                           and of the wgrad (from that workspace and the stash).
  gradients                |d| <= 1e-5 * max|g| per tensor against the float64 replay of the backward from the stash (the kernel's
                           own ReLU masks), the suite's bound (test_mlp_backward_exact_from_stash)
  everything else          torch.equal

Shapes: (D, W) in ARCHS — (1, 128) has no trunk GEMM (pt_trunk unused), (2, 256) takes the `l == 1` tail of the dgrad walk, (3, 128)
one loop round with an even tail, (6, 256) has the skip layer as its last trunk layer, (8, 256) is the workload's — all with view
directions; point counts M against the 32-point wave and the 128-point workgroup: 1, 33, 127, 128, 129, 161."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _inputs as I
from oracle import nerf_oracle as O
from test_gpu_parity import (T, _kwargs, check, check_flips, check_param_grads, dev, make_model, relu_masks,  # noqa: F401  (dev: the
                             stash_blocks)                                                                   # device fixture)

pytestmark = pytest.mark.gpu

C_GEMM = 5e-7 + 4 * 2.0 ** -24
ARCHS = [(1, 128), (2, 256), (3, 128), (6, 256), (8, 256)]
SHAPES = {1: (1, 1), 33: (3, 11), 127: (1, 127), 128: (4, 32), 129: (43, 3), 161: (7, 23)}      # M -> (B rays, S points per ray)
# every architecture meets M = 129 and M = 33; every M meets (8, 256) and (2, 256)
CASES = [(D, W, M) for D, W in ARCHS for M in (129, 33)] + [(D, W, M) for D, W in ((8, 256), (2, 256)) for M in (1, 127, 128, 161)]
OCH, SEED = 5, 11


def _names(D, W):
    return [n for n, _ in I.nerf_param_shapes(D, W, 63, 27, OCH, True)][3:]


# ------------------------------------------------------------------------------------------------ the float64 reference
def forward64(sd64, x, xd, D):
    """NeRF.forward (view directions, skip after layer 4) on encoded inputs in the dtype of its arguments -> (raw [M, 4], the
    activations as the training stash names them: h0 .. h{D-1} and hv rectified, feat linear)."""
    acts, h = {}, x
    for l in range(D):
        inp = torch.cat([x, h], 1) if l == 5 else h
        h = torch.relu(inp @ sd64[f"pts_linears.{l}.weight"].t() + sd64[f"pts_linears.{l}.bias"])
        acts[f"h{l}"] = h
    sigma = h @ sd64["alpha_linear.weight"].t() + sd64["alpha_linear.bias"]
    acts["feat"] = h @ sd64["feature_linear.weight"].t() + sd64["feature_linear.bias"]
    acts["hv"] = torch.relu(torch.cat([acts["feat"], xd], 1) @ sd64["views_linears.0.weight"].t() + sd64["views_linears.0.bias"])
    rgb = acts["hv"] @ sd64["rgb_linear.weight"].t() + sd64["rgb_linear.bias"]
    return torch.cat([rgb, sigma], 1), acts


def replay64(sd64, blk, G, D, W):
    """The backward of NeRF.forward (view directions) in float64 from stashed activations `blk` (stash_blocks: enc, h0 .. h{D-1},
    feat, denc, hv), so the ReLU masks are the stash's own, and the seed gradient G [M, 4] = d(rgb, sigma) -> {parameter: gradient}.
    Checked against torch autograd in float64 by tests/test_host.py::test_bf16x3_float64_replay_equals_autograd."""
    Gd = G.double()
    d_rgb, d_sig = Gd[:, :3], Gd[:, 3:4]
    enc, ref = blk["enc"][:, :63], {}
    dZv = (d_rgb @ sd64["rgb_linear.weight"]) * (blk["hv"] > 0)
    ref["rgb_linear.weight"], ref["rgb_linear.bias"] = d_rgb.t() @ blk["hv"], d_rgb.sum(0)
    vin = torch.cat([blk["feat"], blk["denc"][:, :27]], 1)
    ref["views_linears.0.weight"], ref["views_linears.0.bias"] = dZv.t() @ vin, dZv.sum(0)
    dF = dZv @ sd64["views_linears.0.weight"][:, :W]
    hl = blk[f"h{D-1}"]
    ref["feature_linear.weight"], ref["feature_linear.bias"] = dF.t() @ hl, dF.sum(0)
    ref["alpha_linear.weight"], ref["alpha_linear.bias"] = d_sig.t() @ hl, d_sig.sum(0)
    dZ = (dF @ sd64["feature_linear.weight"] + d_sig @ sd64["alpha_linear.weight"]) * (hl > 0)
    for l in range(D - 1, 0, -1):
        hp = blk[f"h{l-1}"]
        ref[f"pts_linears.{l}.weight"] = dZ.t() @ (torch.cat([enc, hp], 1) if l == 5 else hp)
        ref[f"pts_linears.{l}.bias"] = dZ.sum(0)
        Wl = sd64[f"pts_linears.{l}.weight"]
        dZ = (dZ @ (Wl[:, 63:] if l == 5 else Wl)) * (hp > 0)
    ref["pts_linears.0.weight"], ref["pts_linears.0.bias"] = dZ.t() @ enc, dZ.sum(0)
    return ref


# ------------------------------------------------------------------------------------------------ shared, read-only state
class _Net:
    """One network on the device with what the entry points take: its spec, the fp32 panels and the three-plane panels — and its
    weights in float64 on the host (`sd`: the state dict the model was loaded from)."""

    def __init__(self, dev, D, W, model, sd):
        from consistentnerf_amd import ops
        self.D, self.W, self.dev, self.model = D, W, dev, model
        self.sd64 = {k: torch.as_tensor(v).double() for k, v in sd.items()}
        self.spec = self.model.spec()
        self.net = self.spec.c()
        self.params = [p.detach() for p in self.model.kernel_tensors()]
        self.packed = ops.pack_weights(self.spec, self.params)
        self.packed_bf = ops.pack_weights_bf(self.spec, self.params, 3)


@functools.lru_cache(maxsize=None)
def _net(dev, D, W, seed=SEED):
    return _Net(dev, D, W, *make_model(D, W, True, OCH, seed, dev))


@functools.lru_cache(maxsize=None)
def _points(M):
    """Points uniform in [-3, 3] and one unit direction per ray, as test_mlp_backward_exact_from_stash draws them -> float32
    (pts [M, 3], dirs [B, 3]) on the host, plus a seed gradient [M, 4]."""
    B, S = SHAPES[M]
    rs = np.random.RandomState(5)
    pts = rs.uniform(-3, 3, size=(B, S, 3)).astype(np.float32).reshape(-1, 3)
    dirs = rs.normal(size=(B, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    return T(pts), T(dirs), T(rs.normal(size=(M, 4)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _rays(M):
    """The same point cloud reached the other way: ray rows [B, 11] = (o, d, near, far, unit d) and depths z [B, S], with
    |o_i| <= 1, 1 <= |d| <= 1.3 and z in [0, 1.5], so that every point o + d z stays inside [-3, 3]^3."""
    B, S = SHAPES[M]
    rs = np.random.RandomState(6)
    o = rs.uniform(-1, 1, size=(B, 3))
    d = rs.normal(size=(B, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rs.uniform(1.0, 1.3, size=(B, 1))
    vd = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.concatenate([o, d, np.zeros((B, 1)), np.full((B, 1), 1.5), vd], 1).astype(np.float32)
    return T(rays), T(rs.uniform(0.0, 1.5, size=(B, S)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _fwd(dev, D, W, M, mode="pts"):
    """One bf16x3 training forward -> (raw [M, 4] float64 on the host, its stash on the device, the stash cut into blocks)."""
    from consistentnerf_amd import ops
    n, (B, S) = _net(dev, D, W), SHAPES[M]
    if mode == "pts":
        pts, dirs, _ = _points(M)
        raw, stash = ops.mlp_forward_bf_train(n.spec, n.packed_bf, B, S, pts=pts.to(dev), dirs=dirs.to(dev))
    else:
        rays, z = _rays(M)
        raw, stash = ops.mlp_forward_bf_train(n.spec, n.packed_bf, B, S, rays=rays.to(dev), z=z.to(dev))
    return raw.reshape(M, 4).double().cpu(), stash, stash_blocks(stash, M, D, W, True)


@functools.lru_cache(maxsize=None)
def _fwd_fp32(dev, D, W, M):
    """The exact-fp32 training forward of the same points: the stash the crossed backward tests start from."""
    from consistentnerf_amd import ops
    n, (B, S) = _net(dev, D, W), SHAPES[M]
    pts, dirs, _ = _points(M)
    raw, stash = ops.mlp_forward(n.spec, n.packed, B, S, pts=pts.to(dev), dirs=dirs.to(dev), want_stash=True)
    return raw, stash, stash_blocks(stash, M, D, W, True)


def _per_point(dirs, M):
    B, S = SHAPES[M]
    return dirs[:, None, :].expand(B, S, 3).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ 1. the training forward
@pytest.mark.parametrize("D,W,M", CASES)
def test_forward_raw_vs_float64_both_input_modes(dev, D, W, M):
    """`raw` of ops.mlp_forward_bf_train against the float64 forward, for explicit points + directions and for ray rows (stride 11)
    + depths.  The second mode is held to the bound twice.  The kernel forms a ray's points as the reference does, in float32
    without FMA contraction (R:384), and that IS the input of the encoding: columns 0-2 of the stashed encoding equal the float32
    expression o + d * z bit for bit, and raw meets the float64 forward of THOSE points.  It also meets the float64 forward of
    the points formed as o + d * z in float64 from the same float32 rays and depths: those differ from the float32 points by up to
    1 ulp(3) = 2.4e-7, which the 2^9-frequency encoding turns into 1.2e-4 of phase, so this second figure is mostly the
    conditioning of gamma(x) (about 10x the first) — and still within the bound."""
    n = _net(dev, D, W)
    pts, dirs, _ = _points(M)
    raw, _, blk = _fwd(dev, D, W, M)
    ref, _ = forward64(n.sd64, O.embed(pts.double(), 10), O.embed(_per_point(dirs, M).double(), 4), D)
    check(raw, ref, 3e-5 * max(1.0, float(ref.abs().max())), f"D={D} W={W} M={M} raw, points + directions")
    assert torch.equal(blk["enc"][:, :3].float(), pts)
    rays, z = _rays(M)
    raw, _, blk = _fwd(dev, D, W, M, "rays")
    p32 = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    assert torch.equal(blk["enc"][:, :3].float(), p32), "o + d * z is not the reference's float32 expression"
    xd = O.embed(_per_point(rays[:, 8:11], M).double(), 4)
    ref, _ = forward64(n.sd64, O.embed(p32.double(), 10), xd, D)
    check(raw, ref, 3e-5 * max(1.0, float(ref.abs().max())), f"D={D} W={W} M={M} raw, rays + depths")
    p64 = (rays[:, None, 0:3].double() + rays[:, None, 3:6].double() * z[..., None].double()).reshape(-1, 3)
    r64, _ = forward64(n.sd64, O.embed(p64, 10), xd, D)
    check(raw, r64, 3e-5 * max(1.0, float(r64.abs().max())), f"D={D} W={W} M={M} raw, rays + depths, points formed in float64")


@pytest.mark.parametrize("D,W,M", CASES)
def test_forward_stash_encodings_padding_and_sign_bits(dev, D, W, M):
    """The stash of the bf16x3 training forward: gamma(x) and gamma(d) are bit for bit those of the exact-fp32 training forward
    (both kernels call encode() of csrc/encode.hpp and store the tile with stash_tile), the padding column 63 of gamma(x) and the
    padding columns 27-31 of gamma(d) are exactly 0, the rows of padding points are zero and the ReLU sign-bit words equal
    (h > 0) of the stored activations for every trunk layer and the view branch (the last two asserted inside stash_blocks)."""
    _, _, blk = _fwd(dev, D, W, M)
    _, _, blk32 = _fwd_fp32(dev, D, W, M)
    assert torch.equal(blk["enc"], blk32["enc"]) and torch.equal(blk["denc"], blk32["denc"])
    assert float(blk["enc"][:, 63].abs().max()) == 0.0 and float(blk["denc"][:, 27:].abs().max()) == 0.0
    masks = relu_masks(_fwd(dev, D, W, M)[1], M, D, W, True)      # (decodes the sign-bit words and asserts bit == h > 0)
    assert len(masks) == D + 1 and all(bool(m.any()) for m in masks)
    for k in [f"h{l}" for l in range(D)] + ["hv"]:
        assert float(blk[k].min()) >= 0.0, f"{k} is stored rectified"


@pytest.mark.parametrize("D,W,M", CASES)
def test_forward_each_gemm_within_the_derived_bound(dev, D, W, M):
    """Every GEMM of the bf16x3 training forward on its own: the layer's input as the stash holds it, the product in float64, the
    elementwise bound C_GEMM * (|in| @ |W|.T + |b|) of the header.  This is the check a dropped first-order cross term, a swapped
    plane index or a panel offset that is off by one panel cannot pass."""
    _check_forward_gemms(_net(dev, D, W).sd64, _fwd(dev, D, W, M)[2], D, f"D={D} W={W} M={M}")


def _gemm_ratio(got, exact, scale, c):
    """max over the elements of |got - exact| / (c * scale); elements whose scale is 0 must be exact."""
    err = (got - exact).abs()
    assert float(err[scale == 0].max() if bool((scale == 0).any()) else 0.0) == 0.0
    return float((err / (c * scale).clamp(min=1e-300)).max())


def _check_forward_gemms(sd64, blk, D, tag):
    enc = blk["enc"][:, :63]
    layers = [("pts_linears.0", enc, "h0", True)]
    for l in range(1, D):
        layers.append((f"pts_linears.{l}", torch.cat([enc, blk[f"h{l-1}"]], 1) if l == 5 else blk[f"h{l-1}"], f"h{l}", True))
    layers.append(("feature_linear", blk[f"h{D-1}"], "feat", False))
    layers.append(("views_linears.0", torch.cat([blk["feat"], blk["denc"][:, :27]], 1), "hv", True))
    bad = []
    for name, inp, out, relu in layers:
        Wt, b = sd64[name + ".weight"], sd64[name + ".bias"]
        z = inp @ Wt.t() + b
        z = z.clamp(min=0) if relu else z
        ratio = _gemm_ratio(blk[out], z, inp.abs() @ Wt.abs().t() + b.abs(), C_GEMM)
        print(f"  {tag} {name:16s} K={inp.shape[1]:3d}  max err {float((blk[out] - z).abs().max()):.3e}  max err / bound {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((name, ratio))
    assert not bad, f"GEMMs beyond {C_GEMM:.2e} * (|in| @ |W|.T + |b|): {bad}"


@pytest.mark.parametrize("D,W", [(8, 256), (2, 256), (3, 128)])
def test_forward_rows_are_independent(dev, D, W):
    """Padding lanes and idle waves change nothing: the first M rows of raw from a 161-point call are bit for bit the M-point
    call on the same points (what test_ragged_batch_sizes states for the fp32 kernel), and so are the stash rows."""
    from consistentnerf_amd import ops
    n = _net(dev, D, W)
    rs = np.random.RandomState(77)
    pts = T(rs.uniform(-3, 3, size=(161, 3)).astype(np.float32), dev)
    dirs = rs.normal(size=(161, 3)).astype(np.float32)
    dirs = T(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True), dev)
    big, st_big = ops.mlp_forward_bf_train(n.spec, n.packed_bf, 161, 1, pts=pts, dirs=dirs)
    assert torch.isfinite(big).all()
    blk_big = stash_blocks(st_big, 161, D, W, True)
    for M in (1, 33, 128, 129):
        raw, st = ops.mlp_forward_bf_train(n.spec, n.packed_bf, M, 1, pts=pts[:M].contiguous(), dirs=dirs[:M].contiguous())
        assert torch.equal(raw, big[:M]), f"M = {M}"
        blk = stash_blocks(st, M, D, W, True)
        for k in blk:
            assert torch.equal(blk[k], blk_big[k][:M]), f"M = {M}: stash block {k}"


# ------------------------------------------------------------------------------------------------ the C ABI halves
def _nan_ws(n, M):
    from consistentnerf_amd import _lib
    return torch.full((_lib.load().cnerf_mlp_bwd_ws_floats(C.byref(n.net), M),), float("nan"), device=n.dev)


def _dgrad(n, M, stash, d_raw, bf, ws=None):
    """cnerf_mlp_dgrad[_bf] into a workspace handed over full of NaN -> the workspace."""
    from consistentnerf_amd import _lib, ops
    lib, (B, S) = _lib.load(), SHAPES[M]
    ws = _nan_ws(n, M) if ws is None else ws
    name = "cnerf_mlp_dgrad_bf" if bf else "cnerf_mlp_dgrad"
    rc = getattr(lib, name)(C.byref(n.net), ops._p(n.packed_bf if bf else n.packed), ops._p(d_raw), B, S, ops._p(stash), ops._p(ws),
                            ops._stream())
    assert rc == 0, (name, rc)
    return ws


def _wgrad(n, M, stash, ws, bf, accumulate=False, fill=7.0):
    """cnerf_mlp_wgrad[_bf] from a dgrad's workspace into gradients pre-filled with `fill` -> the gradients."""
    from consistentnerf_amd import _lib, ops
    lib, (B, S) = _lib.load(), SHAPES[M]
    grads = [torch.full(s, fill, device=n.dev) for s in n.spec.tensor_shapes()]
    ptrs = ops._ptrs(grads)
    name = "cnerf_mlp_wgrad_bf" if bf else "cnerf_mlp_wgrad"
    rc = getattr(lib, name)(C.byref(n.net), B, S, ops._p(stash), ops._p(ws), C.byref(ptrs), int(accumulate), ops._stream())
    assert rc == 0, (name, rc)
    return grads


ROWS = [("dgrad bf16x3 + wgrad fp32  ", True, False), ("dgrad fp32   + wgrad bf16x3", False, True),
        ("dgrad bf16x3 + wgrad bf16x3", True, True), ("dgrad fp32   + wgrad fp32  ", False, False)]


@functools.lru_cache(maxsize=None)
def _crossed(dev, D, W, M):
    """The four dgrad x wgrad combinations from ONE fp32 stash and ONE seed gradient -> {(dgrad_bf, wgrad_bf): gradients}, and
    {("ws", dgrad_bf): the blocks of that dgrad's workspace}; the two wgrads of a row pair read the same workspace."""
    n = _net(dev, D, W)
    _, stash, _ = _fwd_fp32(dev, D, W, M)
    G = _points(M)[2].to(dev)
    out = {}
    for dbf in (False, True):
        ws = _dgrad(n, M, stash, G, dbf)
        out["ws", dbf] = ws_blocks(ws, M, D, W)
        for wbf in (False, True):
            out[dbf, wbf] = _wgrad(n, M, stash, ws, wbf)
    return out


def ws_blocks(ws, M, D, W):
    """The gradient workspace a dgrad leaves (csrc/common.hpp NetGeom, csrc/geom.hip: logically [Mp][g_rows] in front of the wgrad
    partials, tile-major like the stash; columns dZ_0 .. dZ_{D-1} of W each, dF of W, dZv of W / 2, then 32 of which the first four
    hold the copy of d_raw) -> {z0 .. z{D-1}, feat, hv, out: [M, cols] float64 on the host}.  The rows of padding points are zero
    in every block the wgrad reads."""
    Mp, rows = (M + 31) // 32 * 32, D * W + W + W // 2 + 32
    full = ws[:Mp * rows].reshape(Mp // 32, rows // 8, 32, 8).permute(0, 2, 1, 3).reshape(Mp, rows).double().cpu()
    out, r = {}, 0
    for name, n in [(f"z{l}", W) for l in range(D)] + [("feat", W), ("hv", W // 2), ("out", 4)]:
        out[name] = full[:M, r:r + n]
        assert Mp == M or float(full[M:, r:r + n].abs().max()) == 0.0, f"padding rows of {name}"
        assert torch.isfinite(out[name]).all(), name
        r += n
    return out


def _rel_errors(names, grads, ref):
    """-> {name: max|g - ref| / max|ref|} of one gradient list against the replay (every tensor finite)."""
    out = {}
    for nm, g in zip(names, grads):
        assert torch.isfinite(g).all(), nm
        r = ref[nm].reshape(g.shape)
        out[nm] = float((g.double().cpu() - r).abs().max() / max(float(r.abs().max()), 1e-30))
    return out


@pytest.mark.parametrize("D,W,M", CASES)
def test_backward_each_kernel_isolated_vs_float64_replay(dev, D, W, M):
    """The bf16x3 dgrad writes the gradient workspace the fp32 wgrad reads, and both dgrads read the fp32 kernel's stash: from one
    stash and one seed gradient, the bf16x3 dgrad in front of the fp32 wgrad isolates the dgrad, the fp32 dgrad in front of the
    bf16x3 wgrad isolates the wgrad body, and both together are the path as trained.  Each of the four, the all-fp32 baseline
    included, is within 1e-5 * max|g| per tensor of the float64 replay from that stash."""
    n, names = _net(dev, D, W), _names(D, W)
    ref = replay64(n.sd64, _fwd_fp32(dev, D, W, M)[2], _points(M)[2], D, W)
    got, bad = _crossed(dev, D, W, M), []
    print(f"  D={D} W={W} M={M}: worst max|g - g64| / max|g64| over the tensors (bound 1e-5)")
    for tag, dbf, wbf in ROWS:
        errs = _rel_errors(names, got[dbf, wbf], ref)
        w = max(errs, key=errs.get)
        print(f"    {tag}  {errs[w]:.3e}  ({w})")
        bad += [(tag.strip(), k, v) for k, v in errs.items() if not v <= 1e-5]
    assert not bad, bad


@pytest.mark.parametrize("D,W,M", CASES)
def test_backward_each_gemm_within_the_derived_bound(dev, D, W, M):
    """Every GEMM of the bf16x3 backward on its own, as the forward's: the operands as the kernel read them — the dgrad's from its
    own workspace and the stash's sign bits, the wgrad's from that workspace and the stash — the product in float64, the bound
    C_GEMM * sum|a||b| elementwise (header; the contraction runs over <= 319 features in the dgrad, over the M <= 161 points of ONE
    point range in the wgrad, so the reduction of the split partials adds nothing).  The 1e-5 * max|g| of the replay cannot see a
    dropped second-order cross term (2^-16 per product); this can.  Not GEMMs: dZv = relu'(hv) * (d_rgb @ rgb_linear) is three
    fp32 multiply-adds on the VALU (4 * 2^-24 * sum|a||b|: one rounding per product and per add), the copy of d_raw is exact, a bias
    gradient is an fp32 column sum (the fp32 constant 5e-7 * sum|dZ|, within C_GEMM).  The all-fp32 baseline's ratios are printed
    next to the three bf16x3 rows', not asserted."""
    n, names = _net(dev, D, W), _names(D, W)
    blk = _fwd_fp32(dev, D, W, M)[2]
    Gd = _points(M)[2].double()
    got, bad = _crossed(dev, D, W, M), []
    for dbf in (True, False):
        g = got["ws", dbf]
        worst = max(_dgrad_gemm_ratios(n.sd64, blk, g, Gd, D, W))
        print(f"  D={D} W={W} M={M} dgrad {'bf16x3' if dbf else 'fp32  '}: worst max err / bound {worst[0]:.3f} ({worst[1]})")
        if dbf and not worst[0] <= 1.0:
            bad.append(("dgrad bf16x3",) + worst)
        for wbf in (True, False):
            worst = max(_wgrad_gemm_ratios(blk, g, dict(zip(names, got[dbf, wbf])), D))
            print(f"  D={D} W={W} M={M} wgrad {'bf16x3' if wbf else 'fp32  '} behind dgrad {'bf16x3' if dbf else 'fp32  '}: "
                  f"worst max err / bound {worst[0]:.3f} ({worst[1]})")
            if (dbf or wbf) and not worst[0] <= 1.0:
                bad.append((f"wgrad bf={wbf} behind dgrad bf={dbf}",) + worst)
    assert not bad, bad


def _dgrad_gemm_ratios(sd, blk, g, Gd, D, W):
    """The dgrad chain GEMM by GEMM from its own workspace `g` (ws_blocks) -> [(max err / bound, name)]."""
    assert torch.equal(g["out"], Gd)
    rows = [("rgb_linear^T", g["hv"], (Gd[:, :3] @ sd["rgb_linear.weight"]) * (blk["hv"] > 0),
             Gd[:, :3].abs() @ sd["rgb_linear.weight"].abs(), 4 * 2.0 ** -24)]
    Wv = sd["views_linears.0.weight"][:, :W]
    rows.append(("views_linears.0^T", g["feat"], g["hv"] @ Wv, g["hv"].abs() @ Wv.abs(), C_GEMM))
    Wf, Wa, ds = sd["feature_linear.weight"], sd["alpha_linear.weight"], Gd[:, 3:4]
    m = blk[f"h{D-1}"] > 0
    rows.append(("feature_linear^T", g[f"z{D-1}"], (g["feat"] @ Wf + ds @ Wa) * m, (g["feat"].abs() @ Wf.abs() + ds.abs() @ Wa.abs()) * m,
                 C_GEMM))
    for l in range(D - 1, 0, -1):
        Wl = sd[f"pts_linears.{l}.weight"][:, 63:] if l == 5 else sd[f"pts_linears.{l}.weight"]
        m = blk[f"h{l-1}"] > 0
        rows.append((f"pts_linears.{l}^T", g[f"z{l-1}"], (g[f"z{l}"] @ Wl) * m, (g[f"z{l}"].abs() @ Wl.abs()) * m, C_GEMM))
    return [(_gemm_ratio(a, b, s, c), nm) for nm, a, b, s, c in rows]


def _wgrad_gemm_ratios(blk, g, grads, D):
    """Every wgrad job (weight and bias) from the workspace `g` it read and the stash -> [(max err / bound, tensor name)]."""
    enc = blk["enc"][:, :63]
    jobs = [("pts_linears.0", g["z0"], enc), ("feature_linear", g["feat"], blk[f"h{D-1}"]),
            ("views_linears.0", g["hv"], torch.cat([blk["feat"], blk["denc"][:, :27]], 1)),
            ("alpha_linear", g["out"][:, 3:4], blk[f"h{D-1}"]), ("rgb_linear", g["out"][:, :3], blk["hv"])]
    jobs += [(f"pts_linears.{l}", g[f"z{l}"], torch.cat([enc, blk[f"h{l-1}"]], 1) if l == 5 else blk[f"h{l-1}"]) for l in range(1, D)]
    gr = {k: t.double().cpu() for k, t in grads.items()}
    rat = []
    for nm, dZ, inp in jobs:
        rat.append((_gemm_ratio(gr[nm + ".weight"], dZ.t() @ inp, dZ.abs().t() @ inp.abs(), C_GEMM), nm + ".weight"))
        rat.append((_gemm_ratio(gr[nm + ".bias"], dZ.sum(0), dZ.abs().sum(0), C_GEMM), nm + ".bias"))
    return rat


# ------------------------------------------------------------------------------------------------ every cross term, one product at a time
def _pattern(i):
    """A positive float32 value whose three bf16 planes are all large: 1 + a1 2^-8 + a2 2^-16 with a1 in {4..7}/8 (so plane 0 is 1
    and plane 1 is a1 2^-8) and a2 in {1, 2, 3}/8 (below half an ulp of plane 1, so plane 2 is a2 2^-16); i picks the pair."""
    return 1.0 + (4 + i % 4) / 8 * 2.0 ** -8 + (1 + (i // 4) % 3) / 8 * 2.0 ** -16


def _planes(t):
    """The three-plane split the kernels make (each plane the bf16 rounding, to nearest even, of what the previous ones left) of
    float32-representable values -> three float64 tensors."""
    r, out = t.float(), []
    for _ in range(3):
        p = r.to(torch.bfloat16).float()
        out.append(p.double())
        r = r - p
    return out


def _weakest_kept_term(a, b):
    """For elementwise single products a * b: over the six cross terms a_p b_q, p + q <= 2, the smallest of max |a_p b_q| /
    (C_GEMM |a||b|) — how far beyond the bound the result lands when the least visible of the six is lost."""
    pa, pb = _planes(a), _planes(b)
    lim = C_GEMM * (a.abs() * b.abs()).double().clamp(min=1e-300)
    return min(float(((pa[p] * pb[q]).abs() / lim).max()) for p in range(3) for q in range(3) if p + q <= 2)


def test_every_kept_cross_term_shows_in_single_product_gemms(dev):
    """The derived bound with nothing to hide behind.  On random operands a lost SECOND-order cross term (w1 x1, w0 x2, w2 x0: at
    most 2^-16 |w||x| per product, signs random) partly cancels over the contraction and can end near the bound; here every GEMM
    output is ONE product, of operands whose three planes are all large, so each of the six kept terms is >= 4x the bound on its
    own (asserted from a host-side three-plane split) and the loss of any one of them, or a plane index swapped for another,
    fails.  A (2, 256) network of diagonal, positive weights, biases 0, M = 33 points with designed coordinates:
      forward   pts_linears.0 (the LDS-operand GEMM): rows >= 128 hold a designed weight on one raw coordinate of gamma(x)
                pts_linears.1 (the register-operand GEMM): diag(designed) on h0, whose columns < 128 are coordinates times 2^-j
      dgrad     views_linears.0^T: diag(designed) on dZv = d_rgb times 2^-j;  pts_linears.1^T: diag(designed) on dZ_1, whose
                columns >= 128 are d_sigma times 2^-j
      wgrad     d pts_linears.1.weight[n >= 128, k < 128] = dZ_1[0, n] h0[0, k] (a wide job: the bf16x3 body), only point 0 seeded
    and every GEMM of the three kernels is held to C_GEMM * sum|a||b| by the checks of the random networks."""
    from consistentnerf_amd import ops
    D, W, M = 2, 256, 33
    B, S = SHAPES[M]
    model, _ = make_model(D, W, True, OCH, SEED, dev)
    pat = torch.tensor([_pattern(i) for i in range(W)], dtype=torch.float32)
    ar = torch.arange(W)
    sd = {k: torch.zeros_like(v, device="cpu") for k, v in model.state_dict().items()}
    sd["pts_linears.0.weight"][ar, ar % 3] = torch.where(ar < 128, 2.0 ** -(ar % 4).float(), pat)
    sd["pts_linears.1.weight"][ar, ar] = pat.flip(0)
    sd["feature_linear.weight"][ar[:128], ar[:128]] = 2.0 ** -(ar[:128] % 3).float()
    sd["alpha_linear.weight"][0, 128:] = 2.0 ** -(ar[128:] % 3).float()
    sd["views_linears.0.weight"][ar[:64], ar[:64]] = pat[:64]
    sd["views_linears.0.weight"][ar[64:128], W + ar[64:128] % 3] = pat[64:128]
    sd["rgb_linear.weight"][ar[:128] % 3, ar[:128]] = 2.0 ** -(ar[:128] % 2).float()
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    n = _Net(dev, D, W, model, sd)
    sd64 = n.sd64
    # (point 0, the one the wgrad sees, gets coordinates whose plane 2 is the largest the pattern has: _pattern(8 .. 10))
    pts = torch.tensor([[_pattern(5 * m + c + 8) for c in range(3)] for m in range(M)], dtype=torch.float32)
    dirs = torch.tensor([[_pattern(7 * b + c + 1) for c in range(3)] for b in range(B)], dtype=torch.float32)
    G = torch.zeros(M, 4)
    G[0] = torch.tensor([_pattern(i) for i in (3, 6, 9, 11)])
    raw, stash = ops.mlp_forward_bf_train(n.spec, n.packed_bf, B, S, pts=pts.to(dev), dirs=dirs.to(dev))
    assert torch.isfinite(raw).all()
    blk = stash_blocks(stash, M, D, W, True)
    assert torch.equal(blk["enc"][:, :3].float(), pts) and torch.equal(blk["denc"][:, :3].float(), _per_point(dirs, M))
    assert all(bool((blk[k] > 0).all()) for k in ("h0", "h1")) and bool((blk["hv"][:, :128] > 0).all())
    # what makes the test sharp: each targeted GEMM's single products show every kept term
    w0, w1, wv = sd["pts_linears.0.weight"], sd["pts_linears.1.weight"], sd["views_linears.0.weight"]
    power = {"pts_linears.0": _weakest_kept_term(w0[ar[128:], ar[128:] % 3][None, :], pts[:, ar[128:] % 3]),
             "pts_linears.1": _weakest_kept_term(w1[ar[:128], ar[:128]][None, :], blk["h0"][:, :128].float())}
    _check_forward_gemms(sd64, blk, D, "single products")
    ws = _dgrad(n, M, stash, G.to(dev), True)
    g = ws_blocks(ws, M, D, W)
    grads = dict(zip(_names(D, W), _wgrad(n, M, stash, ws, True)))
    power["views_linears.0^T"] = _weakest_kept_term(wv[ar[:64], ar[:64]][None, :], g["hv"][:1, :64].float())
    power["pts_linears.1^T"] = _weakest_kept_term(w1[ar[128:], ar[128:]][None, :], g["z1"][:1, 128:].float())
    power["d pts_linears.1.weight"] = _weakest_kept_term(g["z1"][0, 128:].float()[:, None], blk["h0"][0, :128].float()[None, :])
    for k, v in power.items():
        print(f"  {k:24s} the least visible kept cross term alone: {v:.1f} x the bound")
        assert v >= 4.0, (k, v)
    for name, rat in (("dgrad", _dgrad_gemm_ratios(sd64, blk, g, G.double(), D, W)), ("wgrad", _wgrad_gemm_ratios(blk, g, grads, D))):
        worst = max(rat)
        print(f"  single products, {name}: worst max err / bound {worst[0]:.3f} ({worst[1]})")
        assert worst[0] <= 1.0, (name, worst)


@pytest.mark.parametrize("D,W,M", CASES)
def test_wgrad_bf16x3_body_takes_the_wide_jobs_only(dev, D, W, M):
    """Which body of wgrad_mixed_k ran, read off the bits: cnerf_mlp_wgrad_bf and cnerf_mlp_wgrad on the SAME workspace agree bit
    for bit wherever add_net_jobs (csrc/wgrad.hip) plans a narrow job, which stays on the fp32 body, and differ where it plans a wide
    one (wave tiles of 4x4, 4x2 or 2x4), which the bf16x3 body takes.
    W = 256: wide are the W x W GEMMs of pts_linears.l (l >= 1; the h columns of the skip layer), feature_linear and the feature
    columns of views_linears.0 (4x2); narrow are pts_linears.0, the 63 encoding columns of the skip layer, the direction columns
    of views_linears.0, alpha_linear and rgb_linear, with the biases pts_linears.0.bias, alpha_linear.bias and rgb_linear.bias
    (a bias belongs to the job that carries bias_tensor; the biases of wide jobs are left unasserted).
    W = 128: every W x W job plans as 2x2 and the view layer as 2x1: the plan has NO wide job and every tensor is bit-equal."""
    names = _names(D, W)
    got = _crossed(dev, D, W, M)
    for dbf in (False, True):
        bf, fp = dict(zip(names, got[dbf, True])), dict(zip(names, got[dbf, False]))
        if W == 128:
            for k in names:
                assert torch.equal(bf[k], fp[k]), k
            continue
        skip = "pts_linears.5.weight" if D > 5 else None
        vw = "views_linears.0.weight"
        narrow = [(k, slice(None)) for k in ("pts_linears.0.weight", "pts_linears.0.bias", "alpha_linear.weight", "alpha_linear.bias",
                                             "rgb_linear.weight", "rgb_linear.bias")] + [(vw, slice(W, W + 27))]
        wide = [("feature_linear.weight", slice(None)), (vw, slice(0, W))]
        for l in range(1, D):
            k = f"pts_linears.{l}.weight"
            wide.append((k, slice(63, None) if k == skip else slice(None)))
        if skip:
            narrow.append((skip, slice(0, 63)))
        for k, cols in narrow:
            a, b = (bf[k], fp[k]) if bf[k].dim() == 1 else (bf[k][:, cols], fp[k][:, cols])
            assert torch.equal(a, b), f"narrow job {k}[:, {cols}] did not stay on the fp32 body"
        for k, cols in wide:
            assert not torch.equal(bf[k][:, cols], fp[k][:, cols]), f"wide job {k}[:, {cols}] did not run the bf16x3 body"


@pytest.mark.parametrize("D,W", [(8, 256), (2, 256)])
def test_wgrad_accumulates_with_one_add(dev, D, W):
    """accumulate = 1 into gradients pre-filled with 7.0 is bit for bit 7.0 + the overwrite result: the reduction does one fp32
    add per element.  W = 256, M = 129, all three bf16x3 rows."""
    M = 129
    n = _net(dev, D, W)
    _, stash, _ = _fwd_fp32(dev, D, W, M)
    G = _points(M)[2].to(dev)
    for _, dbf, wbf in ROWS[:3]:
        ws = _dgrad(n, M, stash, G, dbf)
        over, acc = _wgrad(n, M, stash, ws, wbf), _wgrad(n, M, stash, ws, wbf, accumulate=True)
        for i, (a, b) in enumerate(zip(acc, over)):
            assert torch.equal(a, 7.0 + b), f"tensor {i}"


@pytest.mark.parametrize("M", [33, 129])
@pytest.mark.parametrize("D,W", [(8, 256), (2, 256), (3, 128)])
def test_poisoned_stash_and_workspace_through_the_c_abi(dev, D, W, M):
    """cnerf_mlp_fwd_bf_train into a stash pre-filled with NaN, then cnerf_mlp_dgrad_bf + cnerf_mlp_wgrad_bf with a workspace
    pre-filled with NaN: every gradient is finite and bit for bit that of the run whose stash was pre-filled with zeros — the
    forward writes every stash word the backward reads (the rows of padding points included), and no kernel reads a workspace word
    it did not write."""
    from consistentnerf_amd import _lib, ops
    lib, n, (B, S) = _lib.load(), _net(dev, D, W), SHAPES[M]
    pts, dirs, G = (t.to(dev) for t in _points(M))
    runs = []
    for fill in (float("nan"), 0.0):
        stash = torch.full((lib.cnerf_mlp_stash_floats(C.byref(n.net), M),), fill, device=dev)
        raw = torch.full((M, 4), fill, device=dev)
        rc = lib.cnerf_mlp_fwd_bf_train(C.byref(n.net), ops._p(n.packed_bf), ops._p(pts), None, 0, ops._p(dirs), None, B, S, ops._p(raw),
                                        ops._p(stash), ops._stream())
        assert rc == 0, rc
        runs.append((raw, _wgrad(n, M, stash, _dgrad(n, M, stash, G, True), True)))
    (raw_nan, g_nan), (raw_zero, g_zero) = runs
    assert torch.isfinite(raw_nan).all() and torch.equal(raw_nan, raw_zero)
    for i, (a, b) in enumerate(zip(g_nan, g_zero)):
        assert torch.isfinite(a).all(), f"tensor {i} is not finite"
        assert torch.equal(a, b), f"tensor {i} differs"


# ------------------------------------------------------------------------------------------------ 3. the route training takes
def _profiled(fn):
    """-> (fn(), the kernel names ops.PROFILE recorded while it ran)."""
    from consistentnerf_amd import ops
    try:
        ops.PROFILE = []
        out = fn()
        names = [nm for nm, *_ in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return out, names


FP32_TRAINING_NAMES = {"mlp_fwd_train", "mlp_dgrad", "mlp_wgrad", "mlp_bwd_live"}


@pytest.mark.parametrize("D,W", [(2, 256), (8, 256)])
def test_run_network_with_training_precision_on_the_model(dev, D, W):
    """model.training_precision = "bf16x3" on a model of plain parameters (no environment variable): run_network + backward launch
    the three bf16x3 kernels and none of the fp32 training kernels; raw meets the oracle at 3e-5 * max(1, max|raw|) and the
    parameter gradients meet the oracle on the kernel's own ReLU branch at 1e-5 (max and L2), every pattern difference within
    round-off of zero, as test_random_networks_vs_oracle states for the default arithmetic."""
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    M = 129
    B, S = SHAPES[M]
    model, sd_np = make_model(D, W, True, OCH, SEED, dev)
    model.training_precision = "bf16x3"
    pts, dirs, G = _points(M)
    e, ed = get_embedder(10, 0)[0], get_embedder(4, 0)[0]
    raw, fwd_names = _profiled(lambda: run_network(pts.reshape(B, S, 3).to(dev), dirs.to(dev), model, e, ed))
    masks = relu_masks(raw.grad_fn.stash, M, D, W, True)
    sd = O.as_tensors(sd_np, True)
    flips = []
    ref = O.query(sd, pts.reshape(B, S, 3), dirs, O.NetCfg(D, W, use_viewdirs=True, output_ch=OCH), masks, flips)
    check_flips(flips)
    check(raw, ref.detach(), 3e-5 * max(1.0, float(ref.detach().abs().max())), "raw")
    Gs = G.reshape(B, S, 4)
    _, bwd_names = _profiled(lambda: (raw * Gs.to(dev)).sum().backward())
    assert fwd_names == ["mlp_fwd_train_bf3"] and sorted(bwd_names) == ["mlp_dgrad_bf3", "mlp_wgrad_bf3"], (fwd_names, bwd_names)
    assert not FP32_TRAINING_NAMES & set(fwd_names + bwd_names)
    (ref * Gs).sum().backward()
    tight = {"t." + k: (p_.grad if p_.grad is not None else torch.zeros_like(p_)).numpy() for k, p_ in sd.items()}
    check_param_grads(model, tight, "t.", "t.", rtol=1e-5, l2tol=1e-5)


def _two_level_step(dev, monkeypatch, prec_coarse, prec_fine):
    """One training step of a coarse + fine pair of (2, 256) networks owned by FusedAdam: render_rays at 8 rays with 16 + 16
    samples, both levels in the loss -> (the one call of ops.mlp_backward_pair as (args, kwargs), the kernel names of the step)."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.optim import FusedAdam
    coarse, _ = make_model(2, 256, True, OCH, 21, dev)
    fine, _ = make_model(2, 256, True, OCH, 22, dev)
    coarse.training_precision, fine.training_precision = prec_coarse, prec_fine
    kw = _kwargs(coarse, fine, 16, 16, 0.0, False, 0.0, False)
    rays = T(I.ray_batch(8, seed=5, near=2.125, far=4.67), dev)
    tgt = torch.rand(8, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    opt = FusedAdam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)
    calls, orig = [], ops.mlp_backward_pair

    def spy(*a, **k):
        calls.append((a, k))
        return orig(*a, **k)
    monkeypatch.setattr(ops, "mlp_backward_pair", spy)

    def step():
        opt.zero_grad()
        out = R.render_rays(rays, **kw)
        (R.img2mse(out["rgb_map"], tgt) + R.img2mse(out["rgb0"], tgt)).backward()
        torch.cuda.synchronize()
    _, names = _profiled(step)
    assert len(calls) == 1, f"the step called ops.mlp_backward_pair {len(calls)} times"
    return calls[0], names, {"fine": fine, "coarse": coarse}


def _check_pair_against_replay(call, models):
    """Both levels of a spied mlp_backward_pair call against the float64 replay from their own stashes: 1e-5 * max|g| per tensor."""
    fs, fp, fg, fB, fS, fst, fgr, cs, cp, cg, cB, cS, cst, cgr = call[0]
    assert (fB, fS, cB, cS) == (8, 32, 8, 16)
    names = _names(2, 256)
    for tag, g_raw, M, st, got in (("fine", fg, fB * fS, fst, fgr), ("coarse", cg, cB * cS, cst, cgr)):
        sd64 = {k: v.detach().double().cpu() for k, v in models[tag].state_dict().items()}
        ref = replay64(sd64, stash_blocks(st, M, 2, 256, True), g_raw.reshape(M, 4).cpu(), 2, 256)
        errs = _rel_errors(names, got, ref)
        w = max(errs, key=errs.get)
        print(f"  {tag}: worst max|g - g64| / max|g64| {errs[w]:.3e} ({w})")
        assert all(v <= 1e-5 for v in errs.values()), errs


def test_two_level_step_takes_the_bf16x3_pair(dev, monkeypatch):
    """Both levels bf16x3: the step launches the two bf16x3 training forwards and ONE merged bf16x3 dgrad + wgrad
    (ops.mlp_backward_pair once, with both plane buffers); the flat gradient is within 1e-5 * max|g| per tensor of the float64
    replay from the two stashes and bit for bit what two separate ops.mlp_backward(..., packed_bf=) calls give."""
    from consistentnerf_amd import ops
    call, names, models = _two_level_step(dev, monkeypatch, "bf16x3", "bf16x3")
    kw = call[1]
    assert kw.get("packed_bf0") is not None and kw.get("packed_bf1") is not None
    assert names.count("mlp_fwd_train_bf3") == 2 and names.count("mlp_dgrad_bf3") == 1 and names.count("mlp_wgrad_bf3") == 1
    assert not FP32_TRAINING_NAMES & set(names), names
    _check_pair_against_replay(call, models)
    fs, fp, fg, fB, fS, fst, fgr, cs, cp, cg, cB, cS, cst, cgr = call[0]
    sep_f = ops.mlp_backward(fs, fp, fg, fB, fS, fst, packed_bf=kw["packed_bf0"])
    sep_c = ops.mlp_backward(cs, cp, cg, cB, cS, cst, packed_bf=kw["packed_bf1"])
    for a, b in zip(list(fgr) + list(cgr), sep_f + sep_c):
        assert torch.equal(a, b.reshape(a.shape)), "the merged bf16x3 backward differs from the separate launches"


@pytest.mark.parametrize("prec_coarse,prec_fine", [("fp32", "bf16x3"), ("bf16x3", "fp32")])
def test_two_level_step_with_mixed_precisions_takes_the_fp32_pair(dev, monkeypatch, prec_coarse, prec_fine):
    """One level bf16x3, the other fp32: the step runs, the forward of each level is its own arithmetic, and the merged backward
    is the exact-fp32 pair (mlp_backward_pair needs BOTH plane buffers for the bf16x3 grids) — same replay bound."""
    call, names, models = _two_level_step(dev, monkeypatch, prec_coarse, prec_fine)
    kw = call[1]
    assert (kw.get("packed_bf0") is None) != (kw.get("packed_bf1") is None)
    assert (kw.get("packed_bf0") is not None) == (prec_fine == "bf16x3")
    assert names.count("mlp_fwd_train_bf3") == 1 and names.count("mlp_fwd_train") == 1
    assert names.count("mlp_dgrad") == 1 and names.count("mlp_wgrad") == 1
    assert "mlp_dgrad_bf3" not in names and "mlp_wgrad_bf3" not in names
    _check_pair_against_replay(call, models)


def test_stale_plane_buffer_is_refused_after_two_updates(dev):
    """The bf16-plane copy a bf16x3 forward used survives ONE parameter update and re-pack before its backward (two buffers
    alternate) and is refused after two, as test_packed_weights_double_buffer states for the fp32 panels.  The planes are re-packed
    here by what re-packs them alone: a bf16x3 evaluation query between the steps (inference_precision, under no_grad), which
    leaves the fp32 panels of the parked forward untouched — so the refusal is the plane buffer's own."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.optim import FusedAdam
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    M = 33
    B, S = SHAPES[M]
    model, _ = make_model(2, 256, True, OCH, 95, dev)
    model.training_precision = model.inference_precision = "bf16x3"
    opt = FusedAdam(list(model.parameters()), lr=1e-2)
    pts, dirs, G = _points(M)
    pts, dirs, G = pts.reshape(B, S, 3).to(dev), dirs.to(dev), G.reshape(B, S, 4).to(dev)
    e, ed = get_embedder(10, 0)[0], get_embedder(4, 0)[0]

    def fwd():
        return (run_network(pts, dirs, model, e, ed) * G).sum()

    def update_and_repack():
        opt.step()
        with torch.no_grad():
            run_network(pts, dirs, model, e, ed)
    opt.zero_grad()
    fwd().backward()
    ref = opt.flat_grad.clone()
    assert float(ref.abs().max()) > 0
    l = fwd()
    update_and_repack()
    opt.zero_grad()
    l.backward()                  # one update: the backward still reads the planes its forward used
    assert torch.equal(opt.flat_grad, ref)
    l = fwd()
    update_and_repack()
    update_and_repack()
    with pytest.raises(ops.CnerfError, match="bf16-plane copy it used has been re-packed"):
        l.backward()
