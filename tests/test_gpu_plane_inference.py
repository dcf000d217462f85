"""The opt-in reduced-precision INFERENCE forwards (csrc/mlp_fwd_bf.hip: modes bf16, bf16x2, bf16x3, fp16x2; the shared-panel kernel
mlp_fwd_bfs_k<NT, MODE, false> and the per-wave kernel mlp_fwd_bf_k<NT, MODE>) against float64, over the architectures, point counts,
input forms and operand ranges they claim.  tests/_planes_ref.py restates the four arithmetics on the CPU; tests/test_planes_ref_cpu.py
shows that the bounds below reject an emulation that loses or mis-pairs any single cross term.

With scale = max(1, max|raw64|) and every distance max|.| / scale against forward64 (float64, same weights and inputs):
  K   the kernel's                     E   the emulation's, fp16 subnormals kept            A   forward64(..., dtype=float32)'s, ATen on the CPU
(a) per (architecture, M, mode):   A <= 2e-6 (well-conditioned inputs: the convention of test_composite_vs_float64),  K <= the mode's
    tier (1e-1, 2e-3, 2e-5, 2e-5),  and  K <= 2 E + 4 A: the kernel is the emulation plus fp32 accumulation, A is what fp32 accumulation
    costs this network, 4 covers a chain order other than ATen's, 2 activations that split differently after an fp32-sized perturbation.
(b) torch.equal throughout: shared-panel == per-wave wherever both exist; four input forms give the same bits on both kernels in every
    mode; raw rows past M keep a sentinel; B = 0 writes nothing.
(c) fp16x2 over its stated range, bf16x3 as the control: cold layers (2^-6, 2^-9: the low planes are fp16 subnormals — the bound holds
    only if conversion, residual and matrix pipe all keep them; the flushed emulation's E is recorded next to K), a hot layer 0, weights
    of 200 with activations in the low thousands, an all-zero trunk layer, the origin and -0.0.
(d) what the kernels do not take raises CnerfError before any launch.
(e) the crafted family (operands whose planes are all maximal and of one sign, one GEMM at a time): kernel against EMULATION,
    elementwise relative to raw, within 4 x the larger of (exact-fp32 kernel vs float64, fp32 CPU forward vs float64) — a bound made of
    independent, already-tested code — with the precondition that every single-term mutant moves the emulation by >= 2 x that bound.

Architectures: _planes_ref.ARCHS.  (5, 128, 7, 2, 4), the odd-D network of 7 / 2 frequencies, cannot be built (D = skip + 1: the reference mis-shapes, the library
refuses: asserted in (d)); (5, 128, 7, 2, 3) stands in.  Point counts: M in {1, 33, 127, 128, 129, 161} as (B, S) with S > 1 against the
32-point wave and the 128-point workgroup; every architecture meets 129 and 33, every M meets (8, 256, ..) and (4, 128, 4, 4, 4).

Every figure is printed, and written to $CNERF_RECORD_DIR/plane_inference.json when that variable names a directory;
profiles/plane_inference.json is the MI355X run this file was written against: the largest K / (2 E + 4 A) per mode is 0.50 (bf16),
0.64 (bf16x2), 0.69 (bf16x3), 0.30 (fp16x2); on the range families 0.51 (bf16x3) and 0.27 (fp16x2), the cold layers at K = 3.2e-7 ...
1.0e-6 where the flushed emulation is at 8.8e-5 ... 4.2e-4; the crafted family at most 0.35 of its bound, every single-term mutant at
least 6.0 x.  The thinnest cases are M = 1 — K and A are then one point's luck, and A is the CPU's (ATen's summation order): (8, 256,
10, 4, 4) M = 1 bf16x3 has K 5.0e-7 against E 7.3e-8 and A 1.4e-7."""
import contextlib
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import _planes_ref as P
from test_gpu_parity import T, dev, make_model  # noqa: F401  (dev: the device fixture)

pytestmark = pytest.mark.gpu

MODES = P.MODES
WORKLOAD, PERWAVE_ONLY = (8, 256, 10, 4, 4), (4, 128, 4, 4, 4)
CASES = [(cfg, M) for cfg in P.ARCHS for M in (129, 33)] + [(cfg, M) for cfg in (WORKLOAD, PERWAVE_ONLY) for M in (1, 127, 128, 161)]
SENTINEL = -7.5


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _both_kernels(cfg):
    """launch_bf: the shared-panel kernel needs the 64- / 32-channel encoding tiles (in_chp == 64; dir_chp is 32 for every encoding)."""
    return 32 < P.embed_dim(cfg[2]) <= 64


# ------------------------------------------------------------------------------------------------ the record
RECORD = {}


def _record(section, key, row):
    RECORD.setdefault(section, {})[key] = row
    out_dir = os.environ.get("CNERF_RECORD_DIR")
    if not out_dir:
        return
    os.makedirs(out_dir, exist_ok=True)
    worst = {}
    for k, r in RECORD.get("float64", {}).items():
        worst[r["mode"]] = max(worst.get(r["mode"], 0.0), r["K"] / r["bound"])
    with open(os.path.join(out_dir, "plane_inference.json"), "w") as f:
        json.dump({"units": "max|d raw| / max(1, max|raw64|); crafted: max over elements of |d raw| / |raw64|",
                   "bound": "K <= 2 E + 4 A and K <= tier; crafted: |kernel - emulation| <= 4 max(F, A)", "tiers": P.TIERS,
                   "worst_K_over_bound": worst, **RECORD}, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ networks and runs
class _Net:
    """One network on the device: its spec, parameters in C-ABI order, and its packed panels by mode ("fp32": the exact kernel's)."""

    def __init__(self, dev, cfg, sd, och=4):
        from consistentnerf_amd import ops
        D, W, L, Lv, skip = cfg
        self.cfg, self.sd, self.dev = cfg, sd, dev
        self.spec = ops.NetSpec(D=D, W=W, multires=L, multires_views=Lv, use_viewdirs=True, output_ch=och, skip=skip)
        self.net = self.spec.c()
        self.params = [t.to(dev) for t in P.kernel_tensors(sd, D)]
        assert [tuple(t.shape) for t in self.params] == [tuple(s) for s in self.spec.tensor_shapes()], cfg      # (the pack kernels index by these)
        self._pk = {}

    def packed(self, mode):
        from consistentnerf_amd import ops
        if mode not in self._pk:
            self._pk[mode] = (ops.pack_weights(self.spec, self.params) if mode == "fp32"
                              else ops.pack_weights_bf(self.spec, self.params, ops.PRECISION_PLANES[mode]))
        return self._pk[mode]


@functools.lru_cache(maxsize=None)
def _net(dev, cfg, family=None):
    if family is None:
        return _Net(dev, cfg, P.state_dict(cfg, P.ARCHS.get(cfg, 4)), P.ARCHS.get(cfg, 4))
    return _Net(dev, cfg, P.range_net(cfg, family))


@contextlib.contextmanager
def _perwave(on):
    if on:
        os.environ["CNERF_BF_PERWAVE"] = "1"
    try:
        yield
    finally:
        os.environ.pop("CNERF_BF_PERWAVE", None)


def _run(n, mode, M, perwave=False, **inputs):
    """One inference forward of `mode` ("fp32": the exact kernel) -> raw [M, 4] on the device."""
    from consistentnerf_amd import ops
    B, S = P.SHAPES[M]
    inputs = {k: v.to(n.dev) for k, v in inputs.items()}
    if mode == "fp32":
        return ops.mlp_forward(n.spec, n.packed("fp32"), B, S, **inputs)[0].reshape(M, 4)
    with _perwave(perwave):
        return ops.mlp_forward_bf(n.spec, n.packed(mode), ops.PRECISION_PLANES[mode], B, S, **inputs).reshape(M, 4)


@functools.lru_cache(maxsize=None)
def _cpu(cfg, M, family=None):
    """-> (sd, pts [M, 3], dirs [B, 3], raw64, scale, A) — the float64 reference, computed once and shared."""
    sd = P.state_dict(cfg, P.ARCHS.get(cfg, 4)) if family is None else P.range_net(cfg, family)
    pts, dirs = P.points(M)
    dpp = P.per_point(dirs, M)
    ref = P.forward64(sd, pts, dpp, cfg)
    scale = max(1.0, float(ref.abs().max()))
    return sd, pts, dirs, ref, scale, P.dist(P.forward64(sd, pts, dpp, cfg, dtype=torch.float32), ref, scale)


@functools.lru_cache(maxsize=None)
def _emu(cfg, M, mode, family=None, flush=False):
    """-> (E, the largest activation, raw) of the emulation on the inputs of _cpu."""
    sd, pts, dirs, ref, scale, _ = _cpu(cfg, M, family)
    raw, amax = P.forward_planes(sd, pts, P.per_point(dirs, M), cfg, mode, flush=flush)
    return P.dist(raw, ref, scale), amax, raw


@functools.lru_cache(maxsize=None)
def _raw(dev, cfg, M, mode, perwave, family=None):
    """The kernel's raw on the inputs of _cpu, on the host."""
    _, pts, dirs, *_ = _cpu(cfg, M, family)
    return _run(_net(dev, cfg, family), mode, M, perwave, pts=pts, dirs=dirs).cpu()


# ------------------------------------------------------------------------------------------------ (a) against float64
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg,M", CASES, ids=_id)
def test_kernel_vs_float64(dev, cfg, M, mode):
    """The kernel launch_bf picks for the architecture (shared-panel where the encoding tiles allow it, per-wave otherwise)."""
    *_, ref, scale, A = _cpu(cfg, M)
    E = _emu(cfg, M, mode)[0]
    raw = _raw(dev, cfg, M, mode, False)
    assert torch.isfinite(raw).all()
    K, bound = P.dist(raw, ref, scale), 2 * E + 4 * A
    print(f"  {cfg} M={M} {mode}: scale {scale:.3g}  K {K:.3e}  E {E:.3e}  A {A:.3e}  K / (2E + 4A) {K / bound:.3f}  K / tier {K / P.TIERS[mode]:.3f}")
    _record("float64", f"{_id(cfg)} M={M} {mode}", dict(mode=mode, kernel="shared" if _both_kernels(cfg) else "perwave", scale=scale, K=K, E=E,
                                                        A=A, bound=bound))
    assert A <= 2e-6, "the fp32 forward itself is far from float64: the inputs are badly conditioned"
    assert K <= P.TIERS[mode], (K, P.TIERS[mode])
    assert K <= bound, (K, E, A)


# ------------------------------------------------------------------------------------------------ (b) one arithmetic
@pytest.mark.parametrize("cfg,M", [c for c in CASES if _both_kernels(c[0])], ids=_id)
def test_shared_panel_equals_per_wave(dev, cfg, M):
    for mode in MODES:
        a, b = _raw(dev, cfg, M, mode, False), _raw(dev, cfg, M, mode, True)
        assert torch.equal(a, b), (mode, float((a - b).abs().max()))


FORM_CFGS = [(2, 128, 10, 4, 4), PERWAVE_ONLY]


def _forms(dev, M):
    """The same points four ways -> [(name, kwargs of ops.mlp_forward_bf)]; pts = o + d * z in fp32 on the device."""
    rays, z = (t.to(dev) for t in P.rays(M))
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3).contiguous()
    nan = torch.full((rays.shape[0], 2), float("nan"), device=dev)
    return [("pts + dirs", dict(pts=pts, dirs=rays[:, 8:11].contiguous())), ("stride 11", dict(rays=rays, z=z)),
            ("stride 8 + dirs", dict(rays=rays[:, :8].contiguous(), z=z, dirs=rays[:, 8:11].contiguous())),
            ("stride 13, NaN in columns 8, 9", dict(rays=torch.cat([rays[:, :8], nan, rays[:, 8:]], 1).contiguous(), z=z))]


@pytest.mark.parametrize("perwave", [False, True], ids=["default", "perwave"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", FORM_CFGS, ids=_id)
def test_four_input_forms_give_the_same_bits(dev, cfg, mode, perwave):
    """(4, 128, 4, 4, 4) has the per-wave kernel only: its two rows run the same kernel, with and without the environment switch."""
    n = _net(dev, cfg)
    for M in (129, 33, 1):
        got = [(name, _run(n, mode, M, perwave, **kw)) for name, kw in _forms(dev, M)]
        assert torch.isfinite(got[0][1]).all()
        for name, raw in got[1:]:
            assert torch.equal(raw, got[0][1]), (M, name, float((raw - got[0][1]).abs().max()))


@pytest.mark.parametrize("perwave", [False, True], ids=["default", "perwave"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", [WORKLOAD, PERWAVE_ONLY], ids=_id)
def test_c_entry_point_leaves_rows_past_M_and_an_empty_batch_alone(dev, cfg, mode, perwave):
    from consistentnerf_amd import _lib, ops
    lib, n, planes = _lib.load(), _net(dev, cfg), ops.PRECISION_PLANES[mode]
    for M in (129, 33, 1):
        B, S = P.SHAPES[M]
        _, pts, dirs, *_ = _cpu(cfg, M)
        pts, dirs = pts.to(dev), dirs.to(dev)
        raw = torch.full((M + 32, 4), SENTINEL, device=dev)
        with _perwave(perwave):
            rc = lib.cnerf_mlp_fwd_bf(C.byref(n.net), ops._p(n.packed(mode)), planes, ops._p(pts), None, 0, ops._p(dirs), None, B, S, ops._p(raw),
                                      ops._stream())
            assert rc == 0, rc
            assert torch.equal(raw[:M].cpu(), _raw(dev, cfg, M, mode, perwave))
            assert (raw[M:] == SENTINEL).all(), f"M = {M}: the launch wrote raw rows past M"
            raw.fill_(SENTINEL)
            rc = lib.cnerf_mlp_fwd_bf(C.byref(n.net), ops._p(n.packed(mode)), planes, ops._p(pts), None, 0, ops._p(dirs), None, 0, S, ops._p(raw),
                                      ops._stream())
        assert rc == 0, rc
        assert (raw == SENTINEL).all(), "B = 0 wrote something"


# ------------------------------------------------------------------------------------------------ (c) the stated range
@pytest.mark.parametrize("mode", ["fp16x2", "bf16x3"])
@pytest.mark.parametrize("family", P.RANGE_FAMILIES)
@pytest.mark.parametrize("cfg", P.RANGE_CFGS, ids=_id)
def test_stated_range_vs_float64(dev, cfg, family, mode):
    """_planes_ref.range_net: cold layers, a hot layer 0, weights of 200 with activations in the low thousands — both kernels, the
    same bits, finite, inside the tier and inside 2 E + 4 A with E the emulation that KEEPS fp16 subnormals.  On the cold layers
    the emulation that flushes them is 5 - 12x over the tier (recorded as E_flush): a kernel found there would mean the conversion,
    the residual or the matrix pipe drops subnormals, and the range statement of the header would be wrong."""
    from consistentnerf_amd import ops
    M = 129
    sd, *_, ref, scale, A = _cpu(cfg, M, family)
    E, amax, _ = _emu(cfg, M, mode, family)
    (_, _, kept), (E_flush, _, flushed) = _emu(cfg, M, "fp16x2", family), _emu(cfg, M, "fp16x2", family, True)
    wmax = max(float(np.abs(v).max()) for k, v in sd.items() if k.endswith(".weight") and k.split(".")[0] not in ("alpha_linear", "rgb_linear"))
    assert wmax < ops.FP16X2_MAX_WEIGHT and amax < ops.FP16X2_MAX_ACTIVATION
    if family == "wide":
        assert wmax == 200.0 and 1000.0 <= amax, (wmax, amax)
    raw = _raw(dev, cfg, M, mode, False, family)
    assert torch.isfinite(raw).all()
    assert torch.equal(raw, _raw(dev, cfg, M, mode, True, family)), "shared-panel and per-wave kernels differ"
    K, bound = P.dist(raw, ref, scale), 2 * E + 4 * A
    d_kept, d_flush = P.dist(raw, kept.double(), scale), P.dist(raw, flushed.double(), scale)      # the kernel against BOTH fp16x2 emulations
    print(f"  {cfg} {family} {mode}: max|w| {wmax:.4g} max|activation| {amax:.4g} scale {scale:.3g}  K {K:.3e}  E {E:.3e}  E_flush(fp16x2) "
          f"{E_flush:.3e}  A {A:.3e}  K / (2E + 4A) {K / bound:.3f}  from the fp16x2 emulation: subnormals kept {d_kept:.3e}, flushed {d_flush:.3e}")
    _record("range", f"{_id(cfg)} {family} {mode}", dict(mode=mode, scale=scale, max_weight=wmax, max_activation=amax, K=K, E=E,
                                                         E_flush_fp16x2=E_flush, A=A, bound=bound, kernel_vs_fp16x2_kept=d_kept,
                                                         kernel_vs_fp16x2_flushed=d_flush))
    assert A <= 2e-6
    assert K <= 2e-5 and K <= bound, (K, E, E_flush, A)
    if mode == "fp16x2" and family.startswith("cold"):      # (follows from the bound: K <= 2e-5 < E_flush; stated for the reader of a failure)
        assert d_kept < d_flush, "the kernel is nearer the emulation that flushes fp16 subnormals"


@pytest.mark.parametrize("mode", ["fp16x2", "bf16x3"])
@pytest.mark.parametrize("cfg", P.RANGE_CFGS, ids=_id)
def test_sparse_layer_origin_and_negative_zero(dev, cfg, mode):
    """A last trunk layer of exactly zero weights: h = relu(bias) for every point, so raw is what the biases (and the ray's
    direction) imply — bit for bit the same for every point of a ray, bit for bit the raw of a network whose EARLIER layers are
    different ones, and inside the bound against float64.  Then the unchanged network: the origin and (-0.0, -0.0, -0.0) give the
    same bits, and putting them into rows 0 and 1 changes no other row."""
    M = 129
    B, S = P.SHAPES[M]
    D = cfg[0]
    sd, pts, dirs, ref_plain, _, _ = _cpu(cfg, M)
    dpp = P.per_point(dirs, M)
    zero = {k: v.copy() for k, v in sd.items()}
    zero[f"pts_linears.{D - 1}.weight"][:] = 0.0
    other = {k: v.copy() for k, v in P.state_dict(cfg, 4, seed=12).items()}
    for k in (f"pts_linears.{D - 1}", "feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"):
        other[k + ".weight"], other[k + ".bias"] = zero[k + ".weight"], zero[k + ".bias"]
    ref = P.forward64(zero, pts, dpp, cfg)
    scale = max(1.0, float(ref.abs().max()))
    A = P.dist(P.forward64(zero, pts, dpp, cfg, dtype=torch.float32), ref, scale)
    E = P.dist(P.forward_planes(zero, pts, dpp, cfg, mode)[0], ref, scale)
    for perwave in (False, True):
        raw = _run(_Net(dev, cfg, zero), mode, M, perwave, pts=pts, dirs=dirs).cpu()
        assert torch.isfinite(raw).all()
        assert torch.equal(raw.reshape(B, S, 4), raw.reshape(B, S, 4)[:, :1].expand(B, S, 4)), "points of one ray differ behind a zero layer"
        assert torch.equal(raw, _run(_Net(dev, cfg, other), mode, M, perwave, pts=pts, dirs=dirs).cpu()), "layers in front of a zero layer show"
        K = P.dist(raw, ref, scale)
        print(f"  {cfg} zero layer {mode} {'per-wave' if perwave else 'shared'}: K {K:.3e}  E {E:.3e}  A {A:.3e}  K / (2E + 4A) {K / (2 * E + 4 * A):.3f}")
        assert K <= 2e-5 and K <= 2 * E + 4 * A, (K, E, A)
        p0 = pts.clone()
        p0[0], p0[1] = 0.0, -0.0
        assert bool(torch.signbit(p0[1]).all()) and not bool(torch.signbit(p0[0]).any())
        got = _run(_net(dev, cfg), mode, M, perwave, pts=p0, dirs=dirs).cpu()
        assert torch.isfinite(got).all()
        assert torch.equal(got[0], got[1]), "the origin and -0.0 give different raw"
        assert torch.equal(got[2:], _raw(dev, cfg, M, mode, perwave)[2:]), "rows 0 and 1 changed another row"
        r0 = P.forward64(sd, p0[:2], dpp[:2], cfg)
        sc = max(1.0, float(ref_plain.abs().max()))
        assert P.dist(got[:2], r0, sc) <= 2e-5


# ------------------------------------------------------------------------------------------------ (d) limits
def _raises_before_launch(fn):
    from consistentnerf_amd import ops
    with pytest.raises(ops.CnerfError):
        fn()
    torch.cuda.synchronize()          # (a launch that went wrong would surface here)


def test_what_the_plane_kernels_do_not_take_raises(dev):
    """W = 64, no view directions, an unknown `planes`, the architecture no reference model has, the bf16x3 TRAINING forward on an
    in_chp = 32 network, and render_rays under no_grad with inference_precision set on a W = 64 / direction-free model: CnerfError,
    never a silent fp32 result."""
    from consistentnerf_amd import ops, run_nerf as R
    from test_gpu_fp16x2 import _kwargs
    M = 33
    B, S = P.SHAPES[M]
    pts, dirs = (t.to(dev) for t in P.points(M))
    good = _net(dev, PERWAVE_ONLY)
    some_buffer = good.packed("bf16x3")
    for spec in (ops.NetSpec(D=2, W=64, use_viewdirs=True), ops.NetSpec(D=2, W=128, use_viewdirs=False),
                 ops.NetSpec(*P.UNBUILDABLE[:4], True, 4, P.UNBUILDABLE[4])):
        for mode, planes in ops.PRECISION_PLANES.items():
            if spec.D != 5:
                params = [torch.zeros(s, device=dev) for s in spec.tensor_shapes()]
                _raises_before_launch(lambda: ops.pack_weights_bf(spec, params, planes))
            _raises_before_launch(lambda: ops.mlp_forward_bf(spec, some_buffer, planes, B, S, pts=pts, dirs=dirs))
    for planes in (0, 4, 16, 17, 19, -1):
        _raises_before_launch(lambda: ops.pack_weights_bf(good.spec, good.params, planes))
        _raises_before_launch(lambda: ops.mlp_forward_bf(good.spec, some_buffer, planes, B, S, pts=pts, dirs=dirs))
    _raises_before_launch(lambda: ops.mlp_forward_bf_train(good.spec, some_buffer, B, S, pts=pts, dirs=dirs))
    rays = T(P.I.ray_batch(8, seed=5, near=2.0, far=6.0), dev)
    for vd, W in ((True, 64), (False, 128)):
        coarse, fine = make_model(2, W, vd, 4, 31, dev)[0], make_model(2, W, vd, 4, 32, dev)[0]
        kw = _kwargs(coarse, fine, 8, 8)
        r = rays if vd else rays[:, :8].contiguous()
        with torch.no_grad():
            assert torch.isfinite(R.render_rays(r, **kw)["rgb_map"]).all()          # the exact-fp32 path takes these models
            for prec in ops.PRECISION_PLANES:
                coarse.inference_precision = fine.inference_precision = prec
                _raises_before_launch(lambda: R.render_rays(r, **kw))


# ------------------------------------------------------------------------------------------------ (e) the crafted family
@pytest.mark.parametrize("mode", list(P.TAIL))
@pytest.mark.parametrize("W,L,Lv,which,shift", P.CRAFTED, ids=_id)
def test_crafted_family_kernel_vs_emulation(dev, W, L, Lv, which, shift, mode):
    """Every kept cross term on its own (tests/test_planes_ref_cpu.py shows the CPU half of this).  bound = 4 max(F, A): F the exact-fp32
    kernel's (ops.mlp_forward, same weights) and A the fp32 CPU forward's distance from float64 — neither is code under test.  Asserted
    first, as the precondition: dropping any single kept term moves the emulation by at least 2 x bound.  Then both kernels, where both
    exist, stay within bound of the emulation.  At two planes only sigma is compared (_planes_ref.crafted_columns)."""
    M = 129
    cfg, sd = P.crafted_net(W, L, Lv, mode, which, shift)
    pts, dirs = P.crafted_points(M, mode)
    dpp, col = P.per_point(dirs, M), P.crafted_columns(mode)
    ref = P.forward64(sd, pts, dpp, cfg)
    assert float(ref.min()) > 0.05, "every watched unit is live"
    ref = ref[:, col]
    n = _Net(dev, cfg, sd)
    A = P.rel_dist(P.forward64(sd, pts, dpp, cfg, dtype=torch.float32)[:, col], ref, ref)
    F = P.rel_dist(_run(n, "fp32", M, pts=pts, dirs=dirs).cpu()[:, col], ref, ref)
    bound = 4 * max(A, F)
    emu = P.forward_planes(sd, pts, dpp, cfg, mode)[0][:, col]
    moves = {t: P.rel_dist(P.forward_planes(sd, pts, dpp, cfg, mode, drop=t)[0][:, col], emu, ref) for t in P.terms_of(mode)[1]}
    row = dict(mode=mode, A=A, F=F, bound=bound, E=P.rel_dist(emu, ref, ref), least_mutant_move=min(moves.values()))
    for perwave in ([False, True] if _both_kernels(cfg) else [False]):
        raw = _run(n, mode, M, perwave, pts=pts, dirs=dirs).cpu()
        assert torch.isfinite(raw).all()
        row["perwave" if perwave or not _both_kernels(cfg) else "shared"] = P.rel_dist(raw[:, col], emu, ref)
    kd = {k: v for k, v in row.items() if k in ("shared", "perwave")}
    print(f"  W={W} L={L} {which} shift {shift} {mode}: A {A:.2e} F {F:.2e} bound {bound:.2e}  kernel vs emulation / bound "
          + " ".join(f"{k} {v / bound:.2f}" for k, v in kd.items()) + "  mutant moves / bound " + " ".join(f"{t}:{v / bound:.1f}" for t, v in moves.items()))
    _record("crafted", f"W={W} L={L} {which} shift={shift} {mode}", row)
    assert bound > 0 and all(v >= 2 * bound for v in moves.values()), ("precondition", moves, bound)
    assert all(v <= bound for v in kd.values()), (kd, bound)
