"""tests/_planes_ref.py checked on the CPU: the float64 forward against the oracle on every architecture the GPU file runs, the plane
emulation against the fixed D8W256 restatement it generalises (kept below word for word), and — the point of the file — that the
bound tests/test_gpu_plane_inference.py asserts CAN FAIL: K <= 2 E + 4 A, with E the emulation's and A the fp32 CPU forward's distance
from float64, rejects every mutant of the emulation that loses or mis-pairs a cross term.

Mutants: each kept cross term dropped from every GEMM, (w1, x1) computed in place of (w1, x0), fp16x2 without its low weight plane,
bf16x3 run as two planes.  The three second-order terms of bf16x3 — (0, 2), (1, 1), (2, 0), each 2^-16 of a product with random
signs — pass the bound on the random networks by 1.5x - 4.7x only (measured here with float64 accumulation), so they are shown a second
time on the crafted family (_planes_ref.crafted_net: operands whose planes are all maximal and of one sign, one GEMM at a time),
where every term on its own is 10x or more of the bound."""
import functools

import pytest
import torch

import _planes_ref as P
from oracle import nerf_oracle as O

M = 129


# ------------------------------------------------------------------------------------------------ the D8W256 restatement, verbatim
def _planes_f16(x, flush):
    out = []
    for _ in range(2):
        h = x.to(torch.float16).to(torch.float32)
        if flush:
            h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
        out.append(h)
        x = x - h
    return out


def _planes_bf16(x):
    out = []
    for _ in range(2):
        h = x.to(torch.bfloat16).to(torch.float32)
        out.append(h)
        x = x - h
    return out


def _embed(x, L):
    out = [x]
    for i in range(L):
        out += [torch.sin(x * 2.0 ** i), torch.cos(x * 2.0 ** i)]
    return torch.cat(out, -1)


def _forward_d8w256(sd, pts, dirs, mode, flush=True):
    from consistentnerf_amd import ops
    D = 8
    if mode == "fp16x2":
        sw, sx = ops.FP16X2_WEIGHT_SHIFT, ops.FP16X2_ACT_SHIFT
        wplanes = lambda w: _planes_f16(w * 2.0 ** sw, flush)                 # noqa: E731
        enc = lambda x: _planes_f16(x * 2.0 ** sx, flush)                     # noqa: E731
        act = lambda a: _planes_f16(a * 2.0 ** -sw, flush)                    # noqa: E731
        acc_scale = 2.0 ** (sw + sx)
    else:
        wplanes = _planes_bf16
        enc = act = _planes_bf16
        acc_scale = 1.0
    g = lambda k: torch.as_tensor(sd[k]).float()                             # noqa: E731

    def gemm(wp, xp):
        return xp[0].double() @ wp[0].double().T + xp[1].double() @ wp[0].double().T + xp[0].double() @ wp[1].double().T

    ex, ed = _embed(pts, 10), _embed(dirs, 4)
    w0 = g("pts_linears.0.weight")
    acc = (gemm(wplanes(w0), enc(ex)) + (g("pts_linears.0.bias") * acc_scale).double()).float()
    amax = 0.0
    for l in range(1, D):
        w = g(f"pts_linears.{l}.weight")
        h = torch.relu(acc)
        amax = max(amax, float(h.abs().max()) / acc_scale)
        if l == 5:
            a = gemm(wplanes(w[:, 63:].contiguous()), act(h)) + gemm(wplanes(w[:, :63].contiguous()), enc(ex))
        else:
            a = gemm(wplanes(w), act(h))
        acc = (a + (g(f"pts_linears.{l}.bias") * acc_scale).double()).float()
    h = torch.relu(acc)
    amax = max(amax, float(h.abs().max()) / acc_scale)
    sig = (h.double() @ (g("alpha_linear.weight") / acc_scale).double().T).float() + g("alpha_linear.bias")
    feat = (gemm(wplanes(g("feature_linear.weight")), act(h)) + (g("feature_linear.bias") * acc_scale).double()).float()
    amax = max(amax, float(feat.abs().max()) / acc_scale)
    wv = g("views_linears.0.weight")
    v = (gemm(wplanes(wv[:, :256].contiguous()), act(feat)) + gemm(wplanes(wv[:, 256:].contiguous()), enc(ed))
         + (g("views_linears.0.bias") * acc_scale).double()).float()
    rgb = (torch.relu(v).double() @ (g("rgb_linear.weight") / acc_scale).double().T).float() + g("rgb_linear.bias")
    return torch.cat([rgb, sig], -1), amax


# ------------------------------------------------------------------------------------------------ 1. forward64 and forward_planes
@pytest.mark.parametrize("cfg", list(P.ARCHS), ids=str)
def test_forward64_equals_the_oracle(cfg):
    """Skips, encoding widths (10 / 4, 7 / 2, 4 / 4, 0 / 0 and the identity) and depths 1 .. 16: bit for bit oracle.query in float64."""
    D, W, L, Lv, skip = cfg
    och = P.ARCHS[cfg]
    sd = P.state_dict(cfg, och)
    for m in (129, 33):
        pts, dirs = P.points(m)
        B, S = P.SHAPES[m]
        want = O.query({k: torch.as_tensor(v).double() for k, v in sd.items()}, pts.double().reshape(B, S, 3), dirs.double(),
                       O.NetCfg(D, W, L, Lv, True, och, (skip,))).reshape(m, 4)
        got = P.forward64(sd, pts, P.per_point(dirs, m), cfg)
        assert got.dtype == torch.float64 and torch.equal(got, want), float((got - want).abs().max())


def test_the_unbuildable_architecture_is_unbuildable():
    """(5, 128, 7, 2, 4), D = skip + 1: the oracle's forward mis-shapes (no wide layer is built, the concatenation still happens) and
    the library refuses the spec — P.ARCHS runs (5, 128, 7, 2, 3) in its place."""
    from consistentnerf_amd import ops
    D, W, L, Lv, skip = P.UNBUILDABLE
    sd = P.state_dict(P.UNBUILDABLE)
    pts, dirs = P.points(33)
    with pytest.raises(RuntimeError):
        O.query({k: torch.as_tensor(v).double() for k, v in sd.items()}, pts.double().reshape(3, 11, 3), dirs.double(),
                O.NetCfg(D, W, L, Lv, True, 4, (skip,)))
    spec = ops.NetSpec(D=D, W=W, multires=L, multires_views=Lv, use_viewdirs=True, output_ch=4, skip=skip)
    with pytest.raises(ops.CnerfError):
        spec.tensor_shapes()


@pytest.mark.parametrize("name", ["random_init", "trained_fine", "trained_fine_hot"])
def test_forward_planes_reproduces_the_d8w256_restatement(name):
    """bf16x2, and fp16x2 with subnormals flushed and kept, on the three D8W256 fixtures of tests/test_fp16x2_cpu.py: raw and the
    largest activation bit for bit."""
    from test_fp16x2_cpu import _nets
    nets, dirs = _nets()
    sd, pts = nets[name]
    cfg = (8, 256, 10, 4, 4)
    for mode, flush in (("bf16x2", False), ("fp16x2", True), ("fp16x2", False)):
        want, amax_w = _forward_d8w256(sd, pts, dirs, mode, flush)
        got, amax_g = P.forward_planes(sd, pts, dirs, cfg, mode, flush=flush)
        assert torch.equal(got, want) and amax_g == amax_w, (mode, flush, float((got - want).abs().max()))


def test_term_sets_are_the_kernels():
    """products<NP> of csrc/mlp_bf_common.hpp keeps the (weight plane i, input plane j) with i + j < NP."""
    for mode, NP in (("bf16", 1), ("bf16x2", 2), ("bf16x3", 3), ("fp16x2", 2)):
        n, terms = P.terms_of(mode)
        assert n == NP and sorted(terms) == sorted((i, j) for i in range(NP) for j in range(NP) if i + j < NP)
    assert P.terms_of("bf16x3", drop=(1, 1))[1] == [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0)]
    assert P.terms_of("bf16x2", pair=((1, 0), (1, 1)))[1] == [(0, 0), (0, 1), (1, 1)]
    assert P.terms_of("fp16x2", drop=[(0, 1), (1, 0)])[1] == [(0, 0)]


# ------------------------------------------------------------------------------------------------ 2. the bound can fail
@functools.lru_cache(maxsize=None)
def _case(cfg):
    """-> (sd, pts, per-point dirs, raw64, scale, A) of one architecture at M = 129."""
    sd = P.state_dict(cfg, P.ARCHS[cfg])
    pts, dirs = P.points(M)
    dirs = P.per_point(dirs, M)
    ref = P.forward64(sd, pts, dirs, cfg)
    scale = max(1.0, float(ref.abs().max()))
    return sd, pts, dirs, ref, scale, P.dist(P.forward64(sd, pts, dirs, cfg, dtype=torch.float32), ref, scale)


@functools.lru_cache(maxsize=None)
def _E(cfg, mode, drop=None, pair=None):
    sd, pts, dirs, ref, scale, _ = _case(cfg)
    return P.dist(P.forward_planes(sd, pts, dirs, cfg, mode, drop=drop, pair=pair)[0], ref, scale)


MUTANTS = [(mode, dict(drop=t), mode) for mode in P.MODES for t in P.terms_of(mode)[1]]
MUTANTS += [(mode, dict(pair=((1, 0), (1, 1))), mode) for mode in ("bf16x2", "bf16x3", "fp16x2")]
MUTANTS += [("bf16x2", {}, "bf16x3")]      # bf16x3 run as two planes: the two-plane result held to the three-plane bound
# ("fp16x2 without the low weight plane" is drop = (1, 0) of fp16x2, in the first list)


def test_the_mutant_list_is_the_stated_one():
    drops = [(m, kw["drop"]) for m, kw, _ in MUTANTS if "drop" in kw]
    assert drops == [("bf16", (0, 0)), ("bf16x2", (0, 0)), ("bf16x2", (0, 1)), ("bf16x2", (1, 0)), ("bf16x3", (0, 0)), ("bf16x3", (0, 1)),
                     ("bf16x3", (1, 0)), ("bf16x3", (0, 2)), ("bf16x3", (1, 1)), ("bf16x3", (2, 0)), ("fp16x2", (0, 0)), ("fp16x2", (0, 1)), ("fp16x2", (1, 0))]


@pytest.mark.parametrize("cfg", list(P.ARCHS), ids=str)
def test_fp32_forward_and_emulation_are_where_the_bound_assumes(cfg):
    """A <= 2e-6 (the inputs are well conditioned: the convention of test_composite_vs_float64) and E <= the mode's tier, on the CPU."""
    A = _case(cfg)[5]
    Es = {mode: _E(cfg, mode) for mode in P.MODES}
    print(f"  {cfg}: A {A:.2e}  " + "  ".join(f"E[{m}] {e:.2e}" for m, e in Es.items()))
    assert A <= 2e-6
    assert all(Es[m] <= P.TIERS[m] for m in P.MODES), Es


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: f"{m[0]}-{m[1]}-as-{m[2]}".replace(" ", ""))
def test_every_mutant_violates_the_bound_on_half_of_the_architectures(mutant):
    mode, kw, held_to = mutant
    rows = []
    for cfg in P.ARCHS:
        bound = 2 * _E(cfg, held_to) + 4 * _case(cfg)[5]
        rows.append((cfg, _E(cfg, mode, **kw) / bound))
    caught = sum(r > 1.0 for _, r in rows)
    print(f"  {mode} {kw} held to {held_to}: E_mutant / (2 E + 4 A) " + " ".join(f"{r:.3g}" for _, r in rows) + f"  -> {caught} of {len(rows)}")
    assert 2 * caught >= len(rows), rows


# ------------------------------------------------------------------------------------------------ 3. the crafted family
def test_crafted_values_split_into_maximal_planes_exactly():
    for mode, (tail, bits) in P.TAIL.items():
        x = torch.from_numpy(P.crafted((64, 3), mode, -3, 1, 9))      # (fp16x2: both scaled planes stay fp16 normals)
        NP = 2 if mode == "fp16x2" else int(mode[-1])
        pl = P.planes_f16(x * 16.0, False) if mode == "fp16x2" else P.planes_bf16(x, NP)
        assert torch.equal(sum(p.double() for p in pl).float(), x * (16.0 if mode == "fp16x2" else 1.0)), mode
        assert all(bool((p > 0).all()) for p in pl), mode
        step = 2.0 ** -11 if mode == "fp16x2" else 2.0 ** -8          # plane p is between a quarter of step^p of the operand and step^p
        for p in range(1, NP):
            r = pl[p] / pl[0]
            assert float(r.min()) >= 0.24 * step ** p and float(r.max()) <= step ** p, (mode, p, float(r.min()), float(r.max()))


CRAFTED = P.CRAFTED


@pytest.mark.parametrize("mode", list(P.TAIL))
@pytest.mark.parametrize("W,L,Lv,which,shift", CRAFTED)
def test_crafted_family_shows_every_single_term(W, L, Lv, which, shift, mode):
    """On the crafted networks every kept term dropped, second-order ones included, moves the emulation by at least 2 x (4 A), elementwise relative to raw: twice
    the CPU half of the bound the GPU test holds the kernel to (there the fp32 kernel's own distance joins the maximum).  The
    emulation itself stays within 4 A of float64: the terms it drops by design are below 2^-24 of a product."""
    cfg, sd = P.crafted_net(W, L, Lv, mode, which, shift)
    pts, dirs = P.crafted_points(M, mode)
    dirs = P.per_point(dirs, M)
    ref = P.forward64(sd, pts, dirs, cfg)
    assert float(ref.min()) > 0.05, "every watched unit is live"
    col = P.crafted_columns(mode)
    ref = ref[:, col]
    A = P.rel_dist(P.forward64(sd, pts, dirs, cfg, dtype=torch.float32)[:, col], ref, ref)
    emu = P.forward_planes(sd, pts, dirs, cfg, mode)[0][:, col]
    bound = 4 * A
    moves = {t: P.rel_dist(P.forward_planes(sd, pts, dirs, cfg, mode, drop=t)[0][:, col], emu, ref) for t in P.terms_of(mode)[1]}
    print(f"  W={W} L={L} {which} shift {shift} {mode}: raw in [{float(ref.min()):.3g}, {float(ref.max()):.3g}] A {A:.2e} E {P.rel_dist(emu, ref, ref):.2e}  "
          "moves / bound " + " ".join(f"{t}:{v / bound:.1f}" for t, v in moves.items()))
    assert A > 0 and all(v >= 2 * bound for v in moves.values()), moves


# ------------------------------------------------------------------------------------------------ 4. the fp16x2 range families
@pytest.mark.parametrize("cfg", P.RANGE_CFGS, ids=str)
def test_cold_layers_need_fp16_subnormals_and_the_wide_family_is_wide(cfg):
    """What DESIGN 7a states of a cold layer: the emulation that keeps fp16 subnormals is inside 2e-5, the one that flushes them is
    over it — so the GPU test of these networks decides whether the whole path keeps them.  And the precondition of the wide family:
    a weight of exactly 200 and hidden activations between 1000 and the 4094 limit, all four families inside the stated range."""
    from consistentnerf_amd import ops
    pts, dirs = P.points(M)
    dirs = P.per_point(dirs, M)
    for family in P.RANGE_FAMILIES:
        sd = P.range_net(cfg, family)
        ref = P.forward64(sd, pts, dirs, cfg)
        scale = max(1.0, float(ref.abs().max()))
        kept, amax = P.forward_planes(sd, pts, dirs, cfg, "fp16x2")
        flushed, _ = P.forward_planes(sd, pts, dirs, cfg, "fp16x2", flush=True)
        e_kept, e_flush = P.dist(kept, ref, scale), P.dist(flushed, ref, scale)
        wmax = max(float(abs(v).max()) for k, v in sd.items() if k.endswith(".weight") and k.split(".")[0] not in ("alpha_linear", "rgb_linear"))
        print(f"  {cfg} {family}: max|w| {wmax:.4g} max|activation| {amax:.4g}  subnormals kept {e_kept:.2e}  flushed {e_flush:.2e}")
        assert wmax < ops.FP16X2_MAX_WEIGHT and amax < ops.FP16X2_MAX_ACTIVATION and torch.isfinite(kept).all()
        assert e_kept <= 2e-5
        if family.startswith("cold"):
            assert e_flush > 2e-5
        if family == "wide":
            assert wmax == 200.0 and amax >= 1000.0
