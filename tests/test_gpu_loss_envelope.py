"""The kernels at the end of the step over their size range, against float64 (tests/_loss_ref.py; its statements, bounds and input
families are checked without a GPU by tests/test_loss_ref_cpu.py):

  masked loss   masked_loss_k (one workgroup) and masked_part_k + masked_fin_k (B > 16384 with a workspace), B = 1 ... 49153, five
                kinds of mask, depth term on / off, local / global counts, g_scale 1 / 0.125: values and EVERY seed element inside
                the derived bounds, NaN patterns, guard tails, the two routes against each other, shards under global counts
  MSE           mse_k and mse_part_k + mse_fin_k through the C ABI (cnerf_mse_ws takes two stages from 16385 elements, ops.mse from
                65537: the window between is reached here only)
  soft forms    soft_lp_k, softmask_k: n = 1 ... 5000, three exponents / temperatures, exact-zero residuals, overflowing weights;
                yardstick 4 A + floor (A = the fp32 ATen lines' own distance from float64)
  patch term    patch_depth_loss_k: (P, n) = (1, 1) ... (16, 1000), four input families, same yardstick
  folded tail   closs_tail_k behind composite_fwd_k at S = 4, B = 1 ... 16392 (1025 partials from B = 8193: the summing loop's second
                pass), every finish; seed weights bit for bit against the stand-alone kernel's
  Adam          adam_k and adam_dev_k, n = 1 ... 2 * 4096 * 256 + 77 (the grid-stride loop's second and third pass), warm moments,
                under- / overflowing, clipped, infinite and NaN gradients: BIT FOR BIT against the numpy float32 restatement, and per
                element inside a derived bound of the float64 step

Every figure is printed; with CNERF_RECORD_DIR naming a directory they go to loss_envelope.json there (profiles/loss_envelope.json is
the MI355X run this file was written against).  Shapes are small but for B or n: no networks, S = 4 samples where compositing is needed.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _inputs as I
import _loss_ref as R

pytestmark = pytest.mark.gpu

torch.set_num_threads(4)
GUARD = 64          # NaN-filled elements behind every buffer a kernel writes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """Bit for bit; a NaN equals a NaN of any sign and payload (IEEE leaves both to the implementation)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def ulps(a, b):
    """Distance of two finite floats of one sign in units of the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def put(row, key, got, ref, bound):
    """row["K/bound x"] = the largest |got - ref| / bound over the elements, with that element's distance ("K x") and bound ("bound x")."""
    got, ref, bound = (np.atleast_1d(np.asarray(a, np.float64)).reshape(-1) for a in (got, ref, bound))
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)
        r = np.where(np.isfinite(ref) & np.isfinite(bound), np.where(d == 0, 0.0, d / bound), 0.0)
    i = int(np.argmax(r)) if r.size else 0
    name = key[len("K/bound "):]
    row[key] = float(r[i]) if r.size else 0.0
    row["K " + name], row["bound " + name] = (float(d[i]), float(bound[i])) if r.size else (0.0, 0.0)


def inside(row):
    return all(v <= 1.0 for k, v in row.items() if k.startswith("K/bound"))


RECORD = {}
_MUTANTS = {}


def _record(section, key, row):
    RECORD.setdefault(section, {})[key] = row
    out_dir = os.environ.get("CNERF_RECORD_DIR")
    if not out_dir:
        return
    if not _MUTANTS:
        rows = [r for r in R.mutant_ratios(large_adam=False)]
        least = {}
        for fam, mu, _case, r in rows:
            least[f"{fam}.{mu}"] = min(least.get(f"{fam}.{mu}", float("inf")), r)
        _MUTANTS.update({k: (v if np.isfinite(v) else "inf") for k, v in least.items()})
        _MUTANTS["least"] = min(v for v in least.values())
    worst = {}
    for sec, cases in RECORD.items():
        for row in cases.values():
            for k, v in row.items():
                if k.startswith("K/bound"):
                    worst[sec] = max(worst.get(sec, 0.0), v)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "loss_envelope.json"), "w") as f:
        json.dump({"bounds": "tests/_loss_ref.py: derived per quantity (masked, mse, adam); 4 A + floor (soft forms, patch term)",
                   "worst_K_over_bound": worst, "least_mutant_ratio_cpu": _MUTANTS,
                   "bit_equality_not_held": RECORD.get("bit_equality_not_held", {}), "cases": RECORD}, f, indent=1, sort_keys=True)


# ================================================================================================ masked loss
def masked_call(dev, kw, route="auto", guard=GUARD):
    """cnerf_masked_loss through the C ABI on buffers with NaN-filled guard tails -> dict(img, dep, d_rgb, d_depth | None) as numpy.
    route: "auto" = a workspace above 16384 rays, as ops.masked_loss allocates; "one" = no workspace (one workgroup whatever B);
    "ws" = a workspace whatever B."""
    from consistentnerf_amd import _lib
    lib = _lib.load()
    B = kw["rgb"].shape[0]
    t = {k: (None if kw[k] is None else T(kw[k], dev)) for k in ("rgb", "tgt", "depth", "prior", "mask", "counts")}
    loss = torch.full((2 + guard,), float("nan"), device=dev)
    d_rgb = torch.full((3 * B + guard,), float("nan"), device=dev)
    d_depth = torch.full((B + guard,), float("nan"), device=dev) if kw["depth"] is not None else None
    ws = None
    if route == "ws" or (route == "auto" and B > R.MASKED_CHUNK):
        ws = torch.empty(lib.cnerf_loss_ws_floats() // 2, device=dev, dtype=torch.float64)
    _lib.check(lib.cnerf_masked_loss(_p(t["rgb"]), _p(t["tgt"]), _p(t["depth"]), _p(t["prior"]), _p(t["mask"]), B, float(kw["far"]),
                                     float(kw["coef"]), _p(t["counts"]), float(kw["g_scale"]), _p(loss), _p(d_rgb), _p(d_depth), _p(ws),
                                     _stream()), "cnerf_masked_loss")
    loss, d_rgb = N(loss), N(d_rgb)
    assert np.isnan(loss[2:]).all() and np.isnan(d_rgb[3 * B:]).all(), "a write past the end of loss / d_rgb"
    out = dict(img=float(loss[0]), dep=float(loss[1]), d_rgb=d_rgb[:3 * B].reshape(B, 3), d_depth=None)
    if d_depth is not None:
        d_depth = N(d_depth)
        assert np.isnan(d_depth[B:]).all(), "a write past the end of d_depth"
        out["d_depth"] = d_depth[:B]
    return out


def check_masked(got, kw, tag):
    """Values and every seed element inside the derived bounds; the NaN pattern of the float64 lines; exact zeros off the sets."""
    ref, bnd = R.masked64(**kw), R.masked_bounds(**kw)
    keys = ("img", "d_rgb") + (("dep", "d_depth") if kw["depth"] is not None else ())
    row = {}
    for k in keys:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (tag, k, "NaN pattern")
        assert np.array_equal(np.isinf(got[k]), np.isinf(ref[k])), (tag, k, "inf pattern")
        put(row, "K/bound " + k, got[k], ref[k], bnd[k])
    m = np.ones(kw["rgb"].shape[0], np.float32) if kw["mask"] is None else kw["mask"]
    neither = (m != 0) & (m != 1)
    assert not got["d_rgb"][neither].any(), (tag, "a colour seed on a ray of neither set")
    if kw["depth"] is not None:
        assert not got["d_depth"][m != 1].any(), (tag, "a depth seed off the m == 1 set")
    else:
        assert got["dep"] == 0.0
    assert inside(row), (tag, row)
    return row


@pytest.mark.parametrize("B", R.MASKED_SIZES, ids=lambda B: f"B{B}-" + ("multi-workgroup" if B > R.MASKED_CHUNK else "one-workgroup"))
def test_masked_loss_inside_derived_bounds(dev, B):
    """Every mask kind x (depth term, global counts, g_scale) at one size.  B > 16384 takes masked_part_k + masked_fin_k: 2 workgroups with
    a one-ray tail (16385), 2 full ones (32768), 4 with a one-ray tail (49153)."""
    from consistentnerf_amd import ops
    worst = {}
    for mask_kind in R.MASK_KINDS:
        for wd, wc, gs in R.masked_variants():
            kw = R.masked_case(B, mask_kind, wd, wc, gs)
            tag = f"B{B}-{mask_kind}-depth{int(wd)}-counts{int(wc)}-g{gs}"
            got = masked_call(dev, kw)
            row = check_masked(got, kw, tag)
            for q in ("img", "d_rgb", "dep", "d_depth"):                 # per quantity the combination nearest to its bound
                if "K/bound " + q in row and row["K/bound " + q] >= worst.get("K/bound " + q, -1.0):
                    worst.update({k + q: row[k + q] for k in ("K/bound ", "K ", "bound ")})
                    worst["at " + q] = tag
            if mask_kind == "zeros" and not wc:
                assert np.isnan(got["img"]) and (not wd or np.isnan(got["dep"])) and np.isfinite(got["d_rgb"]).all(), tag   # N1 = 0
    # the route Python callers take gives the same bits
    kw = R.masked_case(B, "mixed", True, False, 1.0)
    got = masked_call(dev, kw)
    loss, d_rgb, d_depth = ops.masked_loss(T(kw["rgb"], dev), T(kw["tgt"], dev), T(kw["depth"], dev), T(kw["prior"], dev), T(kw["mask"], dev),
                                           kw["far"], kw["coef"])
    assert same_bits(N(loss), [got["img"], got["dep"]]) and same_bits(N(d_rgb), got["d_rgb"]) and same_bits(N(d_depth), got["d_depth"])
    print(f"masked B={B}: worst K / bound {worst}")
    _record("masked", f"B{B}", worst)


@pytest.mark.parametrize("B", [16385, 49153], ids=lambda B: f"B{B}-multi-workgroup-vs-one-workgroup")
def test_masked_loss_routes_agree(dev, B):
    """Without a workspace the entry point runs one workgroup whatever B, with one the chunked route: the seeds are bit-equal (same
    counts, same code), the values within one fp32 ulp (the fp64 sums associate differently), two launches of either bit-identical."""
    for mask_kind, wc in (("mixed", False), ("odd", True)):
        kw = R.masked_case(B, mask_kind, True, wc, 1.0)
        one, one2 = masked_call(dev, kw, "one"), masked_call(dev, kw, "one")
        ws, ws2 = masked_call(dev, kw, "ws"), masked_call(dev, kw, "ws")
        check_masked(one, kw, f"B{B}-one-workgroup")
        for k in ("d_rgb", "d_depth"):
            assert same_bits(one[k], ws[k]), k
        for a, b in ((one, one2), (ws, ws2)):
            assert a["img"] == b["img"] and a["dep"] == b["dep"] and same_bits(a["d_rgb"], b["d_rgb"]) and same_bits(a["d_depth"], b["d_depth"])
        du = {k: ulps(one[k], ws[k]) for k in ("img", "dep")}
        print(f"masked routes B={B} {mask_kind}: ulps between the routes' values {du}")
        assert max(du.values()) <= 1, du
        _record("masked_routes", f"B{B}-{mask_kind}", {"ulps " + k: v for k, v in du.items()})


def test_masked_loss_shards_under_global_counts_multi_workgroup(dev):
    """B = 49153 cut at 16385, both shards called with the whole batch's counts: the shards' losses add up to the float64 statement of
    the whole within the shards' own bounds (and to the single call within those + its own), their seeds concatenate to the single
    call's bit for bit."""
    B, cut = 49153, 16385
    kw = R.masked_case(B, "mixed", True, False, 1.0)
    kw["counts"] = np.array([(kw["mask"] == 1).sum(), (kw["mask"] == 0).sum()], np.float32)
    full = masked_call(dev, kw)
    ref = R.masked64(**kw)
    parts, bounds = [], []
    for sl in (slice(0, cut), slice(cut, B)):
        k2 = dict(kw, **{k: kw[k][sl] for k in ("rgb", "tgt", "depth", "prior", "mask")})
        parts.append(masked_call(dev, k2))
        bounds.append(R.masked_bounds(**k2))
    for k in ("img", "dep"):
        s = parts[0][k] + parts[1][k]
        b = bounds[0][k] + bounds[1][k]
        print(f"masked shards {k}: sum {s!r} float64 {ref[k]!r} single call {full[k]!r} bound {b:.3e}")
        assert abs(s - ref[k]) <= b and abs(s - full[k]) <= b + R.masked_bounds(**kw)[k]
        _record("masked_shards", k, {"K": abs(s - ref[k]), "bound": b, "K/bound": abs(s - ref[k]) / b})
    assert same_bits(np.concatenate([parts[0]["d_rgb"], parts[1]["d_rgb"]]), full["d_rgb"])
    assert same_bits(np.concatenate([parts[0]["d_depth"], parts[1]["d_depth"]]), full["d_depth"])


# ================================================================================================ MSE
def mse_call(dev, x, y, entry, want_seed=True, with_ws=True):
    from consistentnerf_amd import _lib
    lib = _lib.load()
    n = x.size
    xt, yt = T(x, dev), T(y, dev)
    loss = torch.full((1 + GUARD,), float("nan"), device=dev)
    d_x = torch.full((n + GUARD,), float("nan"), device=dev) if want_seed else None
    if entry == "cnerf_mse":
        _lib.check(lib.cnerf_mse(_p(xt), _p(yt), n, _p(loss), _p(d_x), _stream()), entry)
    else:
        ws = torch.empty(max(1, lib.cnerf_mse_ws_floats(n) // 2), device=dev, dtype=torch.float64) if with_ws else None
        _lib.check(lib.cnerf_mse_ws(_p(xt), _p(yt), n, _p(loss), _p(d_x), _p(ws), _stream()), entry)
    loss = N(loss)
    assert np.isnan(loss[1:]).all()
    if d_x is None:
        return float(loss[0]), None
    d_x = N(d_x)
    assert np.isnan(d_x[n:]).all(), "a write past the end of d_x"
    return float(loss[0]), d_x[:n]


def _mse_id(n):
    return f"n{n}-" + ("one-workgroup" if n <= 16384 else "ws-window-16385-65536" if n <= 65536 else "ws-beyond-65536")


@pytest.mark.parametrize("n", R.MSE_SIZES, ids=_mse_id)
def test_mse_both_entry_points_inside_derived_bounds(dev, n):
    """cnerf_mse (one workgroup at any n) and cnerf_mse_ws (two stages above 16384 elements WITH a workspace, one workgroup without):
    value within 4 u, every seed element within 3 u; the seeds of the two forms bit-equal; d_x may be null."""
    x, y = R.mse_inputs(n)
    (v, s), (bv, bs) = R.mse64(x, y), R.mse_bounds(x, y)
    one = mse_call(dev, x, y, "cnerf_mse")
    two = mse_call(dev, x, y, "cnerf_mse_ws")
    fallback = mse_call(dev, x, y, "cnerf_mse_ws", with_ws=False)
    row = {}
    for name, (gv, gsd) in (("one", one), ("ws", two)):
        put(row, f"K/bound value {name}", gv, v, bv)
        put(row, f"K/bound seed {name}", gsd, s, bs)
    assert same_bits(one[1], two[1]) and same_bits(one[1], fallback[1]) and fallback[0] == one[0]
    for entry in ("cnerf_mse", "cnerf_mse_ws"):
        gv, none = mse_call(dev, x, y, entry, want_seed=False)
        assert none is None and gv == (one[0] if entry == "cnerf_mse" else two[0])
    row["ulps one vs ws"] = ulps(one[0], two[0])
    print(f"mse n={n}: {row}")
    assert inside(row) and row["ulps one vs ws"] <= 1, row
    _record("mse", f"n{n}", row)


# ================================================================================================ soft-Lp / softmask
def _soft_check(tag, got, ref, A, bnd, x, y):
    gmax = float(np.abs(ref[1]).max())
    row = {"A loss": A[0], "A seed": A[1]}
    put(row, "K/bound loss", got[0], ref[0], bnd[0])
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all(), (tag, "finite where the float64 lines are")
    assert not got[1][x == y].any(), (tag, "an exact-zero residual has a zero seed")
    put(row, "K/bound seed", got[1], ref[1], np.full(ref[1].shape, bnd[1] * gmax))          # relative to max|seed|
    if len(ref) == 3:
        assert np.isfinite(got[2])
        row["A d_temp"] = A[2]
        put(row, "K/bound d_temp", got[2], ref[2], bnd[2])
    return row


@pytest.mark.parametrize("n", R.SOFT_SIZES)
def test_soft_forms_standalone_within_4A(dev, n):
    """soft_lp_k at coef 0.5 / 1 / 2 and softmask_k at temp 0.05 / 0.3 / 5 on residuals in [-1, 1] with a block of exact zeros: loss,
    seed (relative to max|seed|) and d / d temp within 4 A + floor."""
    from consistentnerf_amd import ops
    x, y = R.soft_inputs(n)
    xt, yt = T(x, dev), T(y, dev)
    worst = {}
    for coef in R.SOFT_COEFS:
        ref, A, bnd = R.soft_yardstick("softlp", x, y, coef)
        L, d = ops.soft_lp_loss(xt, yt, coef)
        row = _soft_check(f"softlp n{n} coef{coef}", (float(L), N(d).astype(np.float64)), ref, A, bnd, x, y)
        print(f"softlp n={n} coef={coef}: {row}")
        _record("softlp", f"n{n}-coef{coef}", row)
        worst.update({k: max(worst.get(k, 0.0), v) for k, v in row.items() if k.startswith("K/")})
    for t in R.SOFT_TEMPS:
        ref, A, bnd = R.soft_yardstick("softmask", x, y, t)
        L, d, dt = ops.softmask_loss(xt, yt, torch.tensor([t], device=dev))
        row = _soft_check(f"softmask n{n} t{t}", (float(L), N(d).astype(np.float64), float(dt)), ref, A, bnd, x, y)
        print(f"softmask n={n} temp={t:.3g}: {row}")
        _record("softmask", f"n{n}-temp{t:.3g}", row)
        worst.update({k: max(worst.get(k, 0.0), v) for k, v in row.items() if k.startswith("K/")})
    assert inside(worst), worst


def test_softmask_overflowing_weights_match_aten_fp32_pattern(dev):
    """Three residuals of 1 at temp 0.01 (d^2 / t = 100 > 89: exp overflows in fp32), the others within 0.5 (d^2 / t <= 25): the
    non-finite pattern of value, seeds and d / d temp equals the fp32 ATen lines' on the CPU."""
    from consistentnerf_amd import ops
    x, y = R.soft_inputs(1025)
    x = (y + 0.5 * (x - y)).astype(np.float32)
    x[[3, 600, 1024]] = y[[3, 600, 1024]] + np.float32(1.0)
    t = R.f32(0.01)
    L32, g32, dt32 = R.softmask_aten(x, y, t, torch.float32)
    L, d, dt = ops.softmask_loss(T(x, dev), T(y, dev), torch.tensor([t], device=dev))
    L, d, dt = float(L), N(d), float(dt)
    print(f"softmask overflow: kernel L {L} d_temp {dt} non-finite seeds {int((~np.isfinite(d)).sum())}; ATen fp32 L {L32} d_temp {dt32} "
          f"non-finite seeds {int((~np.isfinite(g32)).sum())}")
    assert not np.isfinite(L32) and (~np.isfinite(g32)).sum() >= 3
    assert np.isnan(L) == np.isnan(L32) and np.isinf(L) == np.isinf(L32) and np.isnan(dt) == np.isnan(dt32) and np.isinf(dt) == np.isinf(dt32)
    assert np.array_equal(np.isnan(d), np.isnan(g32)) and np.array_equal(np.isinf(d), np.isinf(g32))


# ================================================================================================ patch term
def check_patch(tag, L, g, depth, mono, P, n):
    """loss and per-patch gradient within 4 A + floor of oracle.patch_depth_loss in float64; NaN pattern equal; n = 1: exact zeros."""
    L64, g64 = R.patch_lines(depth, mono, P, n, torch.float64)
    L32, g32 = R.patch_lines(depth, mono, P, n, torch.float32)
    assert np.array_equal(np.isnan(g), np.isnan(g64)), (tag, "NaN pattern")
    if n == 1:
        assert L == 0.0 and L64 == 0.0 and not g.any() and not g64.any(), tag
        return {"K/bound loss": 0.0, "K/bound grad": 0.0}
    A = abs(L32 - L64)
    with np.errstate(all="ignore"):
        kl = float(np.float64(abs(L - L64)) / np.float64(4 * A + R.PATCH_FLOOR * abs(L64))) if L != L64 else 0.0
    row = {"A loss": A, "K loss": abs(L - L64), "bound loss": 4 * A + R.PATCH_FLOOR * abs(L64), "K/bound loss": kl, "K/bound grad": 0.0,
           "A grad": 0.0, "K grad": 0.0, "bound grad": 0.0}
    for p in range(P):
        sl = slice(p * n, (p + 1) * n)
        gmax = np.nanmax(np.abs(g64[sl]))
        if gmax == 0:
            assert not np.nan_to_num(g[sl]).any(), (tag, p, "a gradient where the float64 lines have none")
            continue
        Ap = np.nanmax(np.abs(g32[sl] - g64[sl])) / gmax
        k = np.nanmax(np.abs(g[sl] - g64[sl])) / gmax
        row["A grad"] = max(row["A grad"], float(Ap))
        if k / (4 * Ap + R.PATCH_FLOOR) >= row["K/bound grad"]:                  # of max|g| of the patch
            row.update({"K/bound grad": float(k / (4 * Ap + R.PATCH_FLOOR)), "K grad": float(k), "bound grad": float(4 * Ap + R.PATCH_FLOOR)})
    assert row["K/bound loss"] <= 1.0 and row["K/bound grad"] <= 1.0, (tag, row)
    return row


@pytest.mark.parametrize("P,n", R.PATCH_SIZES)
def test_patch_term_standalone_within_4A(dev, P, n):
    """patch_depth_loss_k, one wave per patch: n < 64 (lanes with no element), n no multiple of 64, P = 1 ... 16; mild / invalid /
    quantised inputs, a patch without a valid prior and one of equal depths (P >= 3); g_scale scales the gradient and not the value."""
    from consistentnerf_amd import ops
    for fam in R.PATCH_FAMILIES:
        if fam == "special" and P < 3:
            continue
        depth, mono = R.patch_inputs(P, n, fam)
        L, g = ops.patch_depth_loss(T(depth, dev), T(mono, dev), P, n)
        row = check_patch(f"P{P} n{n} {fam}", float(L), N(g).astype(np.float64), depth, mono, P, n)
        L8, g8 = ops.patch_depth_loss(T(depth, dev), T(mono, dev), P, n, g_scale=0.125)
        assert float(L8) == float(L) and same_bits(N(g8), N(g) * np.float32(0.125)), "g_scale"
        print(f"patch P={P} n={n} {fam}: {row}")
        _record("patch", f"P{P}-n{n}-{fam}", row)


def test_patch_term_rejects_17_patches(dev):
    from consistentnerf_amd import ops
    from consistentnerf_amd._lib import CnerfError
    depth, mono = R.patch_inputs(17, 8, "mild")
    with pytest.raises(CnerfError):
        ops.patch_depth_loss(T(depth, dev), T(mono, dev), 17, 8)


# ================================================================================================ folded tail
S = 4
TAIL_SIZES = (1, 7, 8, 9, 8184, 8192, 8193, 8200, 16392)


def _tail_id(B):
    return f"B{B}-{(B + 7) // 8}-partials" + ("-second-pass" if (B + 7) // 8 > 1024 else "")


def tail_batch(dev, B, seed=0):
    """raw [B, S, 4], z [B, S], rays [B, 11] on the device + the masked_inputs family's target / prior / mask (numpy)."""
    g = torch.Generator(device="cpu").manual_seed(300 + B + seed)
    raw = (torch.randn(B, S, 4, generator=g) * 3).to(dev)
    z = torch.sort(torch.rand(B, S, generator=g) * (R.FAR - R.NEAR) + R.NEAR, -1).values.to(dev)
    rays = T(I.ray_batch(B, seed=B + seed, near=R.NEAR, far=R.FAR), dev)
    d = R.masked_inputs(B, "mixed", seed=seed)
    return raw, z, rays, d


def standalone_weights(dev, mask, counts=None):
    """(w1, w0, wd) of masked_loss_k for this mask as float32 bits: its seeds on maps whose every residual is exactly 1 (the weights
    depend on the counts alone)."""
    B = mask.shape[0]
    kw = dict(rgb=np.ones((B, 3), np.float32), tgt=np.zeros((B, 3), np.float32), depth=np.full(B, R.FAR, np.float32),
              prior=np.zeros(B, np.float32), mask=mask, far=R.FAR, coef=R.COEF, counts=counts, g_scale=1.0)
    got = masked_call(dev, kw, "one")
    w1 = got["d_rgb"][mask == 1][0, 0] if (mask == 1).any() else None
    w0 = got["d_rgb"][mask == 0][0, 0] if (mask == 0).any() else np.float32(0)
    wd = got["d_depth"][mask == 1][0] if (mask == 1).any() else None
    return w1, w0, wd


def check_d_raw(dev, tag, d_raw, raw, z, rays, g_rgb, g_depth):
    """d_raw against cnerf_composite_bwd fed with given float64-derived seeds: 2e-6 of its largest element (each seed is <= 6 fp32
    operations from its float64 value: the bound of test_gpu_lossforms.py)."""
    from consistentnerf_amd import ops
    want = ops.composite_backward(raw, z, rays, None, False, T(np.asarray(g_rgb, np.float32), dev), None, None,
                                  None if g_depth is None else T(np.asarray(g_depth, np.float32), dev))
    dist, scale = float((d_raw.double() - want.double()).abs().max()), float(want.abs().max())
    print(f"{tag}: d_raw max|d| {dist:.3e} of {scale:.3e}")
    assert torch.isfinite(d_raw).all() and dist <= 2e-6 * scale
    return dist / (2e-6 * scale) if scale > 0 else 0.0


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("B", TAIL_SIZES, ids=_tail_id)
def test_folded_tail_hardmask_finish(dev, B, levels):
    """composite_fwd_k's partials -> closs_tail_k -> composite_bwd_k at the partial counts around one sweep of the tail's 1024 threads:
    the levels' terms inside the derived bounds of the float64 lines on the maps the forward returned, the seed weights in `stats` the
    stand-alone kernel's bit for bit, d_raw against the plain compositing backward fed with the float64 seeds.  (The step tests stay at
    or under 1024 partials: 5120 rays in the C3 steps, 8192 rows in the one-render consistency step.)"""
    from consistentnerf_amd import ops
    row = {}
    batches = [tail_batch(dev, B, seed=lv) for lv in range(levels)]
    d = batches[0][3]
    L = ops.ClossSpec(T(d["tgt"], dev), T(d["mask"], dev), T(d["prior"], dev), R.FAR, R.COEF, 1.0, 1.0, 0.0).checked(B)
    fw = [ops.composite_forward_closs(raw, z, rays, None, False, L, level=lv) for lv, (raw, z, rays, _d) in enumerate(batches)]
    assert fw[0][5].numel() == 5 * ((B + 7) // 8)
    fin = ops.closs_finish(L, B, fw[0][5], fw[1][5] if levels == 2 else None, fw[0][4], fw[1][4] if levels == 2 else None)
    terms, stats = N(fin.terms), N(fin.stats)
    w1, w0, wd = standalone_weights(dev, d["mask"])
    total = bsum = 0.0
    for lv in range(levels):
        rgb, depth = N(fw[lv][0]), N(fw[lv][4])
        kw = dict(rgb=rgb, tgt=d["tgt"], depth=depth, prior=d["prior"], mask=d["mask"], far=R.FAR, coef=R.COEF, counts=None, g_scale=1.0)
        ref, bnd = R.masked64(**kw), R.masked_bounds(**kw)
        put(row, f"K/bound img level {lv}", terms[1 + 3 * lv], ref["img"], bnd["img"])
        put(row, f"K/bound dep level {lv}", terms[2 + 3 * lv], ref["dep"], bnd["dep"])
        total += ref["img"] + ref["dep"]
        bsum += bnd["img"] + bnd["dep"]
        assert same_bits(stats[4 * lv:4 * lv + 3], [w1, w0, wd]), (lv, stats, w1, w0, wd)
        raw, z, rays, _ = batches[lv]
        d_raw = ops.composite_backward_closs(raw, z, rays, None, False, L, fw[lv][0], fw[lv][4], fin.stats[4 * lv:4 * lv + 4],
                                             torch.ones(1, device=dev), None, level=lv)
        row[f"K/bound d_raw level {lv}"] = check_d_raw(dev, f"tail hardmask B={B} level {lv}", d_raw, raw, z, rays, ref["d_rgb"], ref["d_depth"])
    assert abs(terms[0] - total) <= bsum + R.gamma(2 * levels) * total          # the terms' own bounds + the loss's 2 additions per level
    if levels == 1:
        assert not terms[4:7].any()
    print(f"tail hardmask B={B} levels={levels}: {row}")
    assert inside(row), row
    _record("tail_hardmask", f"B{B}-levels{levels}", row)


@pytest.mark.parametrize("rf,df", [("hardmask", "norm"), ("hardmask", "plain"), ("hardmask", "hardmask_coef"), ("softlp", "softlp"),
                                   ("softmask", "softmask"), ("softlp", "hardmask")])
@pytest.mark.parametrize("B", [9, 8200], ids=_tail_id)
def test_folded_tail_lossform_finish(dev, B, rf, df):
    """cnerf_lossform_finish (closs_tail_k<true>: ten partial sums per workgroup) once per form, with the bounds of
    test_lossform_kernels_vs_float64_lines: terms 1e-6 relative, temperature gradients 1e-5, d_raw 2e-6 of its largest element."""
    from consistentnerf_amd import ops
    from test_gpu_lossforms import lines64
    raw, z, rays, d = tail_batch(dev, B)
    tgt, prior, mask = T(d["tgt"], dev), T(d["prior"], dev), T(d["mask"], dev)
    temps = (torch.tensor([0.40318605], device=dev), torch.tensor([0.3], device=dev))
    L = ops.ClossSpec(tgt, mask, prior, R.FAR, 0.2, 1.0, 0.1, 0.0, rgb_form=ops.RGB_FORMS.index(rf), depth_form=ops.DEPTH_FORMS.index(df),
                      lp_coef=0.5, temps=temps + temps).checked(B)
    rgb, _disp, _acc, _w, depth, ws = ops.composite_forward_closs(raw, z, rays, None, False, L)
    assert ws.numel() == 10 * ((B + 7) // 8)
    terms, stats, _pd, _sd, d_temp = ops.lossform_finish(L, B, ws, None, depth, None, rgb, None)
    g_temp = torch.zeros(2, device=dev)
    d_raw = ops.composite_backward_closs(raw, z, rays, None, False, L, rgb, depth, stats[0:8], torch.ones(1, device=dev), None, None, level=0,
                                         d_temp2=d_temp[0:2], g_temp2=g_temp)
    il, dl, g_rgb, g_dep, dt_r, dt_d = lines64(rgb, depth, tgt, prior, mask, rf, df, temps)
    t = N(terms)
    row = {}
    put(row, "K/bound img", float(t[1]), float(il), 1e-6 * abs(float(il)))
    put(row, "K/bound depth", float(t[2]), float(dl), 1e-6 * abs(float(dl)))
    if rf == "softmask":
        put(row, "K/bound d_temp rgb", float(g_temp[0]), float(dt_r), 1e-5 * abs(float(dt_r)))
    if df == "softmask":
        put(row, "K/bound d_temp depth", float(g_temp[1]), 0.1 * float(dt_d), 1e-6 * abs(float(dt_d)))
    assert (float(g_temp[0]) != 0) == (rf == "softmask") and (float(g_temp[1]) != 0) == (df == "softmask")
    row["K/bound d_raw"] = check_d_raw(dev, f"tail {rf}/{df} B={B}", d_raw, raw, z, rays, N(g_rgb), N(0.1 * g_dep))
    print(f"tail forms B={B} {rf}/{df}: {row}")
    assert inside(row), row
    _record("tail_forms", f"B{B}-{rf}-{df}", row)


def _mean3(e, sel):
    return float(e[sel].sum() / (3.0 * sel.sum()))


@pytest.mark.parametrize("coins", [(1, 1, 1, 1), (0, 1, 1, 0)], ids=lambda c: "coins" + "".join(map(str, c)))
@pytest.mark.parametrize("B", [9, 8200], ids=_tail_id)
def test_folded_tail_coin_form(dev, B, coins):
    """cnerf_closs_finish_ss (VT:941-969), two levels: each term over the selected rays or, coin 0, its other branch (the coarse colour
    term falls back to the FINE colours; a depth term to 0).  Colour means 6 u, depth means the masked depth bound; the seed weights
    are the stand-alone kernel's for the selection (coin 1) or for all rays (coin 0), bit for bit."""
    from consistentnerf_amd import ops
    batches = [tail_batch(dev, B, seed=lv) for lv in range(2)]
    d = batches[0][3]
    sel, ones = d["mask"] == 1, np.ones(B, bool)
    L = ops.ClossSpec(T(d["tgt"], dev), T(d["mask"], dev), T(d["prior"], dev), R.FAR, R.COEF, 1.0, 1.0, 0.0, ss_coins=coins).checked(B)
    fw = [ops.composite_forward_closs(raw, z, rays, None, False, L, level=lv) for lv, (raw, z, rays, _d) in enumerate(batches)]
    fin = ops.closs_finish(L, B, fw[0][5], fw[1][5], fw[0][4], fw[1][4])
    terms, stats = N(fin.terms), N(fin.stats)
    e = [((N(f[0]).astype(np.float64) - d["tgt"]) ** 2).sum(1) for f in fw]
    kws = [dict(rgb=N(f[0]), tgt=d["tgt"], depth=N(f[4]), prior=d["prior"], mask=d["mask"], far=R.FAR, coef=R.COEF, counts=None, g_scale=1.0)
           for f in fw]
    dep = [(R.masked64(**k)["dep"], R.masked_bounds(**k)["dep"]) for k in kws]
    want = {1: _mean3(e[0], sel if coins[0] else ones), 2: dep[0][0] if coins[1] else 0.0,
            4: _mean3(e[1], sel) if coins[2] else _mean3(e[0], ones), 5: dep[1][0] if coins[3] else 0.0}
    bound = {1: R.gamma(6) * want[1], 2: dep[0][1] if coins[1] else 0.0, 4: R.gamma(6) * want[4], 5: dep[1][1] if coins[3] else 0.0}
    row = {}
    for k in want:
        put(row, f"K/bound terms[{k}]", terms[k], want[k], bound[k])
    assert abs(terms[0] - sum(want.values())) <= sum(bound.values()) + R.gamma(4) * sum(want.values())      # + the loss's additions
    wsel, _w0, wd = standalone_weights(dev, d["mask"])
    wall, _, _ = standalone_weights(dev, np.ones(B, np.float32))
    zero = np.float32(0)
    w1 = (wsel if coins[0] else wall) + (zero if coins[2] else wall)
    w0 = (zero if coins[0] else wall) + (zero if coins[2] else wall)
    assert same_bits(stats[0:4], [w1, w0, wd if coins[1] else zero, zero]), stats
    assert same_bits(stats[4:8], [wsel if coins[2] else zero, zero, wd if coins[3] else zero, zero]), stats
    print(f"tail coins {coins} B={B}: {row}")
    assert inside(row), row
    _record("tail_coins", f"B{B}-{''.join(map(str, coins))}", row)


@pytest.mark.parametrize("seg", [8, 8192, 16392 - 8], ids=lambda s: f"seg_row{s}")
def test_folded_tail_one_render_form_second_pass(dev, seg):
    """cnerf_closs_finish_ss2 at B = 16392 (2049 partials): rays [0, seg_row) the primary batch, the rest the second render's warped rays
    (mask 1 = live, 0 = padding).  The per-segment sums take a second pass of the loop in at least one segment at every seg_row.  Terms
    against the float64 lines per segment; the seed weights of both segments the stand-alone kernel's on each segment's mask."""
    from consistentnerf_amd import ops
    B = 16392
    raw, z, rays, d = tail_batch(dev, B)
    L = ops.ClossSpec(T(d["tgt"], dev), T(d["mask"], dev), T(d["prior"], dev), R.FAR, R.COEF, 1.0, 1.0, 0.0, ss_coins=(1, 1, 1, 1),
                      seg_row=seg).checked(B)
    rgb, _disp, _acc, _w, depth, ws = ops.composite_forward_closs(raw, z, rays, None, False, L)
    fin = ops.closs_finish(L, B, ws, None, depth, None)
    terms, stats = N(fin.terms), N(fin.stats)
    row = {}
    for name, sl, ti in (("primary", slice(0, seg), (1, 2)), ("warped", slice(seg, B), (8, 9))):
        kw = dict(rgb=N(rgb)[sl], tgt=d["tgt"][sl], depth=N(depth)[sl], prior=d["prior"][sl], mask=d["mask"][sl], far=R.FAR, coef=R.COEF,
                  counts=None, g_scale=1.0)
        ref, bnd = R.masked64(**kw), R.masked_bounds(**kw)
        s1 = kw["mask"] == 1
        img = _mean3(((kw["rgb"].astype(np.float64) - kw["tgt"]) ** 2).sum(1), s1)          # over the selected / live rays alone
        put(row, f"K/bound img {name}", terms[ti[0]], img, R.gamma(6) * img)
        put(row, f"K/bound dep {name}", terms[ti[1]], ref["dep"], bnd["dep"])
        w1, _w0, wd = standalone_weights(dev, kw["mask"])
        st = stats[0:4] if name == "primary" else stats[4:8]
        assert same_bits(st, [w1, np.float32(0), wd, np.float32(0)]), (name, st, w1, wd)
    assert terms[7] == float((d["mask"][seg:] == 1).sum())
    print(f"tail one-render seg_row={seg}: {row}")
    assert inside(row), row
    _record("tail_one_render", f"seg_row{seg}", row)


@pytest.mark.parametrize("B,P,n", [(8200, 8, 100), (8193, 2, 37)], ids=lambda v: str(v))
def test_folded_tail_patch_term_rides(dev, B, P, n):
    """The depth-patch term inside closs_tail_k (waves [0, P) of the tail) on the forward's own depth map: value and patch_d within
    4 A + floor of the oracle, next to the hardmask terms."""
    from consistentnerf_amd import ops
    raw, z, rays, d = tail_batch(dev, B)
    _depth, mono = R.patch_inputs(P, n, "mild")
    L = ops.ClossSpec(T(d["tgt"], dev), T(d["mask"], dev), T(d["prior"], dev), R.FAR, R.COEF, 1.0, 1.0, 1.0, mono=T(mono, dev), P=P, n=n).checked(B)
    rgb, _disp, _acc, _w, depth, ws = ops.composite_forward_closs(raw, z, rays, None, False, L)
    fin = ops.closs_finish(L, B, ws, None, depth, None)
    terms = N(fin.terms)
    row = check_patch(f"tail patch P{P} n{n}", float(terms[3]), N(fin.patch_d)[0].astype(np.float64), N(depth)[:P * n], mono, P, n)
    kw = dict(rgb=N(rgb), tgt=d["tgt"], depth=N(depth), prior=d["prior"], mask=d["mask"], far=R.FAR, coef=R.COEF, counts=None, g_scale=1.0)
    ref, bnd = R.masked64(**kw), R.masked_bounds(**kw)
    put(row, "K/bound img", terms[1], ref["img"], bnd["img"])
    put(row, "K/bound dep", terms[2], ref["dep"], bnd["dep"])
    print(f"tail patch B={B} P={P} n={n}: {row}")
    assert row["K/bound img"] <= 1.0 and row["K/bound dep"] <= 1.0
    _record("tail_patch", f"B{B}-P{P}-n{n}", row)


# ================================================================================================ Adam
def adam_run(dev, n, clip, gs, step, entry):
    """One step on NaN-guarded device buffers through cnerf_adam_step or cnerf_adam_hyper + cnerf_adam_step_dev -> (p, m, v) numpy."""
    from consistentnerf_amd import _lib
    lib = _lib.load()
    p, g, m, v = R.adam_inputs(n, clip, gs)
    bufs = []
    for a in (p, g, m, v):
        t = torch.full((n + GUARD,), float("nan"), device=dev)
        t[:n] = T(a, dev)
        bufs.append(t)
    lr = R.adam_lr(step)
    if entry == "adam_k":
        _lib.check(lib.cnerf_adam_step(*map(_p, bufs), n, step, lr, 0.9, 0.999, 1e-8, float(clip), float(gs), _stream()), "cnerf_adam_step")
    else:
        hyp = torch.empty(8)
        _lib.check(lib.cnerf_adam_hyper(step, lr, 0.9, 0.999, 1e-8, float(clip), float(gs), C.c_void_p(hyp.data_ptr())), "cnerf_adam_hyper")
        assert same_bits(hyp.numpy(), list(R.adam_scalars32(step, lr)) + [np.float32(clip), np.float32(gs)]), hyp
        hd = hyp.to(dev)
        _lib.check(lib.cnerf_adam_step_dev(*map(_p, bufs), n, _p(hd), _stream()), "cnerf_adam_step_dev")
    out = [N(t) for t in bufs]
    for name, o in zip("pgmv", out):
        assert np.isnan(o[n:]).all(), f"a write past the end of {name}"
    assert same_bits(out[1][:n], g), "the gradient buffer was written"
    return (p, g, m, v), (out[0][:n], out[2][:n], out[3][:n])


def _adam_id(c):
    n, clip, gs, step = c
    return f"n{n}-clip{clip}-gs{gs}-step{step}" + ("-grid-stride-second-pass" if n > R.ADAM_SWEEP else "")


@pytest.mark.parametrize("case", R.adam_cases(), ids=_adam_id)
def test_adam_k_and_adam_dev_k_bit_for_bit(dev, case):
    """adam_k against the numpy float32 restatement BIT FOR BIT (every operation of the kernel is one correctly rounded IEEE operation:
    -ffp-contract=off, no fast-math, HIP's correctly rounded division and square root), adam_dev_k the same bits from
    cnerf_adam_hyper's eight floats (which equal the restatement's float-rounded scalars exactly), and both per element inside the
    derived bound of the float64 step wherever the fp32 results are finite.  NaN gradients give NaN p, m, v with and without the clip;
    +-inf clip to +-clip."""
    n, clip, gs, step = case
    clip = R.f32(clip)
    (p, g, m, v), got = adam_run(dev, n, clip, gs, step, "adam_k")
    want = R.adam32(p, g, m, v, step, R.adam_lr(step), clip, gs)
    row = {}
    for name, a, b in zip("pmv", got, want):
        diff = ~(np.isnan(a) & np.isnan(b)) & (bits(a) != bits(b))
        row[f"elements not bit-equal {name}"] = int(diff.sum())
        if diff.any():
            i = int(np.flatnonzero(diff)[0])
            print(f"adam {case} {name}[{i}]: kernel {a[i]!r} restatement {b[i]!r}; p {p[i]!r} g {g[i]!r} m {m[i]!r} v {v[i]!r}")
        assert np.array_equal(np.isnan(a), np.isnan(b)), (name, "NaN pattern")
        assert not diff.any(), (name, int(diff.sum()))
    nan_g = np.isnan(g)
    for a in got:
        assert np.isnan(a[nan_g]).all(), "a NaN gradient must give NaN p, m, v (torch.clamp keeps NaN)"
    if clip > 0:
        inf_g = np.isinf(g)
        assert np.isfinite(got[0][inf_g]).all() and np.isfinite(got[1][inf_g]).all() and np.isfinite(got[2][inf_g]).all()
    _inputs, got_dev = adam_run(dev, n, clip, gs, step, "adam_dev_k")
    for name, a, b in zip("pmv", got_dev, got):
        assert same_bits(a, b), f"adam_dev_k differs from adam_k in {name}"
    ref, bnd = R.adam64(p, g, m, v, step, R.adam_lr(step), clip, gs)
    fin = np.isfinite(got[0]) & np.isfinite(got[1]) & np.isfinite(got[2])
    assert fin.sum() >= n - 16
    for name, a, b, c in zip("pmv", got, ref, bnd):
        put(row, f"K/bound {name}", a[fin], b[fin], c[fin])
    print(f"adam {_adam_id(case)}: {row}")
    assert all(row[f"K/bound {k}"] <= 1.0 for k in "pmv"), row
    _record("adam", _adam_id(case), row)


@pytest.mark.parametrize("clip", [0.0, 0.1], ids=lambda c: f"clip{c}")
def test_adam_nan_gradient_stays_nan(dev, clip):
    """clip_grad_value_ is clamp_(-clip, clip), which keeps NaN: a NaN gradient turns p, m and v to NaN with and without the clip,
    in adam_k and adam_dev_k, and +-inf clips to +-clip (the update of an element whose gradient sits at the clip)."""
    from consistentnerf_amd import ops
    g = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.1, -0.1, 0.02], device=dev)
    outs = []
    for entry in ("adam_k", "adam_dev_k"):
        p, m, v = (torch.full((6,), x, device=dev) for x in (1.0, 0.01, 1e-4))
        if entry == "adam_k":
            ops.adam_step(p, g, m, v, 4, 5e-4, clip=clip)
        else:
            hyp = torch.empty(8)
            ops.adam_hyper(hyp, 4, 5e-4, clip=clip)
            ops.adam_step_dev(p, g, m, v, hyp.to(dev))
        outs.append((N(p), N(m), N(v)))
        for t in outs[-1]:
            assert np.isnan(t[0]), (entry, clip, t)
            assert np.isfinite(t[3:]).all()
        if clip > 0:
            for t in outs[-1]:
                assert t[1] == t[3] and t[2] == t[4], (entry, "+-inf clips to +-clip", t)
    for a, b in zip(*outs):
        assert same_bits(a, b)
