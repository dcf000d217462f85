"""The cross-view warp, the hard-mask precompute and the positional encoding over their input range (run on the MI355X:
`pytest -m gpu`).  A wrong mask bit changes no shape and raises no error: it changes which rays every later step trusts.

  hard masks   hard_mask_k (warp.hip) against oracle.hard_masks bit for bit, per-chunk thresholds equal as fp32 (NaN where the
               oracle has NaN), on three scenes (24 x 32, 37 x 53, 48 x 64; fx != fy, off-centre principal point, one view 75
               degrees round, one held out) x chunk in {1, 7, 255, 256, 257, 1000, HW - 1, HW, HW + 5, 5120} x thr0 in
               {0.1, 1e-6}, a thr0 that stops every chunk at level 0 and one that needs more than 64 doublings.  The inputs are
               conditioned (_inputs.condition_hard_mask_inputs): no pixel sits on a rounding tie, the border or a ladder rung, so
               the oracle alone decides them (tests/test_geometry_inputs.py proves that on the CPU, in float64).  What conditioning
               removes is tested on purpose-built inputs instead: |z - D_ref| EXACTLY on a rung (the comparison is strict), pixels
               EXACTLY on a tie (half to even) and on the border (strict).
               Properties: the OR into a pre-filled mask, untouched slices, the thr_out == nullptr path, a second launch, pairs.
               Non-finite priors: the reference loops forever there; defined behaviour (geometry envelope): a pixel with a NaN / inf
               |z - D_ref| never passes, a chunk with no other in-bounds pixel is a chunk without one.
  warp         warp_points_k at N in {0, 1, 255, 256, 257, 100003}, both flips: Xc within 4 u (|X||r0| + |Y||r1| + |Z||r2| + |t|)
               of float64 (four rounded terms, no contraction), the pixel and the in-bounds flag exact against float64 and the
               oracle on the rows two fp32 evaluations cannot round differently; behind the camera, z_cam == 0, fp32 overflow, NaN
               and inf coordinates field by field against the oracle; every optional output null.
  encoding     embed_k against float64 sin / cos of the exact argument at coordinate scales 1e-3 ... 1e5, L in {10, 4, 1}; the
               reference's own fp32 error (3.6e-8 at every scale) is the yardstick.  The fused kernels (encode.hpp) must see the
               same values: the fp32 forward on points == the same network on ops.embed's rows, bit for bit.

Measured figures go to $CNERF_RECORD_DIR/geometry_envelope.json when that variable names a directory;
profiles/geometry_envelope.json is the copy of the MI355X run this file was written against.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _inputs as I
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

torch.set_num_threads(4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from consistentnerf_amd import ops
    ok, name, cus, lds = ops.device_info(0)
    print(f"device: {name} CUs={cus} LDS/CU={lds}")
    assert ok, f"not a gfx950 device: {name}"
    return torch.device("cuda:0")


def T(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


RECORD = {}


def _record(section, key, row):
    RECORD.setdefault(section, {})[key] = row
    out_dir = os.environ.get("CNERF_RECORD_DIR")
    if not out_dir:
        return
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "geometry_envelope.json"), "w") as f:
        json.dump({"bounds": {"warp_Xc": "4 * 2^-24 * (|X||r0| + |Y||r1| + |Z||r2| + |t|) per component", "embed": EMBED_BOUND,
                              "embed_cap": EMBED_CAP, "nudged_share": 0.02, "dropped_share": 0.02, "conditioning_iterations": 8},
                   "cases": RECORD}, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ 1. hard masks
def _w2c(pose):
    c2w = torch.eye(4)
    c2w[:3, :4] = torch.from_numpy(np.ascontiguousarray(pose[:3, :4]))
    return torch.inverse(c2w).numpy()          # the 4x4 fp32 host inverse, as V:1008-1010 and compute_hard_masks


def _pair(dev, c, t, r, thr0, chunk, mask=None, want_thr=True, depth_ref=None):
    """ops.hard_mask_pair of views (t, r) of case c -> (mask uint8 [HW] numpy, thr fp32 numpy | None)."""
    from consistentnerf_amd import ops
    H, W = c["H"], c["W"]
    m = torch.zeros(H * W, dtype=torch.uint8, device=dev) if mask is None else mask
    dr = c["depths"][r] if depth_ref is None else depth_ref
    thr = ops.hard_mask_pair(H, W, c["K"], c["poses"][t], _w2c(c["poses"][r]), T(c["depths"][t], dev).reshape(-1),
                             T(dr, dev).reshape(-1), thr0, chunk, m, want_thr=want_thr)
    return m.cpu().numpy(), None if thr is None else thr.cpu().numpy()


def _same_thr(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


_ORACLE = {}


def _oracle(scene, i_train, chunk, thr0):
    """oracle.hard_masks on the conditioned scene, computed once per case -> (masks, {(t, r): thresholds})."""
    key = (scene, tuple(i_train), chunk, thr0)
    if key not in _ORACLE:
        c = I.geometry_case(scene)
        masks, log = O.hard_masks(c["H"], c["W"], c["K"], c["poses"], c["depths"], list(i_train), float(np.float32(thr0)), chunk)
        thr = {}
        for t, r, ch, th in log:
            thr.setdefault((int(t), int(r)), []).append(th)
        _ORACLE[key] = (masks, {k: np.array(v, np.float64).astype(np.float32) for k, v in thr.items()})
    return _ORACLE[key]


@pytest.mark.parametrize("scene,i_train,chunk,thr0", I.hard_mask_cases())
def test_hard_masks_vs_oracle(dev, scene, i_train, chunk, thr0):
    """compute_hard_masks and, pair by pair, ops.hard_mask_pair on a fresh mask against oracle.hard_masks: every bit, every
    per-chunk threshold, every NaN; the held-out view stays zero."""
    from consistentnerf_amd import run_nerf_view as V
    c = I.geometry_case(scene)
    H, W = c["H"], c["W"]
    want, want_thr = _oracle(scene, i_train, chunk, thr0)
    masks, thr = V.compute_hard_masks(H, W, c["K"], c["poses"], c["depths"], list(i_train), thr0, chunk, device=dev,
                                      return_thresholds=True)
    diff = masks != want
    n_nan = sum(int(np.isnan(v).sum()) for v in want_thr.values())
    deepest = max(int(np.log2(v[~np.isnan(v)].max() / np.float32(thr0)) + 0.5) for v in want_thr.values() if not np.isnan(v).all())
    print(f"  {H}x{W} chunk={chunk} thr0={thr0:g}: {int(diff.sum())} of {diff.size} mask bits differ; {n_nan} chunks without an "
          f"in-bounds pixel; deepest level {deepest}")
    assert diff.sum() == 0, "hard masks must match the oracle bit for bit"
    assert set(thr) == set(want_thr)
    for k in want_thr:
        assert _same_thr(thr[k], want_thr[k]), (k, thr[k], want_thr[k])
    assert not masks[3].any() and all(not masks[v].any() for v in range(4) if v not in i_train)
    if thr0 == I.GEOMETRY_THR0[2]:
        assert deepest == 0
    if thr0 == I.GEOMETRY_THR0[3]:
        assert 64 < deepest < I.KMAX
    for t in i_train:
        acc = np.zeros(H * W, np.uint8)
        for r in i_train:
            if r != t:
                m, th = _pair(dev, c, t, r, thr0, chunk)
                assert set(np.unique(m)) <= {0, 1} and _same_thr(th, want_thr[(t, r)])
                acc |= m
        assert np.array_equal(acc.astype(bool).reshape(H, W), want[t]), f"OR of the single-pair masks of view {t}"


@pytest.mark.parametrize("chunk", [7, 257])
@pytest.mark.parametrize("scene", range(len(I.GEOMETRY_SCENES)))
def test_hard_mask_properties(dev, scene, chunk):
    """A pre-filled mask keeps every bit that was set and gains exactly the bits a fresh mask gets (the OR over reference views);
    a chunk without an in-bounds pixel leaves its slice untouched; thr_out == nullptr gives the same mask; a second launch
    gives the same bits; the mask of (t, r1, r2) is the OR of the two single-pair masks."""
    c = I.geometry_case(scene)
    H, W = c["H"], c["W"]
    rs = np.random.RandomState(scene * 1000 + chunk)
    touched_nothing = 0
    for t, r1, r2 in ((0, 1, 2), (2, 0, 1)):
        fresh, thr = _pair(dev, c, t, r1, 0.1, chunk)
        pre = (rs.randint(0, 256, size=H * W) * (rs.uniform(size=H * W) < 0.5)).astype(np.uint8)      # any bit pattern, half zero
        got, thr_b = _pair(dev, c, t, r1, 0.1, chunk, mask=T(pre.copy(), dev))
        assert np.array_equal(got, np.where(fresh == 1, 1, pre).astype(np.uint8)), "set bytes become 1, the rest is kept"
        assert np.all(got[pre != 0] != 0) and _same_thr(thr, thr_b)
        dead = np.isnan(thr).repeat(chunk)[:H * W]
        assert (dead.any() or chunk > 7) and np.array_equal(got[dead], pre[dead]) and not fresh[dead].any()
        touched_nothing += int(np.isnan(thr).sum())
        live = ~np.isnan(thr)
        counts = np.add.reduceat(fresh.astype(np.int64), np.arange(0, H * W, chunk))
        assert np.all(counts[live] >= 1) and np.all(counts[~live] == 0), "a live chunk sets at least one pixel, a dead one none"
        no_thr, none = _pair(dev, c, t, r1, 0.1, chunk, want_thr=False)
        assert none is None and np.array_equal(no_thr, fresh)
        again = T(fresh.copy(), dev)
        twice, _ = _pair(dev, c, t, r1, 0.1, chunk, mask=again)
        assert np.array_equal(twice, fresh)
        other, _ = _pair(dev, c, t, r2, 0.1, chunk)
        both = torch.zeros(H * W, dtype=torch.uint8, device=dev)
        _pair(dev, c, t, r1, 0.1, chunk, mask=both)
        both_np, _ = _pair(dev, c, t, r2, 0.1, chunk, mask=both)
        assert np.array_equal(both_np, fresh | other)
    print(f"  {H}x{W} chunk={chunk}: {touched_nothing} chunks without an in-bounds pixel left untouched")
    _record("conditioning", f"{H}x{W}", dict(c["info"], pixels_per_view=H * W))


@pytest.mark.parametrize("scene", [0, 2])
def test_hard_mask_threshold_is_strict(dev, scene):
    """|z - D_ref| EXACTLY on a rung does not pass it (`<`, V:1024).  A reference prior of thr0 * 2^40 ~ 1.1e11 absorbs z_cam (its
    ulp is 8192), so the fp32 difference IS that rung, in the kernel as in the oracle: the pixel passes at level 41.  Rows whose
    prior is the fp32 neighbour below pass at level 40: in a chunk that holds both, only those are set."""
    c = I.geometry_case(scene)
    H, W = c["H"], c["W"]
    rung = np.float32(I.ladder(0.1)[40])
    below = np.nextafter(rung, np.float32(0))
    depths = c["depths"].copy()
    depths[1] = rung
    depths[1, ::3] = below
    chunk = 2 * W + 3
    want, log = O.hard_masks(H, W, c["K"], c["poses"], depths, [0, 1], float(np.float32(0.1)), chunk)
    want_thr = np.array([th for t, r, ch, th in log if (t, r) == (0, 1)], np.float64).astype(np.float32)
    got, thr = _pair(dev, c, 0, 1, 0.1, chunk, depth_ref=depths[1])
    levels = np.round(np.log2(want_thr / np.float32(0.1)))                     # NaN: no in-bounds pixel
    assert set(levels[~np.isnan(levels)].astype(int).tolist()) <= {40, 41} and (levels == 40).any()
    q = I.hard_mask_pair_f64(H, W, c["K"], c["poses"][0], c["poses"][1], c["depths"][0], c["depths"][1], 0.1)
    on_rung = q["inb"] & (np.rint(q["py"]) % 3 != 0) & (levels.repeat(chunk)[:H * W] == 40)
    assert on_rung.sum() > 10 and not want[0].reshape(-1)[on_rung].any(), "the oracle leaves a pixel ON the rung out"
    assert np.array_equal(got.astype(bool).reshape(H, W), want[0]) and _same_thr(thr, want_thr)
    # every row on the rung: level 41 everywhere
    depths[1] = rung
    want, log = O.hard_masks(H, W, c["K"], c["poses"], depths, [0, 1], float(np.float32(0.1)), chunk)
    want_thr = np.array([th for t, r, ch, th in log if (t, r) == (0, 1)], np.float64).astype(np.float32)
    assert np.all(want_thr[~np.isnan(want_thr)] == np.float32(I.ladder(0.1)[41]))
    got, thr = _pair(dev, c, 0, 1, 0.1, chunk, depth_ref=depths[1])
    assert np.array_equal(got.astype(bool).reshape(H, W), want[0]) and _same_thr(thr, want_thr)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("scene", [0, 1])
def test_hard_mask_non_finite_prior(dev, scene, bad):
    """Whole rows of the reference prior are NaN / inf.  The oracle would loop; the expected result is the float64 restatement's,
    in which a non-finite |z - D_ref| has no level: a chunk whose in-bounds pixels all land on such rows is left untouched and
    reports NaN, a chunk with some finite differences takes its threshold from those and leaves the others 0."""
    c = I.geometry_case(scene)
    H, W = c["H"], c["W"]
    dref = c["depths"][1].copy()
    dref[H // 3:2 * H // 3] = bad
    chunk = W + 1
    for thr0 in (0.1, 1e-6):
        q = I.hard_mask_pair_f64(H, W, c["K"], c["poses"][0], c["poses"][1], c["depths"][0], dref, thr0)
        km = I.chunk_levels(q["level"], chunk)
        starts = np.arange(0, H * W, chunk)
        n_inb = np.add.reduceat(q["inb"].astype(np.int64), starts)
        n_fin = np.add.reduceat((q["level"] < I.NO_LEVEL).astype(np.int64), starts)
        all_bad, mixed = (n_inb > 0) & (n_fin == 0), (n_fin > 0) & (n_fin < n_inb)
        assert all_bad.sum() >= 2 and mixed.sum() >= 2, "the case must hold both kinds of chunk"
        live = km < I.NO_LEVEL
        want = (live.repeat(chunk)[:H * W] & (q["level"] == km.repeat(chunk)[:H * W])).astype(np.uint8)
        want_thr = np.where(live, I.ladder(thr0).astype(np.float32)[np.minimum(km, I.KMAX)], np.float32(np.nan))
        pre = np.full(H * W, 2, np.uint8)
        got, thr = _pair(dev, c, 0, 1, thr0, chunk, mask=T(pre.copy(), dev), depth_ref=dref)
        wrong = got != np.where(want == 1, 1, pre)
        print(f"  {H}x{W} {bad} thr0={thr0:g}: {int(all_bad.sum())} chunks all non-finite, {int(mixed.sum())} mixed; "
              f"{int(wrong.sum())} wrong mask bytes; thresholds of the all-non-finite chunks: {thr[all_bad][:4]}")
        assert np.isnan(thr[all_bad]).all(), "a chunk with only non-finite differences reports NaN"
        assert not wrong.any(), f"{int(wrong.sum())} mask bytes differ"
        assert _same_thr(thr, want_thr)
        bad_px = q["inb"] & (q["level"] == I.NO_LEVEL)
        assert bad_px.any() and np.all(got[bad_px] == 2), "a pixel with a non-finite difference is never set"


def test_hard_mask_pair_validates(dev):
    from consistentnerf_amd import ops
    from consistentnerf_amd._lib import CnerfError
    c = I.geometry_case(0)
    H, W = c["H"], c["W"]
    d = T(c["depths"][0], dev).reshape(-1)
    w2c = _w2c(c["poses"][1])

    def call(dt=d, dr=d, mask=None, chunk=256):
        mask = torch.zeros(H * W, dtype=torch.uint8, device=dev) if mask is None else mask
        return ops.hard_mask_pair(H, W, c["K"], c["poses"][0], w2c, dt, dr, 0.1, chunk, mask)

    call()
    for kw in (dict(dt=d[:-1]), dict(dr=d[:-1]), dict(dt=torch.cat([d, d])), dict(mask=torch.zeros(H * W - 1, dtype=torch.uint8, device=dev)),
               dict(mask=torch.zeros(H * W + 1, dtype=torch.uint8, device=dev)), dict(mask=torch.zeros(H * W, dtype=torch.bool, device=dev)),
               dict(mask=torch.zeros(H * W, dtype=torch.float32, device=dev)), dict(mask=torch.zeros(H * W, dtype=torch.uint8)),
               dict(mask=torch.zeros(2 * H * W, dtype=torch.uint8, device=dev)[::2]), dict(chunk=0), dict(chunk=-5)):
        with pytest.raises(CnerfError, match="hard_mask_pair"):
            call(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. warp_points_k
@pytest.mark.parametrize("flip", [True, False])
def test_warp_points_envelope(dev, flip):
    from consistentnerf_amd import ops
    c = I.geometry_case(2)
    H, W, K = c["H"], c["W"], c["K"]
    P, pose = I.warp_envelope_points(c)
    w2c = _w2c(pose)
    p, keep = I.warp_decided_rows(P, w2c, K, H, W, flip)
    o_Xc, o_x, o_y, o_inb = (a.numpy() for a in O.warp_points(T(P), T(w2c), T(K), H, W, flip))
    dropped = 1.0 - keep.mean()
    assert dropped <= 0.02
    bound = 4 * I.U32 * p["S"]
    worst = 0.0
    for N in I.WARP_N:
        Xc, px, py, inb = (a.cpu().numpy() for a in ops.warp_points(T(P[:N], dev), w2c, K, H, W, flip))
        assert Xc.shape == (N, 3) and px.shape == py.shape == inb.shape == (N,)
        if N == 0:
            continue
        ratio = float((np.abs(Xc.astype(np.float64) - p["Xc"][:N]) / bound[:N]).max())
        worst = max(worst, ratio)
        k = keep[:N]
        print(f"  flip={flip} N={N}: Xc error / bound {ratio:.3f}; {int((~k).sum())} rows dropped; in bounds {int(inb[k].sum())}")
        assert ratio <= 1.0, "Xc beyond four roundings of its terms"
        for name, got, f64, orc in (("px", px, p["x"], o_x), ("py", py, p["y"], o_y), ("inb", inb, p["inb"], o_inb)):
            assert np.array_equal(got[k], f64[:N][k]), f"{name} vs float64"
            assert np.array_equal(got[k], orc[:N][k]), f"{name} vs the oracle"
        assert not inb[~np.isfinite(px) | ~np.isfinite(py)].any()
    assert (p["inb"] & keep & (p["Xc"][:, 2] < 0)).sum() > 100, "points behind the camera that land in the image (no depth-sign test)"
    _record("warp", f"flip{int(flip)}", {"Xc_error_over_bound": worst, "dropped_share": float(dropped),
                                        "oracle_Xc_error_over_bound": float((np.abs(o_Xc.astype(np.float64) - p["Xc"]) / bound).max())})


def _special_rows():
    """w2c = [I | (1, -2, 3)] (exact arithmetic) and rows: 0 the camera centre (Xc == 0, z_cam exactly 0), 1-2 in the camera plane
    off the centre, 3-6 in front and behind, 7-9 a pixel beyond fp32, 10-18 NaN / +inf / -inf in each coordinate."""
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, 3] = (1, -2, 3)
    rows = [(-1, 2, -3), (4, 7, -3), (-6, 2, -3), (-0.75, 2.125, -1), (-0.75, 2.125, -5), (-1.1, 1.9, -2.5), (-1.1, 1.9, -3.5),
            (1e35, 2, -3 + 2.0 ** -20), (-1, -1e35, -3 - 2.0 ** -20), (3e38, 3e38, -3 + 2.0 ** -20)]
    for v in (np.nan, np.inf, -np.inf):
        rows += [(v, 2.5, -1), (-0.5, v, -1), (-0.5, 2.5, v)]
    return np.array(rows, np.float32), w2c


@pytest.mark.parametrize("flip", [True, False])
def test_warp_points_special_rows(dev, flip):
    """Field by field against the fp32 oracle, NaN pattern and the sign of every infinity included; inb false wherever the oracle's
    is.  With flip the reference multiplies by diag(1, -1, -1) where the kernel flips two signs, and on two kinds of row that is not
    the same thing (DESIGN.md 2 names both as defined differences): a row with a non-finite camera coordinate (inf * 0 = NaN
    spreads it to the other two; such rows' Xc is compared with the un-flipped oracle's, signs flipped) and a row with z_cam == 0
    off the centre (0 * 0 + 0 * 0 + (+0) * (-1) = +0 where the kernel has -0: the infinite pixel keeps its magnitude and changes
    sign).  Everything else, and everything without flip, is exact; inb never depends on either."""
    from consistentnerf_amd import ops
    c = I.geometry_case(2)
    H, W, K = c["H"], c["W"], c["K"]
    P, w2c_int = _special_rows()
    w2c_scene = _w2c(c["poses"][1])
    sign = np.array([1, -1, -1], np.float32)
    for tag, w2c, rows in (("integer", w2c_int, slice(None)), ("scene", w2c_scene, slice(10, None))):
        Pk = P[rows]
        Xc, px, py, inb = (a.cpu().numpy() for a in ops.warp_points(T(Pk, dev), w2c, K, H, W, flip))
        o_Xc, o_x, o_y, o_inb = (a.numpy() for a in O.warp_points(T(Pk), T(w2c), T(K), H, W, flip))
        plain = O.warp_points(T(Pk), T(w2c), T(K), H, W, False)[0].numpy()
        print(f"  {tag} flip={flip}\n   px {px}\n   oracle {o_x}\n   py {py}\n   oracle {o_y}\n   inb {inb.astype(int)} oracle {o_inb.astype(int)}")
        spread = flip & ~np.isfinite(plain).all(-1)               # inf * 0 in the reference's flip
        plane = flip & (plain[:, 2] == 0) & np.isfinite(plain).all(-1) & plain[:, :2].any(-1)
        assert np.array_equal(Xc[~spread], o_Xc[~spread], equal_nan=True), "Xc"
        assert np.array_equal(Xc[spread], (plain * sign)[spread], equal_nan=True), "Xc of a row with a non-finite coordinate"
        assert not np.isfinite(o_Xc[spread]).all(-1).any()
        for name, got, want in (("px", px, o_x), ("py", py, o_y)):
            assert np.array_equal(got[~plane], want[~plane], equal_nan=True), name
            assert np.array_equal(np.abs(got[plane]), np.abs(want[plane]), equal_nan=True), name + " in the camera plane"
        assert np.array_equal(inb, o_inb) and not inb[~o_inb].any()
        if tag == "integer":
            assert plane.sum() == (2 if flip else 0) and spread.sum() == (9 if flip else 0)
            assert not Xc[0].any() and np.isnan(px[0]) and np.isnan(py[0]) and not inb[0], "the camera centre: 0 / 0"
            assert np.isinf(px[1:3]).all() and np.isinf(px[7]) and np.isinf(py[8]) and not inb[[1, 2, 7, 8, 9]].any()
            zc = Xc[3:7, 2]
            assert (zc < 0).any() and (zc > 0).any() and inb[3:7].all(), "in front and behind: both land in the image"
        assert not inb[-9:].any() and np.isnan(px[-9:]).all() and np.isnan(py[-9:]).all()


@pytest.mark.parametrize("flip", [True, False])
def test_warp_points_ties_and_border(dev, flip):
    """What conditioning removes from the other tests, built exactly: with w2c = [I | t], z_cam = +-1 and dyadic intrinsics the
    projected pixel is exact in fp32.  A pixel at x.5 rounds half to EVEN (torch.round, V:607); a pixel that rounds to 0, W - 1,
    H - 1 is OUT of bounds, its neighbour inside is in (the bounds are strict, V:611-613); cx != cy."""
    from consistentnerf_amd import ops
    H, W = 24, 32
    K = np.array([[32.0, 0, 16.5], [0, 16.0, 10.25], [0, 0, 1]], np.float32)
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, 3] = (1, -2, 3)
    z = -1.0 if flip else 1.0                                     # camera z before the flip
    ys = -1.0 if flip else 1.0
    px = np.concatenate([np.arange(-1, W + 1) + 0.5, np.arange(-1, W + 1), np.arange(-1, W + 1) + 0.25]).astype(np.float64)
    py = np.concatenate([np.arange(-1, H + 1) + 0.5, np.arange(-1, H + 1) + 0.75]).astype(np.float64)
    gx, gy = (a.reshape(-1) for a in np.meshgrid(px, py, indexing="ij"))
    P = np.stack([(gx - 16.5) / 32.0 - 1, ys * (gy - 10.25) / 16.0 + 2, np.full_like(gx, z - 3)], -1).astype(np.float32)
    Xc, x, y, inb = (a.cpu().numpy() for a in ops.warp_points(T(P, dev), w2c, K, H, W, flip))
    o = [a.numpy() for a in O.warp_points(T(P), T(w2c), T(K), H, W, flip)]
    want_x, want_y = np.rint(gx), np.rint(gy)                      # numpy rounds half to even
    assert np.array_equal(o[1], want_x) and np.array_equal(o[2], want_y), "the construction is exact in the oracle's fp32"
    assert np.array_equal(x, want_x) and np.array_equal(y, want_y), "half to even"
    want_inb = (want_x > 0) & (want_x < W - 1) & (want_y > 0) & (want_y < H - 1)
    assert np.array_equal(inb, want_inb) and np.array_equal(inb, o[3]) and np.array_equal(Xc, o[0])
    assert (np.abs(gx - np.floor(gx) - 0.5) == 0).sum() > 0 and want_inb.any() and (~want_inb).any()


def test_warp_points_null_outputs(dev):
    """cnerf_warp_points with each optional output null writes the others as the full call does."""
    from consistentnerf_amd import _lib, ops
    c = I.geometry_case(2)
    H, W, K = c["H"], c["W"], c["K"]
    P, pose = I.warp_envelope_points(c)
    w2c = _w2c(pose)
    Pd = T(P[:257], dev)
    full = ops.warp_points(Pd, w2c, K, H, W, True)
    full = [full[0], full[1], full[2], full[3].to(torch.uint8)]
    lib = _lib.load()
    m = (C.c_float * 12)(*np.ascontiguousarray(w2c[:3, :4], np.float32).reshape(-1).tolist())
    for skip in range(5):
        bufs = [torch.full((257, 3), -7.0, device=dev), torch.full((257,), -7.0, device=dev), torch.full((257,), -7.0, device=dev),
                torch.full((257,), 9, device=dev, dtype=torch.uint8)]
        ptrs = [C.c_void_p(0) if i == skip else C.c_void_p(b.data_ptr()) for i, b in enumerate(bufs)]
        rc = lib.cnerf_warp_points(C.c_void_p(Pd.data_ptr()), 257, m, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]),
                                   H, W, 1, *ptrs, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        for i, (b, f) in enumerate(zip(bufs, full)):
            if i == skip:
                assert bool((b == (9 if i == 3 else -7.0)).all()), "a null output's stand-in buffer must stay untouched"
            else:
                assert torch.equal(b, f), f"output {i} with output {skip} null"


# ------------------------------------------------------------------------------------------------ 3. encoding range
# The reference's fp32 encoding is within 3.6e-8 of float64 at every scale here (test_geometry_inputs.py); embed_k measured
# EMBED_MEASURED at worst on the MI355X (7.13e-8 at L = 4, scale 1; 4.8e-8 ... 6.9e-8 elsewhere: no growth with the argument;
# profiles/geometry_envelope.json).  Asserted: four times the larger of the two.  The cap is
# what test_embed grants on [-4, 4]: a bound beyond it would mean the device sincosf degrades with the argument.
EMBED_ORACLE, EMBED_MEASURED, EMBED_CAP = 3.6e-8, 7.2e-8, 2e-6
EMBED_BOUND = 4 * max(EMBED_ORACLE, EMBED_MEASURED)
assert EMBED_BOUND <= EMBED_CAP


@pytest.mark.parametrize("L", [10, 4, 1])
def test_embed_range(dev, L):
    from consistentnerf_amd import ops
    for scale in I.EMBED_SCALES:
        x = I.embed_envelope_inputs(scale, L)
        ref = I.embed_f64(x, L)
        got = ops.embed(T(x, dev), L).cpu().numpy()
        assert got.shape == ref.shape
        assert np.array_equal(got[:, :3].view(np.uint32), x.view(np.uint32)), "the identity channels are copies (-0 and subnormals too)"
        e_k = float(np.abs(got.astype(np.float64) - ref).max())
        e_o = float(np.abs(O.embed(T(x), L).numpy().astype(np.float64) - ref).max())
        worst = np.unravel_index(np.abs(got.astype(np.float64) - ref).argmax(), ref.shape)
        print(f"  L={L} scale={scale:g}: kernel {e_k:.3e} (x = {x[worst[0], (worst[1] - 3) % 3]!r}, channel {worst[1]}), fp32 oracle "
              f"{e_o:.3e}, bound {EMBED_BOUND:.2e}")
        _record("embed", f"L{L}_scale{scale:g}", {"kernel": e_k, "fp32_oracle": e_o})
        assert e_o <= 4e-8, "the yardstick moved: the reference's own fp32 error"
        assert e_k <= EMBED_BOUND, f"embed_k is {e_k:.3e} from float64 at scale {scale:g} (bound {EMBED_BOUND:.2e})"


@pytest.mark.parametrize("vd", [True, False])
def test_fused_encoding_equals_embed(dev, vd):
    """The fp32 forward on points (encode.hpp inside mlp_fwd.hip) == the same network fed ops.embed's rows through the pre-embedded
    path, bit for bit, at every scale: both kernels hand the first layer the same encodings."""
    from consistentnerf_amd import ops
    from test_gpu_parity import make_model
    model, _ = make_model(2, 64, vd, 4, 5, dev)
    spec = model.spec()
    packed = ops.pack_weights(spec, [p.detach() for p in model.kernel_tensors()])
    rs = np.random.RandomState(12)
    for scale in I.EMBED_SCALES:
        pts = T(I.embed_envelope_inputs(scale, 10, n=300), dev)
        M = pts.shape[0]
        dirs = rs.normal(size=(M, 3)).astype(np.float32)
        dirs = T(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True), dev)
        xe = torch.cat([ops.embed(pts, 10)] + ([ops.embed(dirs, 4)] if vd else []), -1)
        raw_e, _ = ops.mlp_forward_embedded(spec, packed, xe)
        raw_p, _ = ops.mlp_forward(spec, packed, M, 1, pts=pts, dirs=dirs if vd else None)
        raw_p = raw_p.reshape(M, -1)
        assert torch.isfinite(raw_e).all()
        d = float((raw_p - raw_e).abs().max())
        print(f"  vd={vd} scale={scale:g}: max |points - embedded| = {d:.3e} of max |raw| {float(raw_e.abs().max()):.3e}")
        _record("fused", f"vd{int(vd)}_scale{scale:g}", {"max_abs_difference": d})
        assert torch.equal(raw_p, raw_e), f"the fused encoding differs from embed_k's at scale {scale:g}: {d:.3e}"
