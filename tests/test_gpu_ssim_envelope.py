"""The SSIM / MS-SSIM kernels of csrc/ssim.hip over their size range, against float64 (tests/_ssim_env_ref.py; its statements, bounds,
input families and mutants are checked without a GPU by tests/test_ssim_env_cpu.py):

  SSIM        ssim_tile_k<0/1> + ssim_fin_k + ssim_bwd_k: Ho x Wo over the forward tile's edges (8 x 64), W x H over the backward
              tile's (32 x 8), one or neither side filtered, windows 1 / 3 / 7 / 11 / 31, data_range 1 / 255, seven image families, 1 and
              6 planes with per-plane seeds 0, negative and 1e3: the means of S and cs inside the derived forward bound, EVERY element of
              dX and dY inside C_GRAD u A; planes independent bit for bit, dX alone = the pair's dX, seed 0 = gradient exactly 0
  MS-SSIM     cnerf_msssim_fwd / _bwd with an arbitrary seed per level and plane: every parity at every level, 1 ... 6 levels, a last
              level of one window, widths over 64 and 32; v per level, dX / dY with A accumulated through the levels, the pooled pyramid
  avg_pool2   sides 1 ... 65, 3 u; exact on small integers
  patch term  patch_ssim_k at P = 1 ... 16 (fp32 filter: its own count of roundings)
  buffers     every C entry point called on buffers of exactly the size the *_ws_floats queries (or the documented output sizes)
              give + a NaN guard band, all NaN-filled before the call: the guard stays NaN, no output element stays NaN
  limits      even / 0 / 33 windows and N C = 65536 raise and write nothing; NaN / inf pixels stay in their planes

Every measured fraction of a bound is printed; with CNERF_RECORD_DIR naming a directory they go to ssim_envelope.json there
(profiles/ssim_envelope.json is the MI355X run this file was written against).  Truths are computed on the CPU, once per case.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _ssim_env_ref as E

pytestmark = pytest.mark.gpu

torch.set_num_threads(4)
GUARD = 64          # NaN-filled floats behind every buffer a kernel writes
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    """Bit for bit; a NaN equals a NaN of any sign and payload."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def D(t):
    return t.detach().cpu().double()


def put(row, key, got, ref, bound):
    """row["K/bound x"] = the largest |got - ref| / bound over the elements, with that element's distance and bound."""
    got, ref, bound = (np.asarray(a.numpy() if torch.is_tensor(a) else a, np.float64).reshape(-1) for a in (got, ref, bound))
    assert np.isfinite(got).all(), (key, "a non-finite element on finite input")
    d = np.abs(got - ref)
    with np.errstate(all="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    i = int(np.argmax(r))
    name = key[len("K/bound "):]
    row[key], row["K " + name], row["bound " + name] = float(r[i]), float(d[i]), float(bound[i])


def inside(row):
    return all(v <= 1.0 for k, v in row.items() if k.startswith("K/bound"))


RECORD = {}
_MUT = {}


def _record(section, key, row):
    RECORD.setdefault(section, {})[key] = row
    out_dir = os.environ.get("CNERF_RECORD_DIR")
    if not out_dir:
        return
    if not _MUT:
        _MUT.update(E.mutant_summary(E.mutant_rows()))
    worst = {}
    for sec, cases in RECORD.items():
        for r in cases.values():
            for k, v in r.items():
                if k.startswith("K/bound"):
                    worst[sec] = max(worst.get(sec, 0.0), v)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "ssim_envelope.json"), "w") as f:
        json.dump({"bounds": "tests/_ssim_env_ref.py: forward = first-order propagation of the kernel's roundings (K_S, K_CS, NF_PATCH); "
                             "backward = C_GRAD u A + 1e-12 max|g64| elementwise",
                   "C_GRAD": E.C_GRAD, "reference_fp32_largest_ratio_cpu": E.REF_RATIO_MEASURED, "K_S": E.K_S, "K_CS": E.K_CS,
                   "NF_PATCH": E.NF_PATCH, "worst_K_over_bound": worst, "mutants_cpu": _MUT, "cases": RECORD}, f, indent=1, sort_keys=True)


# ================================================================================================ the C entry points on guarded buffers
def nanbuf(n, dev):
    return torch.full((int(n) + GUARD,), NAN, device=dev)


def taken(buf, n, what, written=True):
    """The first n floats of a guarded buffer after the call: the guard still NaN, and (written) no element left NaN."""
    assert torch.isnan(buf[int(n):]).all(), f"a write past the end of {what}"
    out = buf[:int(n)]
    if written:
        assert not torch.isnan(out).any(), f"{what}: an element the kernel did not write (or a NaN on finite input)"
    return out


def lib_():
    from consistentnerf_amd import _lib
    return _lib, _lib.load()


def raw_ssim_fwd(dev, X, Y, win, sigma, C1, C2, finite=True):
    _lib, lib = lib_()
    N, Cc, H, W = X.shape
    nws = lib.cnerf_ssim_ws_floats(N, Cc, H, W, win)
    assert nws == 4 * N * Cc * ((H - (win - 1) * (H >= win) + 7) // 8) * ((W - (win - 1) * (W >= win) + 63) // 64)
    ws, s, cs = nanbuf(nws, dev), nanbuf(N * Cc, dev), nanbuf(N * Cc, dev)
    _lib.check(lib.cnerf_ssim_fwd(_p(X), _p(Y), N, Cc, H, W, win, sigma, C1, C2, _p(s), _p(cs), _p(ws), _stream()), "cnerf_ssim_fwd")
    taken(ws, nws, "the forward workspace", False)
    if finite:
        assert not torch.isnan(ws[:nws].view(torch.float64)).any(), "a tile's partial sums were not written"
    return taken(s, N * Cc, "ssim_nc", finite).view(N, Cc), taken(cs, N * Cc, "cs_nc", finite).view(N, Cc)


def raw_ssim_bwd(dev, X, Y, win, sigma, C1, C2, seed, want_dY=True, finite=True):
    _lib, lib = lib_()
    N, Cc, H, W = X.shape
    nws = lib.cnerf_ssim_bwd_ws_floats(N, Cc, H, W, win)
    assert nws == 4 * N * Cc * (H - (win - 1) * (H >= win)) * (W - (win - 1) * (W >= win))
    ws, dX = nanbuf(nws, dev), nanbuf(X.numel(), dev)
    dY = nanbuf(X.numel(), dev) if want_dY else None
    _lib.check(lib.cnerf_ssim_bwd(_p(X), _p(Y), N, Cc, H, W, win, sigma, C1, C2, _p(seed), _p(dX), _p(dY), _p(ws), _stream()),
               "cnerf_ssim_bwd")
    taken(ws, nws, "the backward workspace", finite)
    return (taken(dX, X.numel(), "dX", finite).view_as(X), taken(dY, X.numel(), "dY", finite).view_as(X) if want_dY else None)


def raw_pool(dev, X):
    _lib, lib = lib_()
    N, Cc, H, W = X.shape
    Ho, Wo = H // 2 + H % 2, W // 2 + W % 2
    out = nanbuf(N * Cc * Ho * Wo, dev)
    _lib.check(lib.cnerf_avg_pool2(_p(X), N, Cc, H, W, _p(out), _stream()), "cnerf_avg_pool2")
    return taken(out, N * Cc * Ho * Wo, "the pooled image").view(N, Cc, Ho, Wo)


def pyr_floats(N, Cc, H, W, levels):
    n = 0
    for _ in range(levels - 1):
        H, W = H // 2 + H % 2, W // 2 + W % 2
        n += N * Cc * H * W
    return 2 * n


def raw_ms_fwd(dev, X, Y, win, sigma, C1, C2, levels):
    _lib, lib = lib_()
    N, Cc, H, W = X.shape
    nws, npyr = lib.cnerf_msssim_ws_floats(N, Cc, H, W, win, levels), pyr_floats(N, Cc, H, W, levels)
    assert nws == lib.cnerf_ssim_ws_floats(N, Cc, H, W, win), "level 0 has the most tiles"
    ws, v, pyr = nanbuf(nws, dev), nanbuf(levels * N * Cc, dev), nanbuf(npyr, dev)
    _lib.check(lib.cnerf_msssim_fwd(_p(X), _p(Y), N, Cc, H, W, win, sigma, C1, C2, levels, _p(v), _p(pyr), _p(ws), _stream()),
               "cnerf_msssim_fwd")
    taken(ws, nws, "the MS-SSIM forward workspace", False)
    return taken(v, levels * N * Cc, "v").view(levels, N, Cc), taken(pyr, npyr, "pyr")


def raw_ms_bwd(dev, X, Y, win, sigma, C1, C2, pyr, g_v, want_dY=True):
    _lib, lib = lib_()
    N, Cc, H, W = X.shape
    levels = g_v.shape[0]
    nws = lib.cnerf_msssim_bwd_ws_floats(N, Cc, H, W, win, levels)
    assert nws == lib.cnerf_ssim_bwd_ws_floats(N, Cc, H, W, win) + pyr_floats(N, Cc, H, W, levels)
    ws, dX = nanbuf(nws, dev), nanbuf(X.numel(), dev)
    dY = nanbuf(X.numel(), dev) if want_dY else None
    pyr = pyr if pyr.numel() else nanbuf(0, dev)                       # one level: nothing is read, the pointer must not be null
    _lib.check(lib.cnerf_msssim_bwd(_p(X), _p(Y), N, Cc, H, W, win, sigma, C1, C2, levels, _p(pyr), _p(g_v), _p(dX), _p(dY), _p(ws),
                                    _stream()), "cnerf_msssim_bwd")
    taken(ws, nws, "the MS-SSIM backward workspace", want_dY)
    return taken(dX, X.numel(), "dX").view_as(X), (taken(dY, X.numel(), "dY").view_as(X) if want_dY else None)


def raw_patch(dev, rgb, tgt, P, want_grad=True):
    """value [1] and d_rgb on a buffer of 16 patches + guard: the rows from P * 256 on stay NaN."""
    _lib, lib = lib_()
    value = nanbuf(1, dev)
    d = nanbuf(16 * 768, dev) if want_grad else None
    _lib.check(lib.cnerf_patch_ssim_loss(_p(rgb), _p(tgt), P, _p(value), _p(d), _stream()), "cnerf_patch_ssim_loss")
    return taken(value, 1, "value"), (taken(d, P * 768, "d_rgb (rows from P * 256 on)").view(P * 256, 3) if want_grad else None)


# ================================================================================================ SSIM
def check_planes(tag, got, ref, A, c):
    row = {}
    for name in ("dX", "dY"):
        g, g64, a = D(got[name]), ref[name], A[name]
        put(row, "K/bound " + name, g, g64, E.grad_bound(a, g64, c))
    return row


@pytest.mark.parametrize("c", E.ssim_cases(), ids=lambda c: c.name)
def test_ssim_forward_and_backward_inside_the_bounds(dev, c):
    from consistentnerf_amd import ops
    t = E.truth(c)
    X, Y, seed = t.X.to(dev), t.Y.to(dev), t.seed.to(dev)
    cfg = (c.win, c.sigma, t.C1, t.C2)
    S, cs = raw_ssim_fwd(dev, X, Y, *cfg)
    dX, dY = raw_ssim_bwd(dev, X, Y, *cfg, seed)
    dX1, none = raw_ssim_bwd(dev, X, Y, *cfg, seed, want_dY=False)
    assert none is None and same_bits(dX1, dX), "dX with want_dY = False is the pair's dX"
    # the route Python callers take, and a second call: the same bits
    oS, ocs = ops.ssim_forward(X, Y, *cfg)
    odX, odY = ops.ssim_backward(X, Y, *cfg, seed)
    assert same_bits(oS, S) and same_bits(ocs, cs) and same_bits(odX, dX) and same_bits(odY, dY)
    assert ops.ssim_forward(X, Y, *cfg, want_cs=False)[1] is None and same_bits(ops.ssim_forward(X, Y, *cfg, want_cs=False)[0], S)
    odX1, onone = ops.ssim_backward(X, Y, *cfg, seed, want_dY=False)
    assert onone is None and same_bits(odX1, dX)
    row = {}
    put(row, "K/bound S", D(S), t.S, t.bS)
    put(row, "K/bound cs", D(cs), t.cs, t.bcs)
    put(row, "K/bound dX", D(dX), t.gx, E.grad_bound(t.Ax, t.gx, E.C_GRAD["ssim"]))
    put(row, "K/bound dY", D(dY), t.gy, E.grad_bound(t.Ay, t.gy, E.C_GRAD["ssim"]))
    if c.fam == "same":
        assert ((D(S) - 1).abs() <= t.bS).all(), "S of an image with itself"
    N, Cc = c.planes
    for n in range(N):
        for ch in range(Cc):
            if float(t.seed[n, ch]) == 0.0:
                assert not dX[n, ch].any() and not dY[n, ch].any(), "a plane with seed 0 has gradient exactly 0"
            if N * Cc > 1:                                                  # plane p of the batch = the same plane run alone
                xs, ys, sd = X[n:n + 1, ch:ch + 1].contiguous(), Y[n:n + 1, ch:ch + 1].contiguous(), seed[n:n + 1, ch:ch + 1].contiguous()
                pS, pcs = ops.ssim_forward(xs, ys, *cfg)
                pdX, pdY = ops.ssim_backward(xs, ys, *cfg, sd)
                assert same_bits(pS[0, 0], S[n, ch]) and same_bits(pcs[0, 0], cs[n, ch]), ("plane", n, ch)
                assert same_bits(pdX[0, 0], dX[n, ch]) and same_bits(pdY[0, 0], dY[n, ch]), ("plane", n, ch)
    print(f"ssim {c.name}: {row}")
    _record("ssim", c.name, row)
    assert inside(row), row


def test_ssim_non_finite_pixels_stay_in_their_planes(dev):
    """One NaN pixel in plane 0 and one inf pixel in plane 1 of three: plane 2's values and gradients are the finite run's bit for bit,
    planes 0 and 1 report a non-finite mean."""
    from consistentnerf_amd import ops
    X, Y = E.images("noise", (1, 3, 19, 75), 77)
    seed = torch.tensor([[0.5, -1.0, 2.0]])
    taps_cfg = (11, 1.5, *E.consts(1.0))
    X, Y, seed = X.to(dev), Y.to(dev), seed.to(dev)
    S, cs = ops.ssim_forward(X, Y, *taps_cfg)
    dX, dY = ops.ssim_backward(X, Y, *taps_cfg, seed)
    Xb = X.clone()
    Xb[0, 0, 9, 40] = NAN
    Xb[0, 1, 3, 70] = float("inf")
    Sb, csb = raw_ssim_fwd(dev, Xb, Y, *taps_cfg, finite=False)
    dXb, dYb = raw_ssim_bwd(dev, Xb, Y, *taps_cfg, seed, finite=False)
    assert not torch.isfinite(Sb[0, 0]) and not torch.isfinite(Sb[0, 1]) and not torch.isfinite(csb[0, 0]) and not torch.isfinite(csb[0, 1])
    assert same_bits(Sb[0, 2], S[0, 2]) and same_bits(csb[0, 2], cs[0, 2])
    assert same_bits(dXb[0, 2], dX[0, 2]) and same_bits(dYb[0, 2], dY[0, 2])
    assert torch.isfinite(dXb[0, 2]).all() and not torch.isfinite(dXb[0, 0]).all() and not torch.isfinite(dXb[0, 1]).all()


# ================================================================================================ avg_pool2
def test_avg_pool2_every_parity(dev):
    """H, W in {1, 2, 3, 4, 5, 64, 65} on two planes of signed values: within 3 u sum|taps| / 4 of avg_pool2d in float64 (padding
    (H % 2, W % 2), counted); exact on small integers; ops.avg_pool2 gives the same bits."""
    from consistentnerf_amd import ops
    worst = {}
    for H in (1, 2, 3, 4, 5, 64, 65):
        for W in (1, 2, 3, 4, 5, 64, 65):
            g = torch.Generator().manual_seed(1000 * H + W)
            X = torch.rand(1, 2, H, W, generator=g) * 2 - 1
            ref, b = E.pool64(X)
            got = raw_pool(dev, X.to(dev))
            assert same_bits(ops.avg_pool2(X.to(dev)), got)
            row = {}
            put(row, "K/bound pool", D(got), ref, b)
            if row["K/bound pool"] >= worst.get("K/bound pool", -1.0):
                worst = dict(row, at=f"{H}x{W}")
            Xi = torch.randint(-8, 9, (1, 2, H, W), generator=g).float()
            assert torch.equal(D(raw_pool(dev, Xi.to(dev))), E.pool64(Xi)[0]), ("small integers pool exactly", H, W)
    print(f"avg_pool2: {worst}")
    _record("avg_pool2", "all", worst)
    assert inside(worst), worst


# ================================================================================================ MS-SSIM
def _weights(levels):
    return list((E.R.MS_WEIGHTS if levels <= 5 else E.MS_WEIGHTS6)[:levels])


@pytest.mark.parametrize("c", E.ms_cases(), ids=lambda c: c.name)
def test_msssim_levels_and_gradients_inside_the_bounds(dev, c):
    from consistentnerf_amd import ops, ssim as S
    t = E.truth(c)
    X, Y, g_v = t.X.to(dev), t.Y.to(dev), t.seed.to(dev)
    cfg = (c.win, c.sigma, t.C1, t.C2)
    v, pyr = raw_ms_fwd(dev, X, Y, *cfg, c.levels)
    dX, dY = raw_ms_bwd(dev, X, Y, *cfg, pyr, g_v)
    dX1, none = raw_ms_bwd(dev, X, Y, *cfg, pyr, g_v, want_dY=False)
    assert none is None and same_bits(dX1, dX), "dX with want_dY = False is the pair's dX"
    ov, opyr = ops.msssim_forward(X, Y, *cfg, c.levels)
    odX, odY = ops.msssim_backward(X, Y, *cfg, opyr, g_v)
    assert same_bits(ov, v) and same_bits(opyr[:pyr.numel()], pyr) and same_bits(odX, dX) and same_bits(odY, dY)
    assert same_bits(ops.msssim_backward(X, Y, *cfg, opyr, g_v, want_dY=False)[0], dX)
    row = {}
    put(row, "K/bound v", D(v), t.v, t.bv)
    put(row, "K/bound dX", D(dX), t.gx, E.grad_bound(t.Ax, t.gx, E.C_GRAD["msssim"]))
    put(row, "K/bound dY", D(dY), t.gy, E.grad_bound(t.Ay, t.gy, E.C_GRAD["msssim"]))
    # the pooled levels the forward keeps: [levels 1.. of X][levels 1.. of Y]
    N, Cc = c.planes
    half, off, pyr_c = pyr.numel() // 2, 0, D(pyr)
    for l in range(1, c.levels):
        x64, y64 = t.pyr[l]
        n = x64.numel()
        for img, base, name in ((x64, 0, "X"), (y64, half, "Y")):
            got = pyr_c[base + off:base + off + n].view_as(img)
            put(row, f"K/bound pyr {name} level {l}", got, img, E.POOL_U * l * E.U * img.abs() * (1 + 1e-6) + 1e-300)
        off += n
    assert off == half
    # the assembled value through consistentnerf_amd.ssim.ms_ssim
    w = _weights(c.levels)
    val = S.ms_ssim(X, Y, data_range=c.dr, size_average=False, win_size=c.win, win_sigma=c.sigma, weights=w)
    w64 = torch.tensor(w, dtype=torch.float64).view(-1, 1, 1)
    val64 = torch.prod(torch.relu(t.v) ** w64, dim=0)                       # [N, C]
    pos, neg = ((t.v - t.bv) > 0).all(0), ((t.v + t.bv) < 0).any(0)
    assert (pos | neg).all(), "a level's mean within its bound of 0: choose another input"
    rel = (w64 * t.bv / (t.v - t.bv).clamp_min(1e-300)).sum(0) + 4 * (c.levels + 1) * E.U     # pow, the product, per level
    bval = torch.where(pos, rel * val64, torch.zeros_like(val64)).mean(1) + 2 * E.U * val64.mean(1)
    put(row, "K/bound ms_ssim", D(val), val64.mean(1), bval + 1e-300)
    print(f"msssim {c.name}: {row}")
    _record("msssim", c.name, row)
    assert inside(row), row


# ================================================================================================ the patch term
@pytest.mark.parametrize("P", range(1, 17))
def test_patch_term_every_patch_count(dev, P):
    from consistentnerf_amd import ops
    for fam in E.PATCH_FAMILIES:
        t = E.patch_truth(P, fam)
        rgb, tgt = t.rgb.to(dev), t.tgt.to(dev)
        value, d = raw_patch(dev, rgb, tgt, P)
        ov, od = ops.patch_ssim_loss(rgb, tgt, P)
        assert same_bits(ov, value) and same_bits(od, d)
        v0, none = raw_patch(dev, rgb, tgt, P, want_grad=False)
        assert none is None and same_bits(v0, value)
        row = {}
        put(row, "K/bound value", D(value), t.v, t.bv)
        sh = (1, 1, -1, 3)
        put(row, "K/bound d_rgb", D(d).reshape(sh), t.g.reshape(sh), E.grad_bound(t.A.reshape(sh), t.g.reshape(sh), E.C_GRAD["patch"]))
        if fam == "same":
            assert abs(float(value) - P / 4) <= t.bv
        print(f"patch P={P} {fam}: {row}")
        _record("patch", f"P{P}-{fam}", row)
        assert inside(row), row


@pytest.mark.parametrize("P", [0, 17])
def test_patch_term_rejects_patch_counts_outside_1_16(dev, P):
    from consistentnerf_amd import ops
    from consistentnerf_amd._lib import CnerfError
    rgb, tgt = E.patch_inputs(17, "noise")
    with pytest.raises(CnerfError):
        ops.patch_ssim_loss(rgb.to(dev), tgt.to(dev), P)
    _lib, lib = lib_()
    value, d = nanbuf(1, dev), nanbuf(17 * 768, dev)
    assert lib.cnerf_patch_ssim_loss(_p(rgb.to(dev)), _p(tgt.to(dev)), P, _p(value), _p(d), _stream()) != 0
    assert torch.isnan(value).all() and torch.isnan(d).all(), "a refused call writes nothing"


# ================================================================================================ beyond the limits
@pytest.mark.parametrize("shape,win", [((1, 1, 40, 40), 2), ((1, 1, 40, 40), 10), ((1, 1, 40, 40), 33), ((1, 1, 40, 40), 0),
                                       ((1, 65536, 1, 1), 11)], ids=lambda v: str(v).replace(" ", ""))
def test_beyond_the_limits_raises_and_writes_nothing(dev, shape, win):
    from consistentnerf_amd import ops
    from consistentnerf_amd._lib import CnerfError
    _lib, lib = lib_()
    N, Cc, H, W = shape
    X = torch.full(shape, 0.5, device=dev)
    Y = torch.full(shape, 0.25, device=dev)
    seed = torch.ones(N, Cc, device=dev)
    C1, C2 = E.consts(1.0)
    with pytest.raises(CnerfError):
        ops.ssim_forward(X, Y, win, 1.5, C1, C2)
    with pytest.raises(CnerfError):
        ops.ssim_backward(X, Y, win, 1.5, C1, C2, seed)
    with pytest.raises(CnerfError):
        ops.msssim_forward(X, Y, win, 1.5, C1, C2, 1)
    n = X.numel()
    s, cs, ws, dX, dY, pyr = (nanbuf(k, dev) for k in (3 * N * Cc, N * Cc, 8 * n + 8, n, n, 2 * n))
    g3 = torch.ones(3, N, Cc, device=dev)
    rcs = [lib.cnerf_ssim_fwd(_p(X), _p(Y), N, Cc, H, W, win, 1.5, C1, C2, _p(s), _p(cs), _p(ws), _stream()),
           lib.cnerf_ssim_bwd(_p(X), _p(Y), N, Cc, H, W, win, 1.5, C1, C2, _p(seed), _p(dX), _p(dY), _p(ws), _stream()),
           lib.cnerf_msssim_fwd(_p(X), _p(Y), N, Cc, H, W, win, 1.5, C1, C2, 3, _p(s), _p(pyr), _p(ws), _stream()),
           lib.cnerf_msssim_bwd(_p(X), _p(Y), N, Cc, H, W, win, 1.5, C1, C2, 3, _p(pyr), _p(g3), _p(dX), _p(dY), _p(ws), _stream())]
    assert all(rc != 0 for rc in rcs), rcs
    for b in (s, cs, ws, dX, dY, pyr):
        assert torch.isnan(b).all(), "a refused call writes nothing"
