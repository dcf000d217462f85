"""GPU tests of csrc/depthvis.hip (ops.depthvis, io_formats.lky_visualize_depth) against the recorded reference frames
(tests/golden/depthvis.npz) and the numpy restatement tests/_depthvis_ref.py.

Bounds: against the float64 form of the restatement (the kernel's running sum is fp64), relative error <= 1e-6: the two bracketing
elements are selected exactly, so anything larger is a wrong bracket.  Image: against the reference (fixture frames) or the float32
form (seeded frames): the LUT index of every pixel within +-1 — observed through the bytes: every pixel's bytes lie within 1 of the
bytes the reference's index, or a neighbouring one, gives —, within 9 = 1 + ceil(255 * largest LUT step) of the reference's bytes where
the index moved, and at most 0.5 % of a frame's pixels differing from the reference at all.
"""
import functools

import numpy as np
import pytest
import torch

import _depthvis_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _fix():
    return golden("depthvis")


def _seeded(H, W, seed, ties):
    """depth smooth plus noise (ties: quantised to 16 values), weights with zero-weight runs at finite depth, exact ones, and a block
    where nothing accumulated (acc 0, disp NaN)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = np.maximum(2 + 3 * xx * yy + np.sin(5 * xx) + 0.1 * rs.standard_normal((H, W)), 0.3)
    if ties:
        depth = 0.5 + 5.5 * np.round(15 * np.clip((depth - 0.5) / 5.5, 0, 1)) / 15
    acc = rs.uniform(size=(H, W)).astype(np.float32)
    acc[rs.uniform(size=(H, W)) < 0.3] = 0
    acc[rs.uniform(size=(H, W)) < 0.1] = 1
    disp = (1 / depth).astype(np.float32)
    disp[H // 4:H // 2, W // 4:W // 2] = np.nan
    acc[H // 4:H // 2, W // 4:W // 2] = 0
    return disp, acc


CASES = {"fix0": None, "fix1": None, "8x8": (8, 8, 1, False), "48x64_ties": (48, 64, 2, True), "161x176": (161, 176, 3, False),
         "161x176_ties": (161, 176, 4, True), "378x504": (378, 504, 5, False)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(disp, acc, reference image float64, its LUT indices or None, float64-form bounds): computed once, never modified."""
    f = _fix()
    if name.startswith("fix"):
        disp, acc = f["disp_" + name[3:]], f["acc_" + name[3:]]
    else:
        disp, acc = _seeded(*CASES[name])
    with np.errstate(all="ignore"):
        x = 1 / disp
    img, idx, _ = R.visualize(x, acc, f["lut"], dtype=np.float32, parts=True)
    if name.startswith("fix"):
        assert np.array_equal(img, f["img_" + name[3:]])
    return disp, acc, img, idx, R.weighted_bounds(x, acc, np.float64)


def _run(dev, disp, acc, **kw):
    from consistentnerf_amd import ops
    d, a = torch.from_numpy(np.ascontiguousarray(disp)).to(dev), torch.from_numpy(np.ascontiguousarray(acc)).to(dev)
    if d.dim() == 2:
        d, a = d[None], a[None]
    f32, u8, b = ops.depthvis(d, a, **kw)
    torch.cuda.synchronize()
    return f32.cpu().numpy(), u8.cpu().numpy(), b.cpu().numpy()


def _check_bounds(got, want, label):
    want = np.asarray(want, np.float64)
    rel = np.abs(got.astype(np.float64) - want) / np.abs(want)
    print(f"{label}: bounds {got} want {want} rel {rel}")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert (rel[~np.isnan(want)] <= 1e-6).all()


def _check_image(f32, u8, acc, img_ref, idx_ref, label):
    lut = _fix()["lut"]
    u8_ref = R.to_u8(img_ref).astype(np.int64)
    a = acc.astype(np.float64)[:, :, None]
    dist = {d: np.abs(u8 - R.to_u8(lut[np.clip(idx_ref + d, 0, 255)] * a + (1 - a)).astype(np.int64)).max(-1) for d in (-1, 0, 1)}
    same = dist[0] <= 1
    near = ~same & ((dist[-1] <= 1) | (dist[1] <= 1))
    byte_d = np.abs(u8 - u8_ref).max(-1)
    frac = (byte_d > 0).mean()
    float_d = np.abs(f32.astype(np.float64) - img_ref).max(-1)
    print(f"{label}: pixels on the reference's LUT entry {same.mean():.6f}, on a neighbouring one {near.mean():.6f}, "
          f"differing at all {frac:.6f}, max byte difference {byte_d.max()}, max float difference {float_d.max():.3e}")
    assert (same | near).all(), "a pixel's LUT index is off by more than one"
    assert byte_d[same].max(initial=0) <= 1 and byte_d[near].max(initial=0) <= 9
    assert frac <= 0.005
    # the float image: four fp32 roundings (<= 4 * 2^-24 at values <= 1) next to the float64 reference where the index agrees, one
    # LUT step times acc more where it moved, and that on at most 0.5 % of the pixels
    step = np.abs(np.diff(lut, axis=0)).max()
    assert (float_d <= step * acc + 1e-6).all() and (float_d > 1e-6).mean() <= 0.005
    assert np.array_equal(R.to_u8(f32), u8)


@pytest.mark.parametrize("name", list(CASES))
def test_bounds_and_image(dev, name):
    disp, acc, img, idx, b64 = _case(name)
    f32, u8, b = _run(dev, disp, acc)
    _check_bounds(b[0], b64, name)
    _check_image(f32[0], u8[0].astype(np.int64), acc, img, idx, name)


def test_reference_bytes_of_the_fixture(dev):
    """The recorded PNG bytes themselves (not only the restatement's) bound the kernel's."""
    f = _fix()
    for k in (0, 1):
        _, u8, _ = _run(dev, f[f"disp_{k}"], f[f"acc_{k}"])
        d = np.abs(u8[0].astype(np.int64) - f[f"u8_{k}"]).max(-1)
        print(f"fixture frame {k}: {(d > 0).mean():.6f} of the pixels differ, max {d.max()}")
        assert d.max() <= 9 and (d > 0).mean() <= 0.005


def test_single_weighted_pixel_and_empty_frame(dev):
    f = _fix()
    # one pixel carries all the weight: both percentiles are that pixel's value; hi_auto - lo_auto = 0 puts its colour outside the
    # parity claim (a quotient of two eps-sized numbers), every other pixel is white
    disp, acc = f["disp_2"], f["acc_2"]
    f32, u8, b = _run(dev, disp, acc)
    with np.errstate(all="ignore"):
        _check_bounds(b[0], R.weighted_bounds(1 / disp, acc, np.float64), "single")
    assert (u8[0][acc == 0] == 255).all() and np.isfinite(f32).all() and f32.min() >= 0 and f32.max() <= 1
    # nothing accumulated anywhere: the reference's image is white
    f32, u8, b = _run(dev, f["disp_3"], f["acc_3"])
    assert (u8 == 255).all() and (f32 == 1).all() and np.isnan(b).all()
    assert (f["u8_3"] == 255).all()


def test_two_calls_identical_and_batch_equals_singles(dev):
    f = _fix()
    frames = [(f["disp_0"], f["acc_0"]), _seeded(48, 64, 2, True), (f["disp_3"], f["acc_3"])]
    disp, acc = np.stack([d for d, _ in frames]), np.stack([a for _, a in frames])
    one, two = _run(dev, disp, acc), _run(dev, disp, acc)
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()
    for k, (d, a) in enumerate(frames):
        for whole, single in zip(one, _run(dev, d, a)):
            assert whole[k].tobytes() == single[0].tobytes()
    assert not np.array_equal(one[1][0], one[1][1])
    d, a = _case("378x504")[:2]
    for x, y in zip(_run(dev, d, a), _run(dev, d, a)):
        assert x.tobytes() == y.tobytes()


def test_explicit_limits(dev):
    disp, acc, _, _, _ = _case("161x176")
    lut = _fix()["lut"]
    with np.errstate(all="ignore"):
        x = 1 / disp
    auto = _run(dev, disp, acc)
    for lo, hi in ((1.5, 3.0), (None, 2.5), (1.25, None)):
        f32, u8, b = _run(dev, disp, acc, lo=lo, hi=hi)
        assert np.array_equal(b, auto[2])                                        # bounds stay the automatic ones
        img, idx, _ = R.visualize(x, acc, lut, lo=lo, hi=hi, parts=True)
        _check_image(f32[0], u8[0].astype(np.int64), acc, img, idx, f"lo={lo} hi={hi}")
        assert not np.array_equal(u8, auto[1])
    zero = _run(dev, disp, acc, lo=0, hi=0.)                                     # `lo or ...`: a passed 0 counts as not passed
    assert all(p.tobytes() == q.tobytes() for p, q in zip(zero, auto))


def test_constant_depth_plane_is_finite_and_in_range(dev):
    """hi_auto - lo_auto < 1e-4 lo_auto: outside the parity claim; only finite, in-range output is asserted."""
    rs = np.random.RandomState(7)
    disp, acc = np.full((48, 64), 0.4, np.float32), rs.uniform(size=(48, 64)).astype(np.float32)
    f32, u8, b = _run(dev, disp, acc)
    assert np.isfinite(f32).all() and f32.min() >= 0 and f32.max() <= 1 and np.isfinite(b).all()
    assert np.allclose(b, 2.5, rtol=1e-6)


def test_wrapper_and_argument_errors(dev):
    from consistentnerf_amd import CnerfError, io_formats, ops
    disp, acc, _, _, _ = _case("48x64_ties")
    with np.errstate(all="ignore"):
        x = 1 / disp
    img = io_formats.lky_visualize_depth(x, acc)
    assert isinstance(img, np.ndarray) and img.shape == (48, 64, 3) and img.dtype == np.float32
    xt = torch.from_numpy(x).to(dev)
    assert np.array_equal(img, ops.depthvis((1. / xt)[None], torch.from_numpy(acc).to(dev)[None], want_u8=False)[0][0].cpu().numpy())
    batch = io_formats.lky_visualize_depth(torch.from_numpy(np.stack([x, x])).to(dev), torch.from_numpy(np.stack([acc, acc])).to(dev))
    assert torch.is_tensor(batch) and batch.shape == (2, 48, 64, 3) and np.array_equal(batch[1].cpu().numpy(), img)
    with pytest.raises(CnerfError):
        ops.depthvis(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4))
    with pytest.raises(CnerfError):
        ops.depthvis(torch.zeros(1, 4, 4, device=dev), torch.zeros(1, 4, 5, device=dev))
