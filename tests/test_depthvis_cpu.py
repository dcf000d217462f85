"""CPU tests of the depth-map image path: the numpy restatement tests/_depthvis_ref.py against the recorded reference frames
(tests/golden/depthvis.npz, make_golden_depthvis.py), the LUT header against the recorded colormap, the standard-library PNG encoder,
and the metrics.txt logic of run_nerf_view.evaluate_testset.  No GPU."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import _depthvis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = 4


@pytest.fixture(scope="module")
def fix(gold):
    return gold("depthvis")


def _x(disp):
    with np.errstate(all="ignore"):
        return 1 / disp


@pytest.mark.parametrize("k", range(N_FRAMES))
def test_float32_restatement_reproduces_the_reference(fix, k):
    img = R.visualize(_x(fix[f"disp_{k}"]), fix[f"acc_{k}"], fix["lut"], dtype=np.float32)
    assert img.dtype == np.float64 and np.abs(img - fix[f"img_{k}"]).max() <= 1e-12
    assert np.array_equal(R.to_u8(img), fix[f"u8_{k}"])


def test_fixture_frames_cover_the_stated_cases(fix):
    assert [fix[f"disp_{k}"].shape for k in range(N_FRAMES)] == [(48, 64), (161, 176), (48, 64), (48, 64)]
    for k in (0, 1):
        acc, disp = fix[f"acc_{k}"], fix[f"disp_{k}"]
        assert (acc == 0).sum() > 100 and (acc == 1).sum() > 100 and 0 <= acc.min() and acc.max() <= 1
        assert np.array_equal(np.isnan(disp), acc == 0)
    assert (fix["acc_2"] > 0).sum() == 1                                  # one pixel carries all the weight
    assert (fix["acc_3"] == 0).all() and (fix["u8_3"] == 255).all()      # nothing accumulated: the reference's image is white


def test_float64_running_sum_moves_no_fixture_pixel(fix):
    """The basis of the GPU test's 0.5 % cap: on the committed frames the float64 running sum (the kernel's) picks the LUT entry the
    reference's float32 one picks, at every pixel."""
    for k in range(N_FRAMES):
        x, acc = _x(fix[f"disp_{k}"]), fix[f"acc_{k}"]
        _, i32, b32 = R.visualize(x, acc, fix["lut"], dtype=np.float32, parts=True)
        _, i64, b64 = R.visualize(x, acc, fix["lut"], dtype=np.float64, parts=True)
        assert np.array_equal(i32, i64)
        assert np.allclose(b32, b64, rtol=1e-6, atol=0, equal_nan=True)


def test_largest_lut_step_is_what_the_gpu_bound_assumes(fix):
    assert np.ceil(255 * np.abs(np.diff(fix["lut"], axis=0)).max()) == 8          # 7.48 / 255: the bound 1 + 8 = 9


def test_lut_header_equals_the_recorded_colormap(fix):
    src = open(os.path.join(ROOT, "consistentnerf_amd", "csrc", "turbo_lut.hpp")).read()
    body = src[src.index("CN_TURBO_LUT[256][3]"):]
    vals = np.array([np.float32(v) for v in re.findall(r"([0-9.eE+-]+)f\b", body)], dtype=np.float32).reshape(256, 3)
    assert np.array_equal(vals, fix["lut"].astype(np.float32))


def test_interp_restatement_matches_numpy():
    rs = np.random.RandomState(0)
    w = rs.uniform(size=200) * (rs.uniform(size=200) > 0.4)                    # runs of equal running sums
    xp, fp = np.cumsum(w), np.sort(rs.standard_normal(200))
    for t in list(rs.uniform(-1, xp[-1] + 1, size=200)) + list(xp[::7]) + [xp[0], xp[-1], np.nan]:
        a, b = R.interp(t, xp, fp), np.interp(t, xp, fp)
        assert a == b or (np.isnan(a) and np.isnan(b))


def _decode_png(data):
    """A test-local decoder for what io_formats.png_bytes writes (8-bit grey / RGB, filter 0), CRCs checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (161, 176)])
@pytest.mark.parametrize("rgb", [True, False])
def test_fallback_png_encoder_roundtrip(tmp_path, shape, rgb):
    from consistentnerf_amd import io_formats as F
    rs = np.random.RandomState(shape[0])
    img = rs.randint(0, 256, size=shape + ((3,) if rgb else ())).astype(np.uint8)
    pth = str(tmp_path / "a.png")
    F.save_img_u8(img, pth, use_pil=False)
    data = open(pth, "rb").read()
    assert data == F.png_bytes(img) and np.array_equal(_decode_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(pth)), img)
    # a float image goes through the reference's byte rule
    f = rs.uniform(-0.2, 1.2, size=shape + (3,))
    f.flat[0] = np.nan
    F.save_img_u8(f, pth, use_pil=False)
    assert np.array_equal(_decode_png(open(pth, "rb").read()), R.to_u8(f))


def test_metrics_file_masked_and_plain_branch(tmp_path):
    from consistentnerf_amd import run_nerf_view as V
    plain = {"psnr": 23.456789012345, "ssim": 0.812345678, "msssim": 0.9, "lpips": 0.123456789}
    masked = dict(plain, psnr_mask=27.5, ssim_mask=0.91, msssim_mask=0.95, lpips_mask=0.0625)
    for m, sfx in ((plain, ""), (masked, "_mask")):
        text = open(V.write_testset_metrics(str(tmp_path), m)).read()
        assert text == f"PSNR: {m['psnr' + sfx]}\nSSIM: {m['ssim' + sfx]}\nLPIPS: {m['lpips' + sfx]}"
        got = dict(ln.split(": ") for ln in text.split("\n"))
        assert [float(got[k]) for k in ("PSNR", "SSIM", "LPIPS")] == [m["psnr" + sfx], m["ssim" + sfx], m["lpips" + sfx]]
