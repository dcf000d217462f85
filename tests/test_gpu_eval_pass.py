"""GPU tests of the test-set pass (V:2034-2087): ops.eval_prep (csrc/depthvis.hip: cnerf_eval_prep) against the ATen lines of
io_formats.img2ssim / img2lpips, and run_nerf_view.evaluate_testset against the composition it replaces (render_path + the io_formats
metric functions) on a seeded pair of D = 4 / W = 64 networks, 2 poses at 161 x 176 (MS-SSIM needs a side above 160)."""
import os

import numpy as np
import pytest
import torch

import _inputs as I
import _lpips_ref as LR

pytestmark = pytest.mark.gpu

H, W, N = 161, 176, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _frames(seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.4 * np.sin(6 * xx[None, :, :, None] + np.arange(3)[None, None, None, :] + np.arange(N)[:, None, None, None]) * np.cos(4 * yy)[None, :, :, None]
    gt = np.clip(base + 0.03 * rs.standard_normal((N, H, W, 3)), 0, 1).astype(np.float32)
    pred = np.clip(gt + 0.08 * rs.standard_normal((N, H, W, 3)), 0, 1).astype(np.float32)
    mask = (xx[None] - 0.5) ** 2 + (yy[None] - 0.45) ** 2 < np.array([0.12, 0.2])[:, None, None]
    return pred, gt, mask


@pytest.mark.parametrize("masked", [False, True])
def test_eval_prep_matches_the_aten_lines(dev, masked):
    from consistentnerf_amd import ops
    pred, gt, mask = _frames(1)
    x, y = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    m = torch.from_numpy(mask).to(device=dev, dtype=torch.float32) if masked else None
    (sp, sg), (lp, lg), sums = ops.eval_prep(x, y, m)
    # io_formats.img2ssim's lines
    ex, ey = (m.unsqueeze(-1) * x, m.unsqueeze(-1) * y) if masked else (x, y)
    assert torch.equal(sp, ex.permute(0, 3, 1, 2).contiguous()) and torch.equal(sg, ey.permute(0, 3, 1, 2).contiguous())
    # io_formats.img2lpips' lines
    eg, ep = ((y - 0.5) * 2.).permute([0, 3, 1, 2]), ((x - 0.5) * 2.).permute([0, 3, 1, 2])
    if masked:
        m3 = m.unsqueeze(1).expand(-1, 3, -1, -1)
        eg, ep = eg * m3 + (1 - m3), ep * m3 + (1 - m3)
    assert torch.equal(lp, ep.contiguous()) and torch.equal(lg, eg.contiguous())
    # the PSNR partials against float64 numpy
    d2 = (pred.astype(np.float64) - gt.astype(np.float64)) ** 2
    mk = mask.astype(np.float64) if masked else np.ones((N, H, W))
    want = [d2.sum()]
    for n in range(N):
        want += [(mk[n] * d2[n].mean(-1)).sum(), mk[n].sum()]
    got = sums.cpu().numpy()
    rel = np.abs(got - np.array(want)) / np.abs(want)
    print("PSNR partials", got, "relative error", rel)
    assert got.dtype == np.float64 and (rel <= 1e-12).all()
    # two calls: identical bits; the selective outputs
    again = ops.eval_prep(x, y, m)
    assert torch.equal(again[2], sums) and torch.equal(again[0][0], sp) and torch.equal(again[1][1], lg)
    only = ops.eval_prep(x, y, m, want_ssim=False, want_sums=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1][0], lp)


def _model(seed, dev):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = I.nerf_state_dict(4, 64, 10, 4, 5, True, seed)
    m = NeRF(D=4, W=64, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Rendered once: the composition of the parent commit (render_path, then the io_formats functions on its host frames) and
    evaluate_testset with and without a foreground mask, files included."""
    from consistentnerf_amd import io_formats as F, run_nerf_view as V
    from consistentnerf_amd.lpips import LPIPS
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    dev = torch.device("cuda:0")
    e, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    kw = dict(network_query_fn=lambda i, v, f: run_network(i, v, f, embed_fn=e, embeddirs_fn=ed), perturb=0.0, N_importance=16,
              network_fine=_model(52, dev), N_samples=16, network_fn=_model(51, dev), white_bkgd=False, raw_noise_std=0.0,
              lindisp=False, ndc=False, near=2.0, far=6.0, use_viewdirs=True)
    focal = 150.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = [torch.from_numpy(F.pose_spherical(th, -30.0, 4.0)).to(dev) for th in (20.0, 65.0)]
    _, gt, mask = _frames(2)
    lpips_fn = LPIPS(net="vgg", weights=LR.package_state_dict(LR.make_weights(0))).to(dev)
    rgbs, disps, accs = V.render_path(poses, (H, W, focal), K, 8192, kw)
    tmp = str(tmp_path_factory.mktemp("testset"))
    out = {}
    for tag, m in (("plain", None), ("mask", mask)):
        d = os.path.join(tmp, tag)
        os.makedirs(os.path.join(d, "frames"))
        out[tag] = (V.evaluate_testset(poses, (H, W, focal), K, 8192, kw, gt, lpips_fn, depth_mask=m, savedir=os.path.join(d, "frames"),
                                       outdir=d), d)
    torch.cuda.synchronize()
    return dict(rgbs=rgbs, disps=disps, accs=accs, gt=gt, mask=mask, lpips_fn=lpips_fn, out=out)


def _read_png(path):
    try:
        from PIL import Image
    except ImportError:
        from test_depthvis_cpu import _decode_png
        return _decode_png(open(path, "rb").read())
    return np.asarray(Image.open(path))


@pytest.mark.parametrize("tag", ["plain", "mask"])
def test_evaluate_testset(dev, scene, tag):
    from consistentnerf_amd import io_formats as F
    from consistentnerf_amd.run_nerf_helpers import img2mse, mse2psnr, to8b
    s = scene
    res, outdir = s["out"][tag]
    rgbs, gt, mask = s["rgbs"], s["gt"], s["mask"]
    # the frames: render_path's, bit for bit
    assert np.array_equal(res["rgbs"], rgbs) and np.array_equal(res["disps"], s["disps"], equal_nan=True)
    assert np.array_equal(res["accs"], s["accs"])
    assert res["rgbs"].shape == (N, H, W, 3) and res["depth_vis_u8"].shape == (N, H, W, 3) and res["depth_vis_u8"].dtype == np.uint8
    # SSIM / MS-SSIM / LPIPS: the same kernels on identical inputs
    want_ssim, want_ms = F.img2ssim(rgbs, gt)
    assert res["ssim"] == float(want_ssim) and res["msssim"] == float(want_ms)
    assert res["lpips"] == float(F.img2lpips(rgbs, gt, s["lpips_fn"]))
    want_psnr = float(mse2psnr(img2mse(torch.from_numpy(rgbs), torch.from_numpy(gt)).cpu()))
    print(f"{tag}: psnr {res['psnr']} (fp32 lines {want_psnr}) ssim {res['ssim']} msssim {res['msssim']} lpips {res['lpips']}")
    assert abs(res["psnr"] - want_psnr) <= 1e-5
    assert abs(res["psnr"] - float(F.img2psnr(rgbs, gt))) <= 1e-5
    keys = ("psnr", "ssim", "lpips")
    if tag == "mask":
        ws, wm = F.img2ssim(rgbs, gt, mask)
        assert res["ssim_mask"] == float(ws) and res["msssim_mask"] == float(wm)
        assert res["lpips_mask"] == float(F.img2lpips(rgbs, gt, s["lpips_fn"], mask=mask))
        want = float(F.img2psnr_mask(torch.from_numpy(rgbs), torch.from_numpy(gt), torch.from_numpy(mask).float()))
        print(f"mask: psnr_mask {res['psnr_mask']} (fp32 lines {want})")
        assert abs(res["psnr_mask"] - want) <= 1e-5 and res["ssim_mask"] != res["ssim"]
        keys = ("psnr_mask", "ssim_mask", "lpips_mask")
    else:
        assert "psnr_mask" not in res
    # the files
    got = dict(ln.split(": ") for ln in open(os.path.join(outdir, "metrics.txt")).read().split("\n"))
    assert [float(got[k]) for k in ("PSNR", "SSIM", "LPIPS")] == [res[k] for k in keys]
    for i in range(N):
        assert np.array_equal(_read_png(os.path.join(outdir, f"depth_{i:03d}.png")), res["depth_vis_u8"][i])
        assert np.array_equal(_read_png(os.path.join(outdir, "frames", f"color_{i:03d}.png")), to8b(rgbs[i]))
    # the depth images are the kernel's on these frames
    from consistentnerf_amd import ops
    _, u8, b = ops.depthvis(torch.from_numpy(s["disps"]).to(dev), torch.from_numpy(s["accs"]).to(dev), want_f32=False)
    assert np.array_equal(u8.cpu().numpy(), res["depth_vis_u8"]) and np.array_equal(b.cpu().numpy(), res["depth_bounds"], equal_nan=True)
