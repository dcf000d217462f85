"""The test-set pass on one MI355X: `python scripts/evalpass_bench.py [--out profiles/evalpass_bench.json]`.

  depthvis   ops.depthvis (cnerf_depthvis: img_u8 + bounds) at 4 x 378 x 504 and 1 x 756 x 1008 against the numpy statement
             (tests/_depthvis_ref.py, float32 form, + to_u8) on this box's host; the bytes the launches move (every select pass reads
             disp and acc, the colour pass reads both and writes 3 bytes per pixel) over the time, next to the 8 TB/s HBM figure.
  testset    wall time of run_nerf_view.evaluate_testset for 4 frames of 378 x 504 (D = 8 / W = 256 networks, 64 + 64 samples, seeded
             LPIPS weights, a foreground mask) against the composition the parent commit offers: render_path, then the io_formats
             metric functions on its host frames and the numpy visualiser.
  launches   device launches of evaluate_testset beyond those of rendering the same poses (everything between the last render
             launch and the first copy to the host), and the copies to the host of both.
The arms alternate round by round (the order flips every round); reported: the median, min and max over the rounds."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8e12


def _frames(N, H, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = np.maximum(2 + 3 * xx * yy + np.sin(5 * xx) + 0.1 * rs.standard_normal((N, H, W)), 0.3)
    acc = np.clip(1.4 * rs.uniform(size=(N, H, W)) - 0.2, 0, 1).astype(np.float32)
    disp = (1 / depth).astype(np.float32)
    disp[acc == 0] = np.nan
    return disp, acc


def _stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": [float(x) for x in v]}


def _window_ms(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def bench_depthvis(shape, dev, rounds=5):
    import _depthvis_ref as Ref
    from conftest import golden
    from consistentnerf_amd import ops
    N, H, W = shape
    disp, acc = _frames(N, H, W, 0)
    d, a = torch.from_numpy(disp).to(dev), torch.from_numpy(acc).to(dev)
    lut = golden("depthvis")["lut"]

    def hip():
        return ops.depthvis(d, a, want_f32=False)

    def host():
        with np.errstate(all="ignore"):
            return [Ref.to_u8(Ref.visualize(1 / disp[n], acc[n], lut)) for n in range(N)]
    u8 = hip()[1].cpu().numpy()
    ref = np.stack(host())
    differ = float((np.abs(u8.astype(int) - ref).max(-1) > 0).mean())
    for _ in range(20):
        hip()
    torch.cuda.synchronize()
    n_hip = max(20, int(300. / _window_ms(hip, 50)))
    ms = {"hip": [], "numpy": []}
    for r in range(rounds):
        for k in (("hip", "numpy") if r % 2 == 0 else ("numpy", "hip")):
            if k == "hip":
                ms[k].append(_window_ms(hip, n_hip))
            else:
                t = time.perf_counter()
                host()
                ms[k].append((time.perf_counter() - t) * 1e3)
    ib = int(np.ceil(np.log2(H * W)))
    passes = (32 + ib + 3) // 4
    moved = N * H * W * (8 * passes + 4 + 8 + 3)
    out = {"shape": list(shape), "pixels_differing_from_numpy": differ, "calls_per_window": n_hip, "select_passes": passes,
           "launches": passes + 2, "bytes_moved": moved, "hip": _stats(ms["hip"]), "numpy": _stats(ms["numpy"])}
    out["bytes_per_s"] = moved / (out["hip"]["median_ms"] * 1e-3)
    out["of_hbm_peak"] = out["bytes_per_s"] / HBM_BYTES_PER_S
    out["numpy_over_hip"] = out["numpy"]["median_ms"] / out["hip"]["median_ms"]
    return out


def bench_testset(dev, rounds=5):
    import _inputs as I
    import _depthvis_ref as Ref
    import _lpips_ref as LR
    from conftest import golden
    from consistentnerf_amd import io_formats as F, run_nerf_view as V
    from consistentnerf_amd.lpips import LPIPS
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import NeRF, get_embedder, img2mse, mse2psnr
    N, H, W, focal = 4, 378, 504, 420.0

    def model(seed):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in I.nerf_state_dict(8, 256, 10, 4, 5, True, seed).items()})
        return m.to(dev)
    e, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    kw = dict(network_query_fn=lambda i, v, f: run_network(i, v, f, embed_fn=e, embeddirs_fn=ed), perturb=0.0, N_importance=64,
              network_fine=model(22), N_samples=64, network_fn=model(21), white_bkgd=False, raw_noise_std=0.0, lindisp=False, ndc=False,
              near=2.0, far=6.0, use_viewdirs=True)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = [torch.from_numpy(F.pose_spherical(th, -30.0, 4.0)).to(dev) for th in (0.0, 30.0, 60.0, 90.0)]
    rs = np.random.RandomState(3)
    gt = rs.uniform(size=(N, H, W, 3)).astype(np.float32)
    mask = rs.uniform(size=(N, H, W)) > 0.4
    lpips_fn = LPIPS(net="vgg", weights=LR.package_state_dict(LR.make_weights(0))).to(dev)
    lut = golden("depthvis")["lut"]
    hwf = (H, W, focal)

    def new():
        return V.evaluate_testset(poses, hwf, K, 32768, kw, gt, lpips_fn, depth_mask=mask)

    def old():
        rgbs, disps, accs = V.render_path(poses, hwf, K, 32768, kw)
        m = {"psnr": float(mse2psnr(img2mse(torch.Tensor(rgbs), torch.Tensor(gt)))),
             "psnr_mask": float(F.img2psnr_mask(torch.Tensor(rgbs), torch.Tensor(gt), torch.from_numpy(mask).float()))}
        m["ssim"], m["msssim"] = (float(v) for v in F.img2ssim(rgbs, gt))
        m["ssim_mask"], m["msssim_mask"] = (float(v) for v in F.img2ssim(rgbs, gt, mask))
        m["lpips"], m["lpips_mask"] = float(F.img2lpips(rgbs, gt, lpips_fn)), float(F.img2lpips(rgbs, gt, lpips_fn, mask=mask))
        with np.errstate(all="ignore"):
            m["depth_vis_u8"] = np.stack([Ref.to_u8(Ref.visualize(1 / disps[n], accs[n], lut)) for n in range(N)])
        return m

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    sys.stdout, keep = open(os.devnull, "w"), sys.stdout         # render_path prints per frame
    try:
        a, b = new(), old()
        for _ in range(2):
            new(), old()
        ms = {"evaluate_testset": [], "composition": []}
        for r in range(rounds):
            for k in (("evaluate_testset", "composition") if r % 2 == 0 else ("composition", "evaluate_testset")):
                ms[k].append(wall(new if k == "evaluate_testset" else old))

        def events(fn):
            torch.cuda.synchronize()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
            d2h = [n for n in names if "DtoH" in n or "Device -> Host" in n]
            return len(names) - len(d2h), len(d2h)

        def render_only():
            with torch.no_grad():
                for c2w in poses:
                    V.render(H, W, K, chunk=32768, c2w=c2w[:3, :4], **kw)
        k_new, c_new = events(new)
        k_ren, c_ren = events(render_only)
        k_old, c_old = events(old)
    finally:
        sys.stdout = keep
    agree = {k: abs(a[k] - b[k]) for k in ("psnr", "psnr_mask", "ssim", "msssim", "ssim_mask", "msssim_mask", "lpips", "lpips_mask")}
    out = {"frames": [N, H, W], "metric_differences_of_the_arms": agree,
           "evaluate_testset": _stats(ms["evaluate_testset"]), "composition": _stats(ms["composition"]),
           "device_events": {"evaluate_testset": {"launches": k_new, "copies_to_host": c_new}, "render_only": {"launches": k_ren, "copies_to_host": c_ren},
                             "composition": {"launches": k_old, "copies_to_host": c_old},
                             "launches_between_last_render_launch_and_first_copy_to_host": k_new - k_ren}}
    out["composition_over_evaluate_testset"] = out["composition"]["median_ms"] / out["evaluate_testset"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "evalpass_bench needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "depthvis": [bench_depthvis(s, dev) for s in ((4, 378, 504), (1, 756, 1008))],
           "testset": bench_testset(dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
