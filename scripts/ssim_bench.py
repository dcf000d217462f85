"""SSIM cost on one MI355X: `python scripts/ssim_bench.py [--out profiles/ssim_bench.json] [--only c3|img]`.

  c3   the C3 training step of bench.py's rig (c3_scene: 378 x 504 views, 4096 rays, 4 patches, both levels, FusedAdam) with
       render_loss(ssim_w=0) and render_loss(ssim_w=0.005) — the same batches, the two arms interleaved round by round so that
       clock / thermal drift falls on both; median ms per step of each.
  img  io_formats.img2ssim (HIP: SSIM + MS-SSIM) on 4 x 756 x 1008 x 3 images against the same statement on ATen in fp32
       (tests/_ssim_ref.py: grouped conv2d, avg_pool2d) on the same device; median ms per call.
`--only c3 [--ssim-w W]` runs a few steps of one arm and nothing else (for a `rocprofv3 --kernel-trace --stats` pass)."""
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


def c3_arm(sc, ssim_w):
    from consistentnerf_amd import raybank as RB, run_nerf as R, run_nerf_view as V
    H, W, K, kw, opt = sc["H"], sc["W"], sc["K"], sc["kw"], sc["opt"]

    def step(i):
        v = i % 3
        starts = RB.draw_patch_starts(H, W, 4, 16)
        rays, target, sel, (d_prior, m, mono_s) = RB.sample_patch_rays(
            sc["img_t"][v], sc["poses"][v], H, W, K, 4096, starts, extras=(sc["dep_t"][v], sc["msk_t"][v], sc["mono_t"][v]),
            render_kwargs=kw)
        loss = V.render_loss(H, W, K, target, mask=m, depth_prior=d_prior, chunk=32768, rays=rays, hardmask_coef=0.2, depth_w=0.1,
                             mono=mono_s, patch_num=4, patch_size=16, patch_w=0.001, ssim_w=ssim_w, retraw=True, **kw)[0]
        opt.zero_grad()
        R.backward(loss)
        opt.step()
        return loss
    return step


def time_c3(dev, rounds=8, steps=10):
    import bench
    sc = bench.c3_scene(dev)
    arms = {w: c3_arm(sc, w) for w in (0.0, 0.005)}
    for w, st in arms.items():
        for i in range(3):
            st(i)
    torch.cuda.synchronize()
    ms = {w: [] for w in arms}
    for r in range(rounds):
        for w in ((0.0, 0.005) if r % 2 == 0 else (0.005, 0.0)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                arms[w](i)
            torch.cuda.synchronize()
            ms[w].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {w: float(np.median(v)) for w, v in ms.items()}
    return {"ms_per_step_ssim_w_0": med[0.0], "ms_per_step_ssim_w_0.005": med[0.005],
            "rel_cost": med[0.005] / med[0.0] - 1.0, "rounds_ms": {str(w): v for w, v in ms.items()}, "steps_per_round": steps}


def time_img(dev, reps=10):
    import _ssim_ref as Ref
    from consistentnerf_amd import io_formats as F
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(4, 756, 1008, 3, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(x.shape, device=dev, generator=g)).clamp(0, 1)

    def med(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))
    hip = med(lambda: F.img2ssim(x, y))
    with torch.no_grad():
        aten = med(lambda: Ref.img2ssim(x, y))
    return {"img2ssim_hip_ms": hip, "img2ssim_aten_fp32_ms": aten, "speedup": aten / hip, "shape": [4, 756, 1008, 3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("c3", "img"), default=None)
    ap.add_argument("--ssim-w", type=float, default=0.005, help="--only c3: the arm to run")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.only == "c3":
        import bench
        st = c3_arm(bench.c3_scene(dev), a.ssim_w)
        for i in range(6):
            st(i)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only != "img":
        res["c3"] = time_c3(dev)
    res["img2ssim"] = time_img(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
