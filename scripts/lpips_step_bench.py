#!/usr/bin/env python
"""Times V's full step loss WITH its patch LPIPS term at bench.py's C3 rig (3 analytic 378 x 504 views, 4096 random rays + 4 patches
of 16 x 16, both levels D=8 W=256, 64 + 128 samples, ssim_w = lpips_w = 0.005, clip + Adam), three arms in ONE process:

    lines    the step as the reference's statements: run_nerf_view._render_loss_lines (render, hardmask_losses, midas_patch_loss,
             patch_ssim) + one patch_lpips per level, loss.backward(), Adam — the only route on which the LPIPS term reached the
             networks before render_loss had lpips_w=
    folded   run_nerf_view.render_loss(..., ssim_w=0.005, lpips_w=0.005, lpips_fn=...): one autograd node, one batched LPIPS pass
    default  the same call with lpips_w = 0: what the term costs inside the fold is folded - default

The arms are alternated window by window; a window is >= --window seconds of back-to-back steps between two device events (the
step count is calibrated per arm first).  Reported per arm: the median and the min - max of the windows' ms per step, and the kernel
launches of one step (torch profiler).  The LPIPS weights are seeded random ones of the right shapes (the arithmetic, and so the
time, does not depend on their values).

    python scripts/lpips_step_bench.py [--rounds 7] [--window 0.5] [--out profiles/lpips_step_bench.json]
    python scripts/lpips_step_bench.py --default-only --root <checkout>     # the default step of another checkout of this package
"""
import argparse
import json
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=None)
ap.add_argument("--default-only", action="store_true", help="time only the default step, called without the LPIPS arguments")
ap.add_argument("--root", default=None, help="the checkout whose package and bench.py to time (default: this one)")
args = ap.parse_args()

ROOT = os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from consistentnerf_amd import lpips as L, raybank as RB, run_nerf as R, run_nerf_view as V  # noqa: E402


def seeded_lpips(dev):
    g = torch.Generator().manual_seed(0)
    sd = {}
    for name, (shape, keys) in L.KEY_TABLE.items():
        if name.startswith("lin"):
            t = torch.rand(shape, generator=g) * (4.0 / shape[1])
        elif name.endswith("weight"):
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / (9 * shape[1]))
        else:
            t = torch.randn(shape, generator=g) * 0.05
        sd[keys[0]] = t
    return L.LPIPS(net="vgg", weights=sd).to(dev)


def make_step(sc, arm, lpips_fn):
    H, W, K, far, kw, opt = sc["H"], sc["W"], sc["K"], sc["far"], sc["kw"], sc["opt"]

    def step(i):
        v = i % 3
        starts = RB.draw_patch_starts(H, W, 4, 16)
        rays, target, sel, (d_prior, m, mono_s) = RB.sample_patch_rays(
            sc["img_t"][v], sc["poses"][v], H, W, K, 4096, starts, extras=(sc["dep_t"][v], sc["msk_t"][v], sc["mono_t"][v]),
            render_kwargs=kw)
        if arm == "lines":
            loss = V._render_loss_lines(H, W, K, target, m, d_prior, 32768, rays, 0.2, far, 1.0, 0.1, mono_s, 4, 16, 0.001, None,
                                        dict(kw, retraw=True), ssim_w=0.005, ssim_patches=4, lpips_w=0.005, lpips_fn=lpips_fn)[0]
            opt.zero_grad()
            loss.backward()
        else:
            extra = dict(lpips_w=0.005 if arm == "folded" else 0.0, lpips_fn=lpips_fn) if arm != "default_plain" else {}
            loss = V.render_loss(H, W, K, target, mask=m, depth_prior=d_prior, chunk=32768, rays=rays, hardmask_coef=0.2, depth_w=0.1,
                                 mono=mono_s, patch_num=4, patch_size=16, patch_w=0.001, ssim_w=0.005, retraw=True, **extra, **kw)[0]
            opt.zero_grad()
            R.backward(loss)
        opt.step()
        return loss
    return step


def window(step, n, i0):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        step(i0 + i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def launches(step):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step(0)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    dev = torch.device("cuda:0")
    sc = bench.c3_scene(dev)
    lp = None if args.default_only else seeded_lpips(dev)
    arms = ["default_plain"] if args.default_only else ["lines", "folded", "default"]
    steps = {a: make_step(sc, a, lp) for a in arms}
    n, it = {}, 0
    for a in arms:                                        # warm-up, then the step count of a window
        for _ in range(5):
            steps[a](it)
            it += 1
        torch.cuda.synchronize()
        ms = window(steps[a], 10, it)
        it += 10
        n[a] = max(5, int(math.ceil(args.window * 1e3 / ms * 1.1)))
    ms = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a in arms:
            ms[a].append(window(steps[a], n[a], it))
            it += n[a]
    out = {"rig": "bench.py C3: 378x504 views, 4096 random + 4 x 256 patch rays, D=8 W=256, 64+128 samples, ssim_w = lpips_w = 0.005, "
                  "clip 0.1 + Adam; sampling launch included",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "checkout": "another (--root)" if args.root else "this one", "arms": {}}
    for a in arms:
        out["arms"][a] = {"ms_per_step_median": round(statistics.median(ms[a]), 4), "ms_per_step_min": round(min(ms[a]), 4),
                          "ms_per_step_max": round(max(ms[a]), 4), "steps_per_window": n[a], "windows_ms": [round(x, 4) for x in ms[a]],
                          "launches_per_step": launches(steps[a])}
    if not args.default_only:
        A = out["arms"]
        out["lpips_term_cost_ms_folded"] = round(A["folded"]["ms_per_step_median"] - A["default"]["ms_per_step_median"], 4)
        out["lpips_term_cost_ms_lines"] = round(A["lines"]["ms_per_step_median"] - A["default"]["ms_per_step_median"], 4)
        out["lines_over_folded"] = round(A["lines"]["ms_per_step_median"] / A["folded"]["ms_per_step_median"], 4)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
