#!/usr/bin/env python3
"""Frame time of `render_path` at 756x1008 (the C5 leg's frame: NDC, 64 + 128 samples, D=8 W=256, chunk 32768, D2H included) in
the exact-fp32 path and the opt-in reduced-precision modes, one process, modes interleaved over REPS rounds; PSNR of each mode's
frame against the fp32 frame.  usage: python scripts/fp16x2_frame.py [reps]"""
import contextlib
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import bench  # noqa: E402
from consistentnerf_amd import io_formats as F, run_nerf as R  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
MODES = ("fp32", "bf16x2", "bf16x3", "fp16x2")


def main():
    dev = torch.device("cuda:0")
    H, W = 756, 1008
    poses, _, render_poses, _ = F.llff_poses(bench.llff_rig(6), (H, W), factor=4, n_render=60)
    focal = float(poses[0, 2, 4])
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]], dtype=np.float32)
    a = bench.make_args(tempfile.mkdtemp())
    a.dataset_type, a.no_ndc, a.raw_noise_std = "llff", False, 1.0
    torch.manual_seed(0)
    _, kw, *_ = R.create_nerf(a)
    kw.update(near=0.0, far=1.0)
    nets = [kw["network_fn"], kw["network_fine"]]
    rp = torch.from_numpy(render_poses[[15]]).to(dev)
    times, frames = {m: [] for m in MODES}, {}
    try:
        with torch.no_grad(), contextlib.redirect_stdout(sys.stderr):
            for rep in range(REPS + 1):                  # round 0 warms every mode up
                for mode in MODES:
                    for n in nets:
                        n.inference_precision = mode
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rgbs, _ = R.render_path(rp, (H, W, focal), K, 32768, kw)
                    torch.cuda.synchronize()
                    if rep:
                        times[mode].append(time.perf_counter() - t0)
                    frames[mode] = np.asarray(rgbs[0], dtype=np.float64)
    finally:
        for n in nets:
            n.inference_precision = "fp32"
    for mode in MODES:
        mse = float(np.mean((frames[mode] - frames["fp32"]) ** 2))
        psnr = "identical" if mse == 0 else f"{-10 * np.log10(mse):.1f} dB"
        t = float(np.median(times[mode]))
        print(f"frame 756x1008 {mode:7s} {t:6.3f} s (median of {REPS}: {' '.join(f'{x:.3f}' for x in times[mode])})  "
              f"{t / float(np.median(times['bf16x3'])):5.2f}x the bf16x3 frame  PSNR vs the fp32 frame: {psnr}", flush=True)


if __name__ == "__main__":
    main()
