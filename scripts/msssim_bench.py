"""MS-SSIM as a loss on one MI355X: `python scripts/msssim_bench.py [--out profiles/msssim_bench.json]`.

Times `v = ms_ssim(x, Y, data_range=1); dX = grad(v, x)` (forward + backward w.r.t. X) at 4 x 3 x 756 x 1008 and 1 x 3 x 512 x 640:
  hip    consistentnerf_amd.ssim.ms_ssim (cnerf_msssim_fwd / cnerf_msssim_bwd)
  aten   the same statement on ATen in fp32 on the same device (tests/_ssim_ref.py: grouped conv2d, avg_pool2d, autograd)
The two arms alternate round by round (the order flips every round), each timed window is a fixed number of calls sized to last
>= 0.5 s between two device events; reported: the median ms per call of each arm, the spread (min .. max over the rounds) and the
ratio of the medians.  Also the number of device launches of one backward of the hip arm, from the profiler."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((4, 3, 756, 1008), (1, 3, 512, 640))
WINDOW_S = 0.5


def _arms(shape, dev):
    import _ssim_ref as Ref
    from consistentnerf_amd import ssim as S
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(*shape, device=dev, generator=g)
    Y = (X + 0.1 * torch.randn(X.shape, device=dev, generator=g)).clamp(0, 1)
    x = X.clone().requires_grad_()

    def arm(fn):
        def call():
            return torch.autograd.grad(fn(x, Y, data_range=1), (x,))[0]
        return call
    return {"hip": arm(S.ms_ssim), "aten": arm(Ref.ms_ssim)}, (x, Y)


def _window_ms(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_shape(shape, dev, rounds=6):
    arms, _ = _arms(shape, dev)
    # the two arms agree (the figures compare the same computation)
    gh, ga = arms["hip"](), arms["aten"]()
    rel = ((gh - ga).abs().max() / ga.abs().max()).item()
    n = {}
    for k, call in arms.items():
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        # sized for twice the least window from the fastest of three warm windows: the clocks rise while the device stays busy,
        # and a window sized on the first calls came out 10 % short of 0.5 s
        once = min(_window_ms(call, 20) for _ in range(3)) / 20
        n[k] = max(5, math.ceil(2 * WINDOW_S * 1e3 / once))
    ms = {k: [] for k in arms}
    windows = {k: [] for k in arms}
    for r in range(rounds):
        for k in (("hip", "aten") if r % 2 == 0 else ("aten", "hip")):
            w = _window_ms(arms[k], n[k])
            windows[k].append(w)
            ms[k].append(w / n[k])
    assert min(min(v) for v in windows.values()) >= WINDOW_S * 1e3, windows
    out = {"shape": list(shape), "rel_diff_of_the_arms": rel, "calls_per_window": n}
    for k, v in ms.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": v}
    out["aten_over_hip"] = out["aten"]["median_ms"] / out["hip"]["median_ms"]
    return out


def backward_launches(shape, dev):
    """Device launches of one backward (w.r.t. X) of the hip arm: all of them, and this library's own by kernel name."""
    from consistentnerf_amd import ssim as S
    _, (x, Y) = _arms(shape, dev)
    torch.autograd.grad(S.ms_ssim(x, Y, data_range=1), (x,))
    v = S.ms_ssim(x, Y, data_range=1)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        torch.autograd.grad(v, (x,))
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    own = [n for n in names if "ssim_tile_k" in n or "ssim_bwd_k" in n]
    return {"shape": list(shape), "all": len(names), "ssim_kernels": len(own), "names": [n[:96] for n in names]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "msssim_bench needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "what": "ms_ssim forward + backward w.r.t. X, ms per call", "window_s": WINDOW_S,
           "shapes": [time_shape(s, dev) for s in SHAPES], "backward_launches": backward_launches(SHAPES[1], dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
