"""LPIPS cost on one MI355X: `python scripts/lpips_bench.py [--out profiles/lpips_bench.json] [--only train|eval]`.

Two routes on the same device, same seeded weights, alternated window by window so that clock drift falls on both; every window is
at least 0.5 s of back-to-back calls between two device events, after a warm-up; median / min / max ms per call over the windows.
  aten   what a caller did before the kernels existed: the statement composed from ATen ops in float32 (tests/_lpips_ref.py:
         F.conv2d on MIOpen, F.max_pool2d, autograd for the backward)
  hip    consistentnerf_amd.lpips.LPIPS (csrc/lpips.hip)
Cases: train = forward + backward w.r.t. in0 on [16, 3, 16, 16] (the per-step work of V: 4 patches x 2 levels, with room);
eval = forward on [1, 3, 512, 640] and [1, 3, 800, 800].  Launch counts of one call of each route come from the profiler's kernel
events; TFLOP/s from the shapes (2 x 9 x Cin x Cout per output pixel, forward over both images, input gradient over one)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _lpips_ref as Ref  # noqa: E402


def conv_flops(N, H, W, backward):
    f, h, w = 0, H, W
    for l, (ci, co) in enumerate(Ref.CHANNELS):
        if l in Ref.POOL_BEFORE:
            h, w = h // 2, w // 2
        f += 2 * 9 * ci * co * h * w * (2 * N + (N if backward else 0))
    return f


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                   and "Memset" not in e.name)
    except Exception as e:  # the count is a report, not a measurement the times depend on
        return f"unavailable: {type(e).__name__}"


def compare(routes, rounds=5):
    reps = {}
    for name, fn in routes.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        one = window(fn, 3)
        reps[name] = max(3, int(np.ceil(500.0 / max(one, 1e-3))))
    ms = {name: [] for name in routes}
    order = list(routes)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            ms[name].append(window(routes[name], reps[name]))
    return {name: {"ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "calls_per_window": reps[name],
                   "launches": launches(routes[name])} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("train", "eval"), default=None)
    a = ap.parse_args()
    from consistentnerf_amd.lpips import LPIPS
    dev = torch.device("cuda:0")
    wts = Ref.make_weights(0)
    wd = {k: [t.to(dev) for t in v] for k, v in wts.items()}
    model = LPIPS(net="vgg", weights=Ref.package_state_dict(wts)).to(dev)
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only != "eval":
        shape = (16, 3, 16, 16)
        x0, x1 = (t.to(dev) for t in Ref.images(shape[0], shape[2], shape[3], 1))

        def hip():
            x = x0.clone().requires_grad_()
            model(x, x1).sum().backward()
            return x.grad

        def aten():
            x = x0.clone().requires_grad_()
            Ref.lpips(x, x1, wd)[0].sum().backward()
            return x.grad
        r = compare({"aten": aten, "hip": hip})
        fl = conv_flops(shape[0], shape[2], shape[3], True)
        for v in r.values():
            v["tflops"] = fl / (v["ms"] * 1e-3) / 1e12
        r["shape"], r["what"], r["hip_over_aten"] = list(shape), "forward + backward w.r.t. in0", r["hip"]["ms"] / r["aten"]["ms"]
        res["train"] = r
    if a.only != "train":
        res["eval"] = []
        for shape in ((1, 3, 512, 640), (1, 3, 800, 800)):
            x0, x1 = (t.to(dev) for t in Ref.images(shape[0], shape[2], shape[3], 2))

            def hip():
                with torch.no_grad():
                    return model(x0, x1)

            def aten():
                with torch.no_grad():
                    return Ref.lpips(x0, x1, wd)[0]
            r = compare({"aten": aten, "hip": hip}, rounds=3)
            fl = conv_flops(shape[0], shape[2], shape[3], False)
            for v in r.values():
                v["tflops"] = fl / (v["ms"] * 1e-3) / 1e12
            r["shape"], r["what"], r["hip_over_aten"] = list(shape), "forward", r["hip"]["ms"] / r["aten"]["ms"]
            res["eval"].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
