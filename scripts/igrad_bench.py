"""The input-gradient kernel on one MI355X: `python scripts/igrad_bench.py [--out profiles/igrad_bench.json]`.

Times, at the C2 fine level (4096 rays x 192 samples = 786 432 points, D8/W256, view directions, skip layer), between HIP events:
  dgrad   cnerf_mlp_dgrad of the level (the launch the new kernel runs behind; unchanged by it)
  igrad   cnerf_mlp_input_grad on the workspace that dgrad wrote (d_pts and d_dirs_pt)
  rays    cnerf_rays_input_grad on its outputs (d_o, d_d, d_viewdirs per ray)
The arms alternate round by round (the order flips every round), each timed window is a fixed number of calls sized to last >= 0.5 s;
reported: the median ms per call of each arm, the spread over the rounds, and igrad / dgrad.  By MFMA count the new kernel issues
576 of the dgrad's ~8 700 v_mfma_f32_32x32x2_f32 per 32-point tile (6.6 %)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, S = 4096, 192
WINDOW_S = 0.5


def _window_ms(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "igrad_bench needs an MI355X"
    from consistentnerf_amd import _lib, ops
    from consistentnerf_amd.run_nerf import _packed
    from consistentnerf_amd.run_nerf_helpers import NeRF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True).to(dev)
    spec, packed, net = model.spec(), _packed(model), model.spec().c()
    g = torch.Generator(device=dev).manual_seed(0)
    pts = torch.rand(B * S, 3, device=dev, generator=g) * 6 - 3
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=g), dim=-1)
    z = torch.rand(B, S, device=dev, generator=g) * 4 + 2
    raw, stash = ops.mlp_forward(spec, packed, B, S, pts=pts, dirs=dirs, want_stash=True)
    d_raw = torch.randn(B * S, 4, device=dev, generator=g)
    ws = ops.mlp_bwd_workspace(spec, B, S, dev)
    d_pts, d_dirs = torch.empty(B * S, 3, device=dev), torch.empty(B * S, 3, device=dev)
    g_rays = torch.zeros(B, 11, device=dev)
    lib, st, p = _lib.load(), ops._stream, ops._p
    arms = {
        "dgrad": lambda: _lib.check(lib.cnerf_mlp_dgrad(C.byref(net), p(packed), p(d_raw), B, S, p(stash), p(ws), st()), "dgrad"),
        "igrad": lambda: _lib.check(lib.cnerf_mlp_input_grad(C.byref(net), p(packed), B, S, p(stash), p(ws), p(d_pts), p(d_dirs), st()),
                                    "igrad"),
        "rays": lambda: _lib.check(lib.cnerf_rays_input_grad(p(d_pts), p(d_dirs), p(z), B, S, p(g_rays), p(g_rays[:, 3:]),
                                                             p(g_rays[:, 8:]), 11, st()), "rays"),
    }
    n = {}
    for k, call in arms.items():        # (dgrad first: the other two read what it writes)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        once = min(_window_ms(call, 5) for _ in range(3)) / 5
        n[k] = max(5, math.ceil(2 * WINDOW_S * 1e3 / once))
    first = d_pts.clone()
    ms, windows = {k: [] for k in arms}, {k: [] for k in arms}
    for r in range(a.rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            w = _window_ms(arms[k], n[k])
            windows[k].append(w)
            ms[k].append(w / n[k])
    assert min(min(v) for v in windows.values()) >= WINDOW_S * 1e3, windows
    assert torch.equal(first, d_pts), "cnerf_mlp_input_grad is not identical from run to run"
    res = {"device": torch.cuda.get_device_name(0), "what": "ms per call at the C2 fine level", "points": B * S, "net": "D8/W256, view directions",
           "window_s": WINDOW_S, "calls_per_window": n}
    for k, v in ms.items():
        res[k] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": v}
    res["igrad_over_dgrad"] = res["igrad"]["median_ms"] / res["dgrad"]["median_ms"]
    res["mfma_count_ratio"] = 576 / 8704
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
