"""The camera pose kernels on one MI355X: `python scripts/pose_bench.py [--out profiles/pose_bench.json]`.

Times, at the training batch (B = 4096 rays drawn over n_views = 3 poses of a 378 x 504 image), between HIP events:
  compose       cnerf_pose_compose of the 3 poses
  rays_at       cnerf_gen_rays_at (coords + view)
  rays_at_bwd   cnerf_gen_rays_at_bwd (two launches: the chunk sums and the per-view reduction)
  compose_bwd   cnerf_pose_compose_bwd
Each arm is a captured hipGraph of CALLS calls replayed back to back (a kernel of a few microseconds launched call by call from
Python measures the enqueue, not the kernel); `stream_us` is the same call enqueued call by call, for comparison.  The arms alternate
round by round (the order flips every round), each timed window is sized to last >= 0.5 s; reported: the median microseconds per call
of each arm and the spread over the rounds."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, N_VIEWS, H, W = 4096, 3, 378, 504
K = [[407.0, 0.0, 252.0], [0.0, 407.0, 189.0], [0.0, 0.0, 1.0]]
CALLS = 200
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
    assert torch.cuda.is_available(), "pose_bench needs an MI355X"
    from consistentnerf_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    c2w0 = torch.eye(4, device=dev)[:3].repeat(N_VIEWS, 1, 1).contiguous()
    rot, trans = 0.05 * torch.randn(N_VIEWS, 3, device=dev, generator=g), 0.1 * torch.randn(N_VIEWS, 3, device=dev, generator=g)
    coords = torch.stack([torch.randint(0, H, (B,), device=dev, generator=g), torch.randint(0, W, (B,), device=dev, generator=g)], -1)
    view = torch.randint(0, N_VIEWS, (B,), device=dev, generator=g)
    c2w, o, d = torch.empty(N_VIEWS, 12, device=dev), torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
    g_o, g_d = torch.randn(B, 3, device=dev, generator=g), torch.randn(B, 3, device=dev, generator=g)
    lib, st, p = _lib.load(), ops._stream, ops._p
    ws = torch.empty(lib.cnerf_gen_rays_at_bwd_ws_floats(B, N_VIEWS) // 2, device=dev, dtype=torch.float64)
    d_c2w, d_rot, d_trans = torch.empty(N_VIEWS, 12, device=dev), torch.empty(N_VIEWS, 3, device=dev), torch.empty(N_VIEWS, 3, device=dev)
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    arms = {
        "compose": lambda: _lib.check(lib.cnerf_pose_compose(p(c2w0), p(rot), p(trans), N_VIEWS, p(c2w), st()), "compose"),
        "rays_at": lambda: _lib.check(lib.cnerf_gen_rays_at(H, W, fx, fy, cx, cy, p(c2w), N_VIEWS, p(coords), p(view), 0, B, p(o), p(d), st()),
                                      "rays_at"),
        "rays_at_bwd": lambda: _lib.check(lib.cnerf_gen_rays_at_bwd(H, W, fx, fy, cx, cy, p(g_o), p(g_d), N_VIEWS, p(coords), p(view), 0, B,
                                                                     p(d_c2w), p(ws), 0, st()), "rays_at_bwd"),
        "compose_bwd": lambda: _lib.check(lib.cnerf_pose_compose_bwd(p(c2w0), p(rot), p(d_c2w), N_VIEWS, p(d_rot), p(d_trans), st()),
                                          "compose_bwd"),
    }
    graphs, n, n_stream = {}, {}, {}
    side = torch.cuda.Stream()
    for k, call in arms.items():        # (in data order: each arm reads what the one before wrote)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                for _ in range(CALLS):
                    call()
        graphs[k] = gr
        gr.replay()
        torch.cuda.synchronize()
        once = min(_window_ms(gr.replay, 3) for _ in range(3)) / 3
        n[k] = max(3, math.ceil(2 * WINDOW_S * 1e3 / once))
        once = min(_window_ms(call, 50) for _ in range(3)) / 50
        n_stream[k] = max(50, math.ceil(2 * WINDOW_S * 1e3 / once))
    first = d_c2w.clone()
    us, windows, us_stream = {k: [] for k in arms}, {k: [] for k in arms}, {k: [] for k in arms}
    for r in range(a.rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            w = _window_ms(graphs[k].replay, n[k])
            windows[k].append(w)
            us[k].append(1e3 * w / (n[k] * CALLS))
            us_stream[k].append(1e3 * _window_ms(arms[k], n_stream[k]) / n_stream[k])
    assert min(min(v) for v in windows.values()) >= WINDOW_S * 1e3, windows
    assert torch.equal(first, d_c2w), "cnerf_gen_rays_at_bwd is not identical from run to run"
    res = {"device": torch.cuda.get_device_name(0), "what": "microseconds per call, a captured graph of CALLS calls replayed", "B": B,
           "n_views": N_VIEWS, "image": [H, W], "calls_per_graph": CALLS, "window_s": WINDOW_S, "replays_per_window": n}
    for k, v in us.items():
        res[k] = {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v)), "rounds_us": v,
                  "stream_us": float(np.median(us_stream[k]))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
