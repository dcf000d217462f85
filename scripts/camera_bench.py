"""The camera-row route on one MI355X: `python scripts/camera_bench.py [--out profiles/camera_bench.json]`.

From a learnable pose to the ray batch of render() and back, at the training batch (B = 4096 rays drawn over n_views = 3 poses of a
378 x 504 image), forward + backward through autograd of `(rows * G).sum()`-like seeding (rows.backward(G)), between HIP events:
  one_node        pose.camera_rows(host K, ndc=False, use_viewdirs=True): 1 launch forward, 2 backward
  three_node      get_rays_at + the non-NDC pack node (what render(rays=..., ndc=False) builds): 1 + 1 launches forward, 1 + 2 backward
  one_node_ndc_K  pose.camera_rows(device K requiring grad, ndc=True): the route that has no three-node form
one_node and three_node produce the same rows (asserted bit for bit) and the same pose gradient (asserted to 1e-5 of its largest
element: the one-node backward evaluates each ray in fp64).  These are eager steps, enqueued call by call from Python: the time is
mostly the host's (autograd nodes, ctypes calls, allocations), which is what the three nodes cost a training step.
  k_rows / k_rows_bwd   the two C entry points alone, as captured hipGraphs of CALLS calls replayed back to back (kernel time)
The arms alternate round by round (the order flips every round), each timed window is sized to last >= 0.5 s; reported: the median
microseconds per step (or call) of each arm and the spread over the rounds."""
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
    assert torch.cuda.is_available(), "camera_bench needs an MI355X"
    from consistentnerf_amd import _lib, ops
    from consistentnerf_amd.pose import camera_rows
    from consistentnerf_amd.run_nerf import _PackRaysFn
    from consistentnerf_amd.run_nerf_helpers import get_rays_at
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rs = np.random.RandomState(0)
    # forward-facing poses (the NDC arm divides by d_z)
    w = torch.from_numpy(rs.uniform(-0.1, 0.1, size=(N_VIEWS, 3)).astype(np.float32)).to(dev)
    t = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(N_VIEWS, 3)).astype(np.float32)).to(dev)
    c2w0 = torch.eye(4, device=dev)[:3].repeat(N_VIEWS, 1, 1).contiguous()
    c2w = ops.pose_compose(c2w0, w, t).requires_grad_(True)
    Kd = torch.tensor(K, device=dev).requires_grad_(True)
    coords = torch.stack([torch.randint(0, H, (B,), device=dev, generator=g), torch.randint(0, W, (B,), device=dev, generator=g)], -1)
    view = torch.randint(0, N_VIEWS, (B,), device=dev, generator=g)
    G = torch.randn(B, 11, device=dev, generator=g)
    G[:, 6:8] = 0

    def one_node():
        c2w.grad = None
        camera_rows(H, W, K, c2w, coords, view, near=0., far=1., use_viewdirs=True, ndc=False).backward(G)

    def three_node():
        c2w.grad = None
        o, d = get_rays_at(H, W, K, c2w, coords, view)
        _PackRaysFn.apply(o, d, 0., 1., True).backward(G)

    def one_node_ndc_K():
        c2w.grad = Kd.grad = None
        camera_rows(H, W, Kd, c2w, coords, view, near=0., far=1., use_viewdirs=True, ndc=True).backward(G)

    # the two routes agree
    r1 = camera_rows(H, W, K, c2w, coords, view, near=0., far=1., use_viewdirs=True, ndc=False)
    r3 = _PackRaysFn.apply(*get_rays_at(H, W, K, c2w, coords, view), 0., 1., True)
    assert torch.equal(r1, r3), "the two routes build different rows"
    one_node()
    g1 = c2w.grad.clone()
    three_node()
    g3 = c2w.grad.clone()
    agree = float((g1 - g3).abs().max() / g3.abs().max())
    assert agree <= 1e-5, agree

    lib, st, p = _lib.load(), ops._stream, ops._p
    c12 = c2w.detach().reshape(N_VIEWS, 12).contiguous()
    rows = torch.empty(B, 11, device=dev)
    ws = torch.empty(lib.cnerf_camera_rows_bwd_ws_floats(B, N_VIEWS) // 2, device=dev, dtype=torch.float64)
    d_c2w, d_K = torch.empty(N_VIEWS, 12, device=dev), torch.empty(3, 3, device=dev)
    Kc = Kd.detach()
    kernels = {
        "k_rows": lambda: _lib.check(lib.cnerf_camera_rows(H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, p(Kc), p(c12), N_VIEWS, p(coords), p(view), 0, B,
                                                           0.0, 1.0, 1, 1, p(rows), st()), "rows"),
        "k_rows_bwd": lambda: _lib.check(lib.cnerf_camera_rows_bwd(H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, p(Kc), p(c12), N_VIEWS, p(coords), p(view),
                                                                   0, B, 1, 1, p(G), p(d_c2w), p(d_K), p(ws), 0, st()), "rows_bwd"),
    }
    steps = {"one_node": one_node, "three_node": three_node, "one_node_ndc_K": one_node_ndc_K}
    call, n = {}, {}
    side = torch.cuda.Stream()
    for k, f in kernels.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                for _ in range(CALLS):
                    f()
        gr.replay()
        torch.cuda.synchronize()
        call[k] = gr.replay
        once = min(_window_ms(gr.replay, 3) for _ in range(3)) / 3
        n[k] = max(3, math.ceil(2 * WINDOW_S * 1e3 / once))
    for k, f in steps.items():
        for _ in range(200):      # (the first eager steps are slower: allocator, autograd and ctypes warm up)
            f()
        torch.cuda.synchronize()
        call[k] = f
        once = min(_window_ms(f, 200) for _ in range(3)) / 200
        n[k] = max(50, math.ceil(3 * WINDOW_S * 1e3 / once))
    first = d_c2w.clone()
    us, windows = {k: [] for k in call}, {k: [] for k in call}
    for r in range(a.rounds):
        for k in (list(call) if r % 2 == 0 else list(call)[::-1]):
            ms = _window_ms(call[k], n[k])
            windows[k].append(ms)
            us[k].append(1e3 * ms / (n[k] * (CALLS if k in kernels else 1)))
    assert min(min(v) for v in windows.values()) >= WINDOW_S * 1e3, windows
    assert torch.equal(first, d_c2w), "cnerf_camera_rows_bwd is not identical from run to run"
    res = {"device": torch.cuda.get_device_name(0),
           "what": "microseconds per eager forward + backward step (one_node, three_node, one_node_ndc_K) and per C call in a captured graph "
                   "of CALLS calls (k_rows, k_rows_bwd)",
           "B": B, "n_views": N_VIEWS, "image": [H, W], "calls_per_graph": CALLS, "window_s": WINDOW_S, "per_window": n,
           "pose_grad_one_vs_three_node": agree}
    for k, v in us.items():
        res[k] = {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v)), "rounds_us": v}
    res["three_over_one"] = res["three_node"]["median_us"] / res["one_node"]["median_us"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
