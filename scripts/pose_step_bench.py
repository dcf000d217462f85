"""The training step with learnable cameras on one MI355X: `python scripts/pose_step_bench.py [--out profiles/pose_step_bench.json]`.

The C2 shape of bench.py — 4096 rays, 64 coarse + 192 fine samples, two D8 / W256 networks with view directions, FusedAdam — with
the rays built from three learnable cameras (CameraPoses + CameraIntrinsics in a torch.optim.Adam, three views of a 378 x 504
image, the pixels of scripts/camera_bench.py).  Four arms, from one tree in one process, each a whole step (rows, forward, backward,
both optimizer steps):
  a_default     render_loss(rows=) on rows built without a graph: the default step, no camera gradient
  b_rows_folded render_loss(rows=) on rows that require grad: the folded route (three pair launches + the two camera launches more)
  c_rows_lines  batchify_rays(rows) + img2mse(rgb) + img2mse(rgb0): the loss as launches of its own; the two levels' MLP backward and
                input-gradient launches pair up on this route as well (_link_levels)
  d_rows_lines_unpaired  the same with run_nerf.MERGE_BWD off: every level on its own, the launch sequence the camera gradients had
                before the levels paired (two dgrad + wgrad passes, the single input-gradient launches, fills and adds)
The arms alternate round by round (the order flips every round) after a warm-up, each timed window is sized to last >= 0.5 s and
ends with a device synchronise; reported: the median milliseconds per step of each arm and the range over the rounds, then the
per-kernel records of ops._timed for one more step of each arm (HIP events around every launch that has a record)."""
import argparse
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, N_VIEWS, H, W = 4096, 3, 378, 504
K0 = [[407.0, 0.0, 252.0], [0.0, 407.0, 189.0], [0.0, 0.0, 1.0]]
N_COARSE, N_IMPORTANCE, NEAR, FAR = 64, 128, 2.125, 4.67      # the fine level evaluates N_COARSE + N_IMPORTANCE = 192 samples
WINDOW_S, WARMUP, PROFILED = 0.5, 20, 5


def _args(tmp):
    return argparse.Namespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=N_IMPORTANCE, netdepth=8, netwidth=256,
                              netdepth_fine=8, netwidth_fine=256, netchunk=1024 * 64, lrate=5e-4, basedir=tmp, expname="pose_step",
                              ft_path=None, no_reload=True, perturb=1.0, N_samples=N_COARSE, white_bkgd=False, raw_noise_std=0.0,
                              dataset_type="dtu", no_ndc=True, lindisp=False)


def _window_ms(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pose_step_bench needs an MI355X"
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.pose import CameraIntrinsics, CameraPoses, camera_rows
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    with tempfile.TemporaryDirectory() as tmp:
        kw, _, _, _, opt = R.create_nerf(_args(tmp))
    g = torch.Generator(device=dev).manual_seed(0)
    rs = np.random.RandomState(0)
    w = torch.from_numpy(rs.uniform(-0.1, 0.1, size=(N_VIEWS, 3)).astype(np.float32)).to(dev)
    t = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(N_VIEWS, 3)).astype(np.float32)).to(dev)
    c2w0 = ops.pose_compose(torch.eye(4, device=dev)[:3].repeat(N_VIEWS, 1, 1).contiguous(), w, t)
    poses = CameraPoses(c2w0).to(dev)
    intr = CameraIntrinsics(torch.tensor(K0), learn_focal=True, learn_center=True, tie_focal=False).to(dev)
    cam_opt = torch.optim.Adam(list(poses.parameters()) + list(intr.parameters()), lr=1e-4)
    coords = torch.stack([torch.randint(0, H, (B,), device=dev, generator=g), torch.randint(0, W, (B,), device=dev, generator=g)], -1)
    view = torch.randint(0, N_VIEWS, (B,), device=dev, generator=g)
    target = torch.rand(B, 3, device=dev, generator=g)

    def rows(grad):
        with torch.set_grad_enabled(grad):
            return camera_rows(H, W, intr(), poses(), coords, view, near=NEAR, far=FAR, use_viewdirs=True, ndc=False)

    def a_default():
        loss = R.render_loss(H, W, K0, target, 32768, rows=rows(False), retraw=True, **kw)[0]
        opt.zero_grad()
        R.backward(loss)
        opt.step()

    def b_rows_folded():
        loss = R.render_loss(H, W, K0, target, 32768, rows=rows(True), retraw=True, **kw)[0]
        opt.zero_grad()
        cam_opt.zero_grad(set_to_none=True)
        R.backward(loss)
        opt.step()
        cam_opt.step()

    def c_rows_lines():
        out = R.batchify_rays(rows(True), 32768, retraw=True, **{k: v for k, v in kw.items() if k not in ("use_viewdirs", "ndc")})
        loss = R.img2mse(out["rgb_map"], target) + R.img2mse(out["rgb0"], target)
        opt.zero_grad()
        cam_opt.zero_grad(set_to_none=True)
        R.backward(loss)
        opt.step()
        cam_opt.step()

    def d_rows_lines_unpaired():
        R.MERGE_BWD = False
        try:
            c_rows_lines()
        finally:
            R.MERGE_BWD = True

    arms = {"a_default": a_default, "b_rows_folded": b_rows_folded, "c_rows_lines": c_rows_lines, "d_rows_lines_unpaired": d_rows_lines_unpaired}
    n = {}
    for k, f in arms.items():
        for _ in range(WARMUP):
            f()
        torch.cuda.synchronize()
        once = min(_window_ms(f, 5) for _ in range(2)) / 5
        n[k] = max(5, math.ceil(1.15 * WINDOW_S * 1e3 / once))
    ms, windows = {k: [] for k in arms}, {k: [] for k in arms}
    for r in range(a.rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            wms = _window_ms(arms[k], n[k])
            windows[k].append(wms)
            ms[k].append(wms / n[k])
    assert min(min(v) for v in windows.values()) >= WINDOW_S * 1e3, windows
    # per-kernel records (HIP events around each launch that ops._timed wraps): the median over PROFILED more steps of each arm
    kernels = {}
    for k, f in arms.items():
        per = {}
        for _ in range(PROFILED):
            ops.PROFILE = []
            f()
            torch.cuda.synchronize()
            step = {}
            for name, units, e0, e1 in ops.PROFILE:
                step.setdefault(name, [0.0, 0])
                step[name][0] += e0.elapsed_time(e1)
                step[name][1] += units
            ops.PROFILE = None
            for name, (t_ms, units) in step.items():
                per.setdefault(name, {"ms": [], "units": units})["ms"].append(t_ms)
        kernels[k] = {name: {"median_ms": float(np.median(v["ms"])), "min_ms": float(min(v["ms"])), "max_ms": float(max(v["ms"])),
                             "units": v["units"]} for name, v in per.items()}
    res = {"device": torch.cuda.get_device_name(0),
           "what": "milliseconds per whole training step (rows, forward, backward, FusedAdam step; b, c and d also the cameras' Adam step)",
           "B": B, "n_views": N_VIEWS, "image": [H, W], "samples_coarse_fine": [N_COARSE, N_COARSE + N_IMPORTANCE], "networks": "2 x D8/W256, view directions",
           "window_s": WINDOW_S, "steps_per_window": n, "rounds": a.rounds}
    for k, v in ms.items():
        res[k] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": v}
    res["b_minus_a_ms"] = res["b_rows_folded"]["median_ms"] - res["a_default"]["median_ms"]
    res["b_minus_c_ms"] = res["b_rows_folded"]["median_ms"] - res["c_rows_lines"]["median_ms"]
    res["b_minus_d_ms"] = res["b_rows_folded"]["median_ms"] - res["d_rows_lines_unpaired"]["median_ms"]
    res["kernels_ms_per_step"] = kernels
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
