#!/usr/bin/env python3
"""The host side of one eager C3 step (bench.c3_step_fn on bench.c3_scene): wall time per step, the Python time to issue a step, and
wall time minus the kernel time torch.profiler records, over 50 steps.  Prints one JSON line.
usage: python scripts/c3_host_time.py"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import bench  # noqa: E402

N = 50
dev = torch.device("cuda:0")
sc = bench.c3_scene(dev)
step = bench.c3_step_fn(sc)
for i in range(10):
    step(i)
torch.cuda.synchronize()
out = {}
for rep in range(3):
    t0 = time.perf_counter()
    for i in range(N):
        step(10 + i)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    out.setdefault("wall_ms", []).append(1e3 * (time.perf_counter() - t0) / N)
    out.setdefault("enqueue_ms", []).append(1e3 * t_enq / N)
with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
    for i in range(N):
        step(10 + i)
    torch.cuda.synchronize()
dev_us = sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in prof.events()
             if e.device_type == torch.autograd.DeviceType.CUDA)
out["device_ms"] = dev_us / 1e3 / N
out["host_ms"] = [w - out["device_ms"] for w in out["wall_ms"]]
print(json.dumps(out))
