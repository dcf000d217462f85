#!/usr/bin/env python3
"""Golden-vector generator for the camera pose gradient. Runs ONLY in the build container (needs the reference checkout), in the
manner of make_golden.py / make_golden_lossforms.py: the reference's own run_nerf_helpers is imported and its get_rays (H:164-173) is
called with a pose that requires grad, on a 5 x 7 camera with a non-centred principal point and fx != fy; a fixed random upstream
gradient (G_o, G_d) is pushed back through it. Once in float32 and once with float64 as the default dtype (the reference's linspace
pixel grid then is float64 too: the whole function in float64). The *outputs* (arrays only) go to pose_grad_tiny.npz next to this
file. No reference source, bytecode or pickled object is written.

usage:  python tests/golden/make_golden_pose.py
"""
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from make_golden_lossforms import REF  # noqa: E402  (where the reference checkout lies)

H_IMG, W_IMG = 5, 7
K = [[6.5, 0.0, 3.25], [0.0, 5.75, 2.75], [0.0, 0.0, 1.0]]


def inputs():
    rs = np.random.RandomState(57)
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    c2w = np.concatenate([q, rs.uniform(-2, 2, size=(3, 1))], 1).astype(np.float32)
    G_o = rs.normal(size=(H_IMG, W_IMG, 3)).astype(np.float32)
    G_d = rs.normal(size=(H_IMG, W_IMG, 3)).astype(np.float32)
    return c2w, G_o, G_d


def run(H, c2w, G_o, G_d, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        pose = torch.from_numpy(c2w).to(dtype).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (meshgrid without indexing=)
            rays_o, rays_d = H.get_rays(H_IMG, W_IMG, K, pose)
        assert rays_o.dtype == dtype and rays_d.dtype == dtype
        ((rays_o * torch.from_numpy(G_o).to(dtype)).sum() + (rays_d * torch.from_numpy(G_d).to(dtype)).sum()).backward()
        return rays_o.detach().numpy().copy(), rays_d.detach().numpy(), pose.grad.numpy()
    finally:
        torch.set_default_dtype(old)


def main():
    sys.path.insert(0, REF)
    import run_nerf_helpers as H
    c2w, G_o, G_d = inputs()
    out = dict(c2w=c2w, K=np.asarray(K, np.float64), G_o=G_o, G_d=G_d)
    out["rays_o"], out["rays_d"], out["d_c2w"] = run(H, c2w, G_o, G_d, torch.float32)
    out["rays_o64"], out["rays_d64"], out["d_c2w64"] = run(H, c2w, G_o, G_d, torch.float64)
    assert out["d_c2w"].dtype == np.float32 and out["d_c2w64"].dtype == np.float64 and out["d_c2w"].shape == (3, 4)
    path = os.path.join(HERE, "pose_grad_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote pose_grad_tiny.npz ({os.path.getsize(path) / 1024:.1f} KiB), {len(out)} arrays")


if __name__ == "__main__":
    main()
