#!/usr/bin/env python3
"""Golden-vector generator for the NDC and intrinsics gradients. Runs ONLY in the build container (needs the reference checkout), in
the manner of make_golden_pose.py: the reference's own run_nerf_helpers is imported and its get_rays (H:164-173) and ndc_rays
(H:186-202, near plane 1) are called with a pose AND a camera matrix K that are tensors requiring grad — K[0][0] is the `focal` of
ndc_rays, as render() passes it (R:116) — on a 5 x 7 forward-facing camera with a non-centred principal point and fx != fy. The view
directions are those of the pre-NDC rays_d (R:103-110). A fixed random upstream gradient (G_o, G_d, G_v) is pushed back through the
NDC origins, the NDC directions and the view directions. Once in float32 and once with float64 as the default dtype. The *outputs*
(arrays only) go to ndc_grad_tiny.npz next to this file. No reference source, bytecode or pickled object is written.

usage:  python tests/golden/make_golden_ndc.py
"""
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from make_golden_lossforms import REF  # noqa: E402  (where the reference checkout lies)

H_IMG, W_IMG = 5, 7
K = [[6.5, 0.0, 3.25], [0.0, 5.75, 2.75], [0.0, 0.0, 1.0]]


def inputs():
    import _camera_ref as CR
    rs = np.random.RandomState(61)
    c2w = CR.forward_poses(1, 61)[0]
    G = [rs.normal(size=(H_IMG, W_IMG, 3)).astype(np.float32) for _ in range(3)]
    return c2w, G


def run(H, c2w, G, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        pose = torch.from_numpy(c2w).to(dtype).requires_grad_(True)
        Kt = torch.tensor(K, dtype=dtype).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (meshgrid without indexing=)
            rays_o, rays_d = H.get_rays(H_IMG, W_IMG, Kt, pose)
        viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
        o_ndc, d_ndc = H.ndc_rays(H_IMG, W_IMG, Kt[0][0], 1., rays_o, rays_d)
        assert o_ndc.dtype == dtype and d_ndc.dtype == dtype and viewdirs.dtype == dtype
        G_o, G_d, G_v = (torch.from_numpy(g).to(dtype) for g in G)
        ((o_ndc * G_o).sum() + (d_ndc * G_d).sum() + (viewdirs * G_v).sum()).backward()
        rows = torch.cat([o_ndc, d_ndc, viewdirs], -1).reshape(-1, 9)
        return rows.detach().numpy().copy(), pose.grad.numpy().copy(), Kt.grad.numpy().copy(), float(rays_d.detach()[..., 2].abs().min())
    finally:
        torch.set_default_dtype(old)


def main():
    sys.path.insert(0, REF)
    import run_nerf_helpers as H
    c2w, G = inputs()
    out = dict(c2w=c2w, K=np.asarray(K, np.float64), G_o=G[0], G_d=G[1], G_v=G[2])
    out["rows"], out["d_c2w"], out["d_K"], dz = run(H, c2w, G, torch.float32)
    out["rows64"], out["d_c2w64"], out["d_K64"], _ = run(H, c2w, G, torch.float64)
    assert out["rows"].dtype == np.float32 and out["rows64"].dtype == np.float64 and out["rows"].shape == (35, 9)
    assert out["d_c2w"].shape == (3, 4) and out["d_K"].shape == (3, 3) and dz >= 0.85, dz
    path = os.path.join(HERE, "ndc_grad_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote ndc_grad_tiny.npz ({os.path.getsize(path) / 1024:.1f} KiB), {len(out)} arrays; min |d_z| = {dz:.3f}")


if __name__ == "__main__":
    main()
