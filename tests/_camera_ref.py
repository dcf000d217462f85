"""Dtype-generic torch restatement of what csrc/camera_grad.hip computes, for autograd in float64 (and float32 for the bound): from
a pixel to the finished ray row of render()'s batch — get_rays of the pixel (tests/_pose_ref.get_rays_at, H:164-173), the view
direction of the PRE-NDC ray (R:103-110), then ndc_rays with near plane 1 (H:186-202) — differentiable in the poses and in the
camera matrix K, which enters as a [3, 3] tensor of the working dtype.  tests/test_camera_cpu.py holds it to the reference's own
get_rays + ndc_rays (fixture `ndc_grad_tiny`)."""
import numpy as np
import torch

import _pose_ref as P

K1 = [[23.5, 0.0, 13.25], [0.0, 21.75, 8.5], [0.0, 0.0, 1.0]]      # non-centred principal point, fx != fy
H1, W1 = 19, 29


def forward_poses(n, seed):
    """n forward-facing poses [n, 3, 4] float32: [Exp(w) | t] with w ~ U(-0.15, 0.15)^3 and t ~ U(-0.3, 0.3)^3, so that the NDC
    warp's divisions by d_z stay tame (the camera looks down -z; |d_z| >= 0.85 over the test images, asserted by each test)."""
    rs = np.random.RandomState(seed)
    w, t = rs.uniform(-0.15, 0.15, size=(n, 3)), rs.uniform(-0.3, 0.3, size=(n, 3))
    R = P.so3_exp(torch.from_numpy(w)).numpy()
    return np.concatenate([R, t[:, :, None]], -1).astype(np.float32)


def ndc_coefs(H, W, focal):
    """The two coefficients of H:193-199 in focal's dtype (tensor arithmetic; the focal length serves both axes)."""
    return -1. / (W / (2. * focal)), -1. / (H / (2. * focal))


def ndc_warp(o, d, ax, ay):
    """[B, 3] pre-NDC rays -> the NDC pair, near plane 1: the origin slides to the plane z = -1 along the ray, then the projection."""
    t = -(1. + o[:, 2]) / d[:, 2]
    p = o + t[:, None] * d
    o_ndc = torch.stack([ax * p[:, 0] / p[:, 2], ay * p[:, 1] / p[:, 2], 1. + 2. / p[:, 2]], -1)
    d_ndc = torch.stack([ax * (d[:, 0] / d[:, 2] - p[:, 0] / p[:, 2]), ay * (d[:, 1] / d[:, 2] - p[:, 1] / p[:, 2]), -2. / p[:, 2]], -1)
    return o_ndc, d_ndc


def rows(H, W, K, c2w, coords, view=None, near=0., far=1., use_viewdirs=False, ndc=True, coef_paths=True):
    """K [3, 3] and c2w [n_views, 3, 4] (or [3, 4]) tensors of one float dtype, coords [B, 2] int64 (row, col), view [B] int64 or
    None -> rows [B, 8 | 11] = [o, d, near, far (, viewdirs)].  coef_paths=False cuts the graph from K[0][0] to the two NDC
    coefficients (the values stay): what a backward that forgot those paths would compute."""
    o, d = P.get_rays_at(H, W, K, c2w, coords, view)
    cols = []
    if use_viewdirs:
        cols.append(d / torch.norm(d, dim=-1, keepdim=True))
    if ndc:
        ax, ay = ndc_coefs(H, W, K[0][0] if coef_paths else K[0][0].detach())
        o, d = ndc_warp(o, d, ax, ay)
    B = coords.shape[0]
    return torch.cat([o, d, torch.full((B, 1), near, dtype=o.dtype), torch.full((B, 1), far, dtype=o.dtype)] + cols, -1)


def grads(H, W, K, c2w, coords, view, G, use_viewdirs, ndc, dtype, coef_paths=True):
    """Autograd of sum(rows * G) in `dtype` -> (rows, d_c2w [n_views, 12], d_K [3, 3]) as float64 tensors; also min |d_z| of the
    pre-NDC directions."""
    Kt = torch.tensor(K, dtype=dtype).requires_grad_(True) if not torch.is_tensor(K) else K.detach().to(dtype).requires_grad_(True)
    pose = torch.as_tensor(c2w).to(dtype).reshape(-1, 3, 4).requires_grad_(True)
    r = rows(H, W, Kt, pose, coords, view, 0., 1., use_viewdirs, ndc, coef_paths)
    (r * torch.as_tensor(G).to(dtype)).sum().backward()
    return r.detach().double(), pose.grad.double().reshape(-1, 12), Kt.grad.double()


def min_abs_dz(H, W, K, c2w, coords, view):
    _, d = P.get_rays_at(H, W, torch.tensor(K, dtype=torch.float64), torch.as_tensor(c2w).double().reshape(-1, 3, 4), coords, view)
    return float(d[:, 2].abs().min())
