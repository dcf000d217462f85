"""Dtype-generic torch restatement of what csrc/rays_grad.hip computes, for autograd in float64 (and float32 for the bound):
get_rays_at = the text of oracle.nerf_oracle.get_rays (H:164-173) indexed by coords / view, and the pose composition
c2w = [Exp(rot) R0 | t0 + trans] with Rodrigues' formula in CLOSED form (the series only at theta = 0 exactly, where the closed form
is 0 / 0: float64 needs no small-angle care above that for the angles the tests use, >= 1e-6)."""
import torch


def pixel_coords(H, W, first=0, B=None):
    """[B, 2] (row, col) of the row-major pixels first .. first + B - 1."""
    idx = torch.arange(first, first + (H * W - first if B is None else B))
    return torch.stack([idx // W, idx % W], -1)


def get_rays_at(H, W, K, c2w, coords, view=None):
    """c2w [n_views, 3, 4] (or [3, 4]) in any float dtype, coords [B, 2] int64 (row, col), view [B] int64 or None (view 0) ->
    (rays_o [B, 3], rays_d [B, 3]).  The intrinsics enter in c2w's dtype, like the Python scalars of the reference."""
    c2w = c2w[None] if c2w.dim() == 2 else c2w
    dt = c2w.dtype
    jj, ii = coords[:, 0].to(dt), coords[:, 1].to(dt)
    dirs = torch.stack([(ii - K[0][2]) / K[0][0], -(jj - K[1][2]) / K[1][1], -torch.ones_like(ii)], dim=-1)      # H:167
    pose = c2w[torch.zeros(coords.shape[0], dtype=torch.int64) if view is None else view]                          # [B, 3, 4]
    rays_d = torch.sum(dirs[..., None, :] * pose[:, :3, :3], dim=-1)                                               # H:170
    rays_o = pose[:, :3, -1]                                                                                        # H:172
    return rays_o, rays_d


def hat(w):
    """[N, 3] -> the cross-product matrices [N, 3, 3]."""
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def so3_exp(w):
    """Rodrigues: Exp(w) = I + sin(t) / t K + (1 - cos t) / t^2 K^2, t = |w|, K = hat(w), per row of w [N, 3], with
    (1 - cos t) / t^2 written as (sin(t / 2) / (t / 2))^2 / 2 (the same function without the cancellation).  A row that is zero
    exactly takes the leading series terms instead (A = 1 - t^2 / 6, B = 1 / 2 - t^2 / 24: the right value AND first derivative at 0)."""
    t2 = (w * w).sum(-1)
    zero = t2 == 0
    t = torch.sqrt(torch.where(zero, torch.ones_like(t2), t2))
    A = torch.where(zero, 1 - t2 / 6, torch.sin(t) / t)
    B = torch.where(zero, 0.5 - t2 / 24, 0.5 * (torch.sin(t / 2) / (t / 2)) ** 2)
    K = hat(w)
    return torch.eye(3, dtype=w.dtype) + A[:, None, None] * K + B[:, None, None] * (K @ K)


def pose_compose(c2w0, rot, trans):
    """c2w0 [N, 3, 4], rot, trans [N, 3] -> [N, 3, 4]."""
    return torch.cat([so3_exp(rot) @ c2w0[:, :, :3], (c2w0[:, :, 3] + trans)[:, :, None]], -1)
