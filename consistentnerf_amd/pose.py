"""Learnable camera poses: c2w[n] = [Exp(rot[n]) R0_n | t0_n + trans[n]] around fixed initial poses, with the rotation update in
axis-angle form so that a refined pose stays a rigid motion (optimising the twelve floats of c2w directly lets the rotation drift off
SO(3)).  The reference optimises no pose; this is the small parametrisation pose-refining NeRF trainers use.

    poses = CameraPoses(c2w0)                                   # [N,3,4] or [N,4,4]
    opt = torch.optim.Adam(list(net.parameters()) + list(poses.parameters()))      # (or optim.FusedAdam)
    o, d = get_rays_at(H, W, K, poses(), coords, view)          # the rays of the batch's pixels, from the device poses
    rgb, *_ = render(H, W, K, rays=(o, d), ndc=False, **kw)
    img2mse(rgb, target).backward()                             # poses.rot.grad, poses.trans.grad

Value and gradient are one HIP launch each for all views (csrc/rays_grad.hip: cnerf_pose_compose[_bwd]); both are exact at rot = 0,
where the parameters start, and lose no digits for small angles.

With the NDC warp (forward-facing scenes, the reference's default) and / or a learnable camera matrix the batch is built one level
lower, as the rows render() would hand to batchify_rays (csrc/camera_grad.hip: one node over the poses and K):

    intr = CameraIntrinsics(K)                                  # fx = fx0 exp(s), cx = cx0 + c: starts at K
    rows = camera_rows(H, W, intr(), poses(), coords, view, near=0., far=1., use_viewdirs=True, ndc=True)
    out = batchify_rays(rows, chunk, **render_kwargs_train)
    img2mse(out['rgb_map'], target).backward()                  # poses.rot.grad, poses.trans.grad, intr.log_focal.grad"""
import torch
import torch.nn as nn

from . import ops


class _ComposeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c2w0, rot, trans):
        ctx.save_for_backward(c2w0, rot)
        return ops.pose_compose(c2w0, rot.detach(), trans.detach())

    @staticmethod
    def backward(ctx, g):
        c2w0, rot = ctx.saved_tensors
        d_rot, d_trans = ops.pose_compose_bwd(c2w0, rot.detach(), g, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return None, d_rot, d_trans


class CameraPoses(nn.Module):
    """N camera-to-world poses around the fixed `c2w0` ([N,3,4] or [N,4,4]: the top three rows are kept as the buffer `c2w0`).
    Parameters `rot` (axis-angle) and `trans`, both [N,3] and zero: forward() starts at c2w0, bit for bit.  learn_rot / learn_trans
    = False freezes one of them."""

    def __init__(self, c2w0, learn_rot=True, learn_trans=True):
        super().__init__()
        c2w0 = torch.as_tensor(c2w0, dtype=torch.float32)
        if c2w0.dim() != 3 or c2w0.shape[0] < 1 or c2w0.shape[1] not in (3, 4) or c2w0.shape[2] != 4:
            raise ValueError(f"c2w0 must be [N,3,4] or [N,4,4], got {tuple(c2w0.shape)}")
        self.register_buffer("c2w0", c2w0[:, :3, :4].detach().clone().contiguous())
        n = c2w0.shape[0]
        self.rot = nn.Parameter(torch.zeros(n, 3, device=c2w0.device), requires_grad=bool(learn_rot))
        self.trans = nn.Parameter(torch.zeros(n, 3, device=c2w0.device), requires_grad=bool(learn_trans))

    def forward(self):
        """-> c2w [N,3,4], one autograd node over both parameters."""
        return _ComposeFn.apply(self.c2w0, self.rot, self.trans)

    def c2w(self, i):
        """The pose of view i, [3,4]."""
        return self.forward()[i]


class CameraIntrinsics(nn.Module):
    """A learnable camera matrix around the fixed K0 (3 x 3): fx = fx0 exp(s_x), fy = fy0 exp(s_y) — a focal length stays positive
    and its step is relative — and cx = cx0 + c_x, cy = cy0 + c_y.  Parameters `log_focal` ([1] with tie_focal: one s for both
    axes, else [2]) and `center` ([2]), all zero: forward() starts at K0, bit for bit.  forward() composes the [3,3] tensor with a
    few elementwise torch operations where K0 lives (nine floats once per step; nothing is copied to the host); camera_rows reads
    it in device memory and returns its gradient."""

    def __init__(self, K0, learn_focal=True, learn_center=False, tie_focal=True):
        super().__init__()
        K0 = torch.as_tensor(K0, dtype=torch.float32)
        if tuple(K0.shape) != (3, 3):
            raise ValueError(f"K0 must be [3,3], got {tuple(K0.shape)}")
        self.register_buffer("K0", K0.detach().clone().contiguous())

        def hot(r, c):
            m = torch.zeros(3, 3, device=K0.device)
            m[r, c] = 1.0
            return m
        self.register_buffer("_fx", hot(0, 0))
        self.register_buffer("_fy", hot(1, 1))
        self.register_buffer("_cx", hot(0, 2))
        self.register_buffer("_cy", hot(1, 2))
        self.register_buffer("_rest", torch.ones(3, 3, device=K0.device) - hot(0, 0) - hot(1, 1))
        self.log_focal = nn.Parameter(torch.zeros(1 if tie_focal else 2, device=K0.device), requires_grad=bool(learn_focal))
        self.center = nn.Parameter(torch.zeros(2, device=K0.device), requires_grad=bool(learn_center))

    def forward(self):
        """-> K [3,3]: K0 * (1 everywhere, exp(s) on the two focal entries) + the centre offsets."""
        e = torch.exp(self.log_focal)
        scale = self._fx * e[0] + self._fy * e[-1] + self._rest
        return self.K0 * scale + (self._cx * self.center[0] + self._cy * self.center[1])


def camera_rows(H, W, K, c2w, coords=None, view=None, near=0., far=1., use_viewdirs=False, ndc=True, first=0, B=None):
    """The ray batch of render() for chosen pixels as ONE autograd node over the poses and the camera matrix: rows [B, 8|11] =
    [o, d, near, far (, viewdirs)] (get_rays H:164-173, viewdirs of the pre-NDC direction R:103-110, ndc_rays H:186-202), the tensor
    render() hands to batchify_rays — the same bits as the rows of render(c2w=...) for the same pose and pixel.

        rows = camera_rows(H, W, intr(), poses(), coords, view, near=0., far=1., use_viewdirs=True, ndc=True)
        out = batchify_rays(rows, chunk, **render_kwargs_train)       # R:55-67: the dict render() reshapes
        img2mse(out['rgb_map'], target).backward()                    # poses.rot.grad, poses.trans.grad, intr.log_focal.grad

    c2w: float32 [3,4] | [4,4] | [N,3,4] | [N,4,4] on the GPU, as get_rays_at takes it; coords [B,2] int64 (row, col), or None: the
    B row-major pixels from `first` on; view [B] int64 (None = pose 0).  K: a host 3 x 3 (list / numpy; no gradient), or a float32
    [3,3] tensor on the GPU, read in device memory with or without grad (CameraIntrinsics()); with ndc the two coefficients of
    H:193-199 then are formed from K[0][0] in the kernel and K.grad holds their part too.  near / far: Python scalars.  In-range
    coords and view are the caller's duty."""
    from .run_nerf_helpers import _CameraRowsFn, _pose_tensor
    if torch.is_tensor(near) or torch.is_tensor(far):
        raise ops.CnerfError("camera_rows: near / far are Python scalars (per-ray bounds: write rows[:, 6:8] of a detached copy)")
    return _CameraRowsFn.apply(_pose_tensor(c2w, "camera_rows"), K, H, W, coords, view, float(near), float(far), bool(use_viewdirs),
                               bool(ndc), int(first), B)
