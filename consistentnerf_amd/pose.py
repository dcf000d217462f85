"""Learnable camera poses: c2w[n] = [Exp(rot[n]) R0_n | t0_n + trans[n]] around fixed initial poses, with the rotation update in
axis-angle form so that a refined pose stays a rigid motion (optimising the twelve floats of c2w directly lets the rotation drift off
SO(3)).  The reference optimises no pose; this is the small parametrisation pose-refining NeRF trainers use.

    poses = CameraPoses(c2w0)                                   # [N,3,4] or [N,4,4]
    opt = torch.optim.Adam(list(net.parameters()) + list(poses.parameters()))      # (or optim.FusedAdam)
    o, d = get_rays_at(H, W, K, poses(), coords, view)          # the rays of the batch's pixels, from the device poses
    rgb, *_ = render(H, W, K, rays=(o, d), ndc=False, **kw)
    img2mse(rgb, target).backward()                             # poses.rot.grad, poses.trans.grad

Value and gradient are one HIP launch each for all views (csrc/rays_grad.hip: cnerf_pose_compose[_bwd]); both are exact at rot = 0,
where the parameters start, and lose no digits for small angles."""
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
