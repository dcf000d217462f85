"""CPU restatement of the "fp16x2" inference arithmetic (csrc/mlp_fwd_bf.hip, PL_F16): every GEMM operand as two fp16 planes
x = h + l (h = fp16(x), l = fp16(x - h), round to nearest even), the three products w_h x_h + w_h x_l + w_l x_h, and the
power-of-two scale rule the kernel applies — imported from the package, so this file fails without the feature.

Worst case for the hardware: every plane value below fp16's smallest normal (2^-14) is FLUSHED to zero here, as a matrix pipe
that ignores subnormal inputs would.  The products are exact and the accumulation is float64 rounded to fp32 once per GEMM, so
the figure isolates the split error (the kernel's fp32 accumulation adds about 1e-7).  Bound: the project's fp32-like tier,
2e-5 of max(1, max|raw|) against a float64 forward, and strictly better than the emulated bf16x2 on the same inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _inputs as I
import _planes_ref as P
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (8, 256, 10, 4, 4)


def _forward(sd, pts, dirs, mode, flush=True):
    """The network as the kernel computes it (tests/_planes_ref.py) -> (raw, the largest activation)."""
    return P.forward_planes(sd, pts, dirs, CFG, mode, flush=flush)


def _ref64(sd, pts, dirs):
    return P.forward64(sd, pts, dirs, CFG)


def _nets():
    rs = np.random.RandomState(0)
    M = 2048
    out = {"random_init": (I.nerf_state_dict(8, 256, 10, 4, 4, True, 11), torch.tensor(rs.uniform(-2, 2, (M, 3)), dtype=torch.float32))}
    g = golden("render_rays_trained")
    rays = torch.tensor(g["rays"])
    near, far = g["near_far"]
    z = torch.tensor(rs.uniform(near, far, (M, 1)), dtype=torch.float32)
    rr = rays[rs.randint(0, rays.shape[0], M)]
    fine = {k[2:]: g[k] for k in g if k.startswith("f.")}
    out["trained_fine"] = (fine, rr[:, :3] + rr[:, 3:6] * z)
    hot = dict(fine)       # layer 0 x64: activations in the hundreds, the upper end of what a NeRF trunk sees
    hot["pts_linears.0.weight"] = fine["pts_linears.0.weight"] * 64.0
    hot["pts_linears.0.bias"] = fine["pts_linears.0.bias"] * 64.0
    out["trained_fine_hot"] = (hot, rr[:, :3] + rr[:, 3:6] * z)
    dirs = torch.tensor(rs.normal(size=(M, 3)), dtype=torch.float32)
    return out, dirs / dirs.norm(dim=-1, keepdim=True)


def test_scale_rule_is_one_rule_in_header_kernel_and_package():
    from consistentnerf_amd import ops
    hdr = open(os.path.join(ROOT, "consistentnerf_amd", "csrc", "mlp_bf_common.hpp")).read()
    m = re.search(r"constexpr int F16_SW = (\d+), F16_SX = (\d+);", hdr)
    assert m and (int(m.group(1)), int(m.group(2))) == (ops.FP16X2_WEIGHT_SHIFT, ops.FP16X2_ACT_SHIFT)
    abi = open(os.path.join(ROOT, "include", "cnerf.h")).read()
    m = re.search(r"#define CNERF_PLANES_FP16X2 (\d+)", abi)
    assert m and int(m.group(1)) == ops.PLANES_FP16X2 == ops.PRECISION_PLANES["fp16x2"]
    assert len(set(ops.PRECISION_PLANES.values())) == len(ops.PRECISION_PLANES)       # one cache key per mode
    # conversion stays finite inside the documented range
    assert float(torch.tensor(ops.FP16X2_MAX_WEIGHT * 2.0 ** ops.FP16X2_WEIGHT_SHIFT).to(torch.float16)) == 65504.0
    assert float(torch.tensor(ops.FP16X2_MAX_ACTIVATION * 2.0 ** ops.FP16X2_ACT_SHIFT).to(torch.float16)) == 65504.0


def test_planes_argument_of_the_c_abi():
    """CNERF_PLANES_FP16X2 sizes like two bf16 planes; every value other than 1, 2, 3 and it is still rejected (host only)."""
    from consistentnerf_amd import _lib, ops
    lib = _lib.load()
    net = ops.NetSpec(D=8, W=256, use_viewdirs=True, output_ch=5).c()
    n2 = lib.cnerf_packed_bf_bytes(C.byref(net), 2)
    assert n2 > 0 and lib.cnerf_packed_bf_bytes(C.byref(net), ops.PLANES_FP16X2) == n2
    for bad in (0, 4, 16, 17, 19, 34, -1):
        assert lib.cnerf_packed_bf_bytes(C.byref(net), bad) == -1, bad
        assert lib.cnerf_pack_weights_bf(C.byref(net), None, bad, None, None) == -2, bad
        assert lib.cnerf_mlp_fwd_bf(C.byref(net), None, bad, None, None, 0, None, None, 0, 1, None, None) == -2, bad
    assert lib.cnerf_pack_weights_bf(C.byref(net), None, ops.PLANES_FP16X2, None, None) == -1           # null arguments
    assert lib.cnerf_mlp_fwd_bf(C.byref(net), None, ops.PLANES_FP16X2, None, None, 0, None, None, 0, 1, None, None) == -1


@pytest.mark.parametrize("name", ["random_init", "trained_fine", "trained_fine_hot"])
def test_fp16x2_arithmetic_reaches_the_fp32_like_tier_with_subnormals_flushed(name):
    nets, dirs = _nets()
    sd, pts = nets[name]
    ref = _ref64(sd, pts, dirs)
    scale = max(1.0, float(ref.abs().max()))
    out, amax = _forward(sd, pts, dirs, "fp16x2", flush=True)
    out_keep, _ = _forward(sd, pts, dirs, "fp16x2", flush=False)
    out_bf, _ = _forward(sd, pts, dirs, "bf16x2")
    e = float((out.double() - ref).abs().max()) / scale
    e_keep = float((out_keep.double() - ref).abs().max()) / scale
    e_bf = float((out_bf.double() - ref).abs().max()) / scale
    print(f"  {name}: max|raw| {scale:.3g}, max|activation| {amax:.3g}: fp16x2 flush {e:.2e}, subnormals kept {e_keep:.2e}, "
          f"bf16x2 {e_bf:.2e} ({e_bf / e:.1f}x)")
    from consistentnerf_amd import ops
    assert torch.isfinite(out).all() and amax < ops.FP16X2_MAX_ACTIVATION
    assert e <= 2e-5 and e_keep <= 2e-5
    assert e < e_bf
