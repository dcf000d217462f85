"""GPU tests of the opt-in "fp16x2" inference forward (csrc/mlp_fwd_bf.hip, PL_F16: two fp16 planes per operand, three products on
v_mfma_f32_32x32x16_f16, power-of-two operand scaling), modelled on test_bf16_plane_inference_forward and
test_bf16_plane_inference_is_opt_in_and_never_trains of tests/test_gpu_parity.py.  Its tier is the project's fp32-like one — the
bf16x3 bound of that test, 2e-5 of max(1, max|raw|) — not a number of its own."""
import os

import numpy as np
import pytest
import torch

import _inputs as I
from conftest import golden

pytestmark = pytest.mark.gpu

TIER = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def T(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


def _model(D, W, seed, dev, och=4):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = I.nerf_state_dict(D, W, 10, 4, och, True, seed)
    m = NeRF(D=D, W=W, input_ch=63, output_ch=och, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m.to(dev)


def _trained(g, dev, hot=1.0):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    out = []
    for tag in ("c.", "f."):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
        sd = {k[len(tag):]: T(g[k]) for k in g if k.startswith(tag)}
        if hot != 1.0:
            sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * hot
            sd["pts_linears.0.bias"] = sd["pts_linears.0.bias"] * hot
        m.load_state_dict(sd, strict=True)
        out.append(m.to(dev))
    return out


def _kwargs(coarse, fine, Nc, Nf):
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    e, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    q = lambda inputs, viewdirs, fn: run_network(inputs, viewdirs, fn, embed_fn=e, embeddirs_fn=ed)  # noqa: E731
    return dict(network_query_fn=q, perturb=0.0, N_importance=Nf, network_fine=fine, N_samples=Nc, network_fn=coarse,
                white_bkgd=False, raw_noise_std=0.0, lindisp=False)


def _perwave(fn):
    os.environ["CNERF_BF_PERWAVE"] = "1"
    try:
        return fn()
    finally:
        del os.environ["CNERF_BF_PERWAVE"]


@pytest.mark.parametrize("D,W,tag", [(8, 256, "mlp_D8W256_vd"), (8, 128, "mlp_D8W128_vd"), (4, 128, "mlp_D4W128_vd")])
def test_fp16x2_forward_tier_order_and_one_arithmetic(dev, D, W, tag):
    """1. Tier: against the reference capture and against the exact-fp32 kernel, at M, M - 13 and 300 points.  2. Order: strictly
    below the bf16x2 error in the same run (ratio printed, no factor asserted).  3. The shared-panel and per-wave kernels are
    bit-identical, and eight launches on 40 000 points equal the per-wave result (the ring race check)."""
    from consistentnerf_amd import ops
    g = golden(tag)
    model = _model(D, W, 11, dev)
    spec = model.spec()
    pts, dirs = T(g["pts"], dev).reshape(-1, 3).contiguous(), T(g["dirs"], dev)
    M = pts.shape[0]
    dirs = dirs if dirs.shape[0] == M else dirs[:, None, :].expand(-1, M // dirs.shape[0], -1).reshape(-1, 3).contiguous()
    ref, _ = ops.mlp_forward(spec, ops.pack_weights(spec, model.kernel_tensors()), M, 1, pts=pts, dirs=dirs)
    cap = T(g["raw"], dev).reshape(M, 1, 4)
    scale = max(1.0, float(cap.abs().max()))
    errs, errs32 = {}, {}
    for name in ("bf16x2", "fp16x2"):
        planes = ops.PRECISION_PLANES[name]
        pk = ops.pack_weights_bf(spec, model.kernel_tensors(), planes)
        for Mr in (M, M - 13, 300):
            p_, d_ = pts[:Mr].contiguous(), dirs[:Mr].contiguous()
            raw = ops.mlp_forward_bf(spec, pk, planes, Mr, 1, pts=p_, dirs=d_)
            assert torch.isfinite(raw).all()
            errs[name] = max(errs.get(name, 0.0), float((raw - cap[:Mr]).abs().max()) / scale)
            errs32[name] = max(errs32.get(name, 0.0), float((raw - ref[:Mr]).abs().max()) / scale)
            raw_v = _perwave(lambda: ops.mlp_forward_bf(spec, pk, planes, Mr, 1, pts=p_, dirs=d_))
            assert torch.equal(raw, raw_v), (name, Mr, float((raw - raw_v).abs().max()))
        print(f"  {tag} {name}: max|d raw| / max(1, max|raw|) vs the capture {errs[name]:.3e}, vs the fp32 kernel {errs32[name]:.3e}")
    print(f"  {tag}: bf16x2 / fp16x2 error ratio vs the capture {errs['bf16x2'] / max(errs['fp16x2'], 1e-30):.1f}x")
    rs = np.random.RandomState(5)
    big = T(rs.uniform(-2, 2, size=(40000, 3)).astype(np.float32), dev)
    bdirs = T(rs.normal(size=(40000, 3)).astype(np.float32), dev)
    planes = ops.PLANES_FP16X2
    pk = ops.pack_weights_bf(spec, model.kernel_tensors(), planes)
    want = _perwave(lambda: ops.mlp_forward_bf(spec, pk, planes, 40000, 1, pts=big, dirs=bdirs))
    for rep in range(8):
        got = ops.mlp_forward_bf(spec, pk, planes, 40000, 1, pts=big, dirs=bdirs)
        assert torch.equal(got, want), (rep, float((got - want).abs().max()))
    assert errs["fp16x2"] <= TIER and errs32["fp16x2"] <= TIER
    assert errs["fp16x2"] < errs["bf16x2"]


def test_fp16x2_trained_network_and_range(dev):
    """4. The trained coarse + fine nets of render_rays_trained on its 1024 rays under no_grad: PSNR of the fp16x2 render against
    the fp32 render >= that of bf16x2 in the same run and >= bf16x2's floor of 60 dB (all three printed).  Then the hot variant —
    layer-0 weight and bias of both nets x64, activations in the hundreds — stays finite and within the tier against the
    exact-fp32 kernel on the same points."""
    from consistentnerf_amd import ops, run_nerf as R
    g = golden("render_rays_trained")
    coarse, fine = _trained(g, dev)
    rays = T(g["rays"], dev)
    kw = _kwargs(coarse, fine, 64, 128)
    psnr = {}
    try:
        with torch.no_grad():
            ref = R.render_rays(rays, **kw)
            for prec in ("bf16x2", "bf16x3", "fp16x2"):
                coarse.inference_precision = fine.inference_precision = prec
                out = R.render_rays(rays, **kw)
                assert torch.isfinite(out["rgb_map"]).all()
                mse = float(((out["rgb_map"] - ref["rgb_map"]) ** 2).mean())
                psnr[prec] = 150.0 if mse == 0 else -10.0 * np.log10(mse)
    finally:
        coarse.inference_precision = fine.inference_precision = "fp32"
    print("  trained nets, rendered rgb vs the fp32 render: " + ", ".join(f"{k} {v:.1f} dB" for k, v in psnr.items()))
    assert psnr["fp16x2"] >= psnr["bf16x2"] and psnr["fp16x2"] >= 60.0
    # the hot variant, network by network, on sample points along the fixture's rays
    near, far = (float(x) for x in g["near_far"])
    z = torch.linspace(near, far, 64, device=dev)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[None, :, None]).reshape(-1, 3).contiguous()
    dirs = rays[:, None, -3:].expand(-1, 64, -1).reshape(-1, 3).contiguous()
    M = pts.shape[0]
    for net in _trained(g, dev, hot=64.0):
        spec = net.spec()
        want, _ = ops.mlp_forward(spec, ops.pack_weights(spec, net.kernel_tensors()), M, 1, pts=pts, dirs=dirs)
        got = ops.mlp_forward_bf(spec, ops.pack_weights_bf(spec, net.kernel_tensors(), ops.PLANES_FP16X2), ops.PLANES_FP16X2,
                                 M, 1, pts=pts, dirs=dirs)
        scale = max(1.0, float(want.abs().max()))
        e = float((got - want).abs().max()) / scale
        print(f"  hot variant (layer 0 x64): max|raw| {scale:.4g}, fp16x2 vs the fp32 kernel {e:.3e} of it")
        assert torch.isfinite(got).all() and e <= TIER


def test_fp16x2_is_opt_in_keyed_by_mode_and_sees_weight_updates(dev):
    """5. Default fp32; a forward that may need gradients runs the fp32 training kernel; under no_grad both levels run the fp16x2
    kernel (by profile name); an unknown precision raises a ValueError that names fp16x2; bf16x2 -> fp16x2 -> bf16x2 gives the
    bf16x2 bits again (the packed-panel cache is keyed by mode); an in-place weight update reaches the next forward."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.run_nerf_helpers import NeRF
    assert NeRF.inference_precision == "fp32"
    coarse, fine = _model(8, 256, 21, dev, 5), _model(8, 256, 22, dev, 5)
    rays = T(I.ray_batch(1000, seed=5, near=2.125, far=4.67), dev)
    kw = _kwargs(coarse, fine, 64, 128)

    def kinds_of(fn):
        ops.PROFILE = []
        try:
            out = fn()
            return out, [n for n, *_ in ops.PROFILE]
        finally:
            ops.PROFILE = None
    # (CNERF_TRAIN_PRECISION=bf16x3 runs the suite with the three-plane training kernels: their names differ)
    train_name = "mlp_fwd_train_bf3" if os.environ.get("CNERF_TRAIN_PRECISION", "fp32") == "bf16x3" else "mlp_fwd_train"
    try:
        with torch.no_grad():
            _, k0 = kinds_of(lambda: R.render_rays(rays, **kw))
        assert k0.count("mlp_fwd") == 2
        coarse.inference_precision = fine.inference_precision = "bf16x2"
        with torch.no_grad():
            b0 = R.render_rays(rays, **kw)["rgb_map"].clone()
        coarse.inference_precision = fine.inference_precision = "fp16x2"
        with torch.no_grad():
            out, k = kinds_of(lambda: R.render_rays(rays, **kw))
        assert k.count("mlp_fwd_fp16x2") == 2 and "mlp_fwd" not in k and not any(n.startswith("mlp_fwd_bf") for n in k)
        f0 = out["rgb_map"].clone()
        _, k = kinds_of(lambda: R.render_rays(rays, **kw))              # autograd on: the training kernels, with a stash
        assert k.count(train_name) == 2 and "mlp_fwd_fp16x2" not in k
        coarse.inference_precision = fine.inference_precision = "bf16x2"
        with torch.no_grad():
            b1 = R.render_rays(rays, **kw)["rgb_map"]
        assert torch.equal(b0, b1) and not torch.equal(b0, f0)
        coarse.inference_precision = fine.inference_precision = "fp16x2"
        with torch.no_grad():
            fine.rgb_linear.bias.add_(0.25)
            f1 = R.render_rays(rays, **kw)["rgb_map"]
            fine.rgb_linear.bias.sub_(0.25)
            f2 = R.render_rays(rays, **kw)["rgb_map"]
        assert float((f1 - f0).abs().max()) > 1e-3 and float((f2 - f0).abs().max()) <= 1e-6
        coarse.inference_precision = "fp8"
        with pytest.raises(ValueError, match="fp16x2"):
            with torch.no_grad():
                R.render_rays(rays, **kw)
    finally:
        coarse.inference_precision = fine.inference_precision = "fp32"


def test_fp16x2_pack_and_forward_replay_from_a_graph(dev):
    """6. Pack + forward recorded with torch.cuda.graph replay to the eager bits — also after the weights changed in place, which
    only holds if the pack call reads nothing back on the host."""
    from consistentnerf_amd import ops
    model = _model(8, 256, 11, dev)
    spec, planes = model.spec(), ops.PLANES_FP16X2
    rs = np.random.RandomState(9)
    M = 5000
    pts = T(rs.uniform(-2, 2, size=(M, 3)).astype(np.float32), dev)
    dirs = T(rs.normal(size=(M, 3)).astype(np.float32), dev)
    params = [p.detach() for p in model.kernel_tensors()]
    eager = ops.mlp_forward_bf(spec, ops.pack_weights_bf(spec, params, planes), planes, M, 1, pts=pts, dirs=dirs).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pk = ops.pack_weights_bf(spec, params, planes)
        ops.mlp_forward_bf(spec, pk, planes, M, 1, pts=pts, dirs=dirs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.pack_weights_bf(spec, params, planes, out=pk)
        raw = ops.mlp_forward_bf(spec, pk, planes, M, 1, pts=pts, dirs=dirs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(raw, eager)
    with torch.no_grad():
        params[0].mul_(1.5)
    eager2 = ops.mlp_forward_bf(spec, ops.pack_weights_bf(spec, params, planes), planes, M, 1, pts=pts, dirs=dirs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(raw, eager2) and not torch.equal(eager2, eager)
