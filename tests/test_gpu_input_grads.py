"""Input gradients (csrc/mlp_igrad.hip): run_network with pts / viewdirs requiring grad and render(rays=(rays_o, rays_d)) with the
rays requiring grad, against the oracle (O.query / O.render_rays) in float64 differentiated by autograd on the ReLU branch the
kernel took (its sign bits passed in; pattern differences only within round-off of zero, check_flips).

Error measure, per gradient tensor: err = max|g - g64| / max|g64|.  Bound: the larger of
  1e-5                              what the parameter gradients are held to on the kernel's branch (check_param_grads(rtol=1e-5)), and
  4 x err of the float32 oracle     the same oracle, same masks, evaluated in float32 on the CPU: the reference's own arithmetic; the
                                    factor covers a different summation order and OCML against Sleef sin / cos.
Both are printed by every check.  Inputs of the points form: those of test_mlp_backward_exact_from_stash (RandomState(5), pts ~
U(-3, 3), unit directions, weights of seed 11).
"""
import numpy as np
import pytest
import torch

import _inputs as I
from oracle import nerf_oracle as O
from test_gpu_parity import T, _kwargs, check_flips, dev, make_model, relu_masks, stash_blocks  # noqa: F401  (dev: the device fixture)

pytestmark = pytest.mark.gpu


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def _check(name, g, g64, g32):
    err, err32 = _err(g, g64), _err(g32, g64)
    bound = max(1e-5, 4.0 * err32)
    print(f"  {name}: err {err:.3e} | float32 oracle err {err32:.3e} -> bound max(1e-5, 4 x that) = {bound:.3e}")
    assert err <= bound, f"{name}: err {err:.3e} > bound {bound:.3e}"
    return err, bound


# ------------------------------------------------------------------------------------------------ the points form
# name -> (D, W, multires, multires_views, use_viewdirs, output_ch)
NETS = {"D8W256_vd_skip": (8, 256, 10, 4, True, 4), "D4W128_vd": (4, 128, 10, 4, True, 4), "D4W128_novd_och5": (4, 128, 10, 4, False, 5),
        "D2W64_vd": (2, 64, 10, 4, True, 4), "D8W64_identity_skip": (8, 64, -1, -1, True, 4)}
SHAPES = [(24, 16), (37, 13), (1, 1)]      # M = 384 whole tiles, M = 481 a ragged last tile, a single point


def _state_dict(net):
    D, W, L, Ld, vd, och = NETS[net]
    if L == 10:
        return I.nerf_state_dict(D, W, 10, 4, och, vd, 11)
    rs, sd = np.random.RandomState(11), {}
    for name, shape in I.nerf_param_shapes(D, W, 3, 3, och, vd):
        if name.endswith(".weight"):
            b = np.sqrt(6.0 / shape[1])
            sd[name] = rs.uniform(-b, b, size=shape).astype(np.float32)
        else:
            sd[name] = rs.uniform(-0.1, 0.1, size=shape).astype(np.float32)
    return sd


def _model(net, dev):
    D, W, L, Ld, vd, och = NETS[net]
    if L == 10:
        return make_model(D, W, vd, och, 11, dev)
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = _state_dict(net)
    m = NeRF(D=D, W=W, input_ch=3, output_ch=och, skips=[4], input_ch_views=3, use_viewdirs=vd)
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m.to(dev), sd


def _points_inputs(net, B, S):
    rs = np.random.RandomState(5)
    pts = rs.uniform(-3, 3, size=(B, S, 3)).astype(np.float32)
    dirs = rs.normal(size=(B, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    G = rs.normal(size=(B, S, 5 if net == "D4W128_novd_och5" else 4)).astype(np.float32)
    return pts, dirs, G


def _run_points(dev, net, B, S, pts_grad=True, frozen=False, precision=None):
    """run_network + backward of (raw * G).sum() -> (d_pts, d_viewdirs, parameter gradients, the node's stash)."""
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    D, W, L, Ld, vd, och = NETS[net]
    model, _ = _model(net, dev)
    if precision is not None:
        model.training_precision = precision
    if frozen:
        for p in model.parameters():
            p.requires_grad_(False)
    e, ed = get_embedder(L, 0 if L >= 0 else -1)[0], get_embedder(Ld, 0 if Ld >= 0 else -1)[0]
    pts, dirs, G = _points_inputs(net, B, S)
    tp, td = T(pts, dev).requires_grad_(pts_grad), (T(dirs, dev).requires_grad_(pts_grad) if vd else None)
    raw = run_network(tp, td, model, e, ed)
    stash = raw.grad_fn.stash
    (raw * T(G, dev)).sum().backward()
    return tp.grad, (td.grad if vd else None), [p.grad for p in model.kernel_tensors()], stash


_POINTS = {}


def _points_result(dev, net, B, S):
    """The default run of a case (shared by the tests that compare against it)."""
    key = (net, B, S)
    if key not in _POINTS:
        _POINTS[key] = _run_points(dev, net, B, S)
    return _POINTS[key]


def _points_oracle(net, B, S, masks, dtype, flips=None):
    D, W, L, Ld, vd, och = NETS[net]
    sd = {k: T(v).to(dtype) for k, v in _state_dict(net).items()}
    pts, dirs, G = _points_inputs(net, B, S)
    tp, td = T(pts).to(dtype).requires_grad_(True), T(dirs).to(dtype).requires_grad_(True)
    raw = O.query(sd, tp, td if vd else None, O.NetCfg(D, W, L, Ld, vd, och), masks, flips)
    (raw * T(G).to(dtype)).sum().backward()
    return tp.grad.double(), (td.grad.double() if vd else None)


def _check_points(dev, net, B, S, d_pts, d_dirs, stash):
    D, W, L, Ld, vd, och = NETS[net]
    blk = stash_blocks(stash, B * S, D, W, vd, in_chp=64 if L == 10 else 32)
    masks = [blk[f"h{l}"] > 0 for l in range(D)] + ([blk["hv"] > 0] if vd else [])
    flips = []
    p64, v64 = _points_oracle(net, B, S, masks, torch.float64, flips)
    check_flips(flips)
    p32, v32 = _points_oracle(net, B, S, masks, torch.float32)
    assert d_pts.shape == (B, S, 3)
    out = [_check("d_pts", d_pts, p64, p32)]
    if vd:
        assert d_dirs.shape == (B, 3)
        out.append(_check("d_viewdirs", d_dirs, v64, v32))
    return out


@pytest.mark.parametrize("B,S", SHAPES)
@pytest.mark.parametrize("net", list(NETS))
def test_points_form_against_float64(dev, net, B, S):
    """run_network with pts and viewdirs requiring grad, loss (raw * G).sum(): d_pts [B, S, 3] and d_viewdirs [B, 3].
    Measured on the MI355X over the 15 cases (exact fp32): d_pts err 1.6e-7 .. 2.0e-6 (float32 oracle 2.0e-7 .. 2.4e-6; the largest of
    both is the single point of D4/W128), d_viewdirs err 5.8e-8 .. 2.3e-7 (float32 oracle 5.8e-8 .. 3.1e-7); no ReLU pattern difference."""
    d_pts, d_dirs, _, stash = _points_result(dev, net, B, S)
    _check_points(dev, net, B, S, d_pts, d_dirs, stash)


def test_parameter_gradients_are_untouched(dev):
    """The same call with and without the inputs requiring grad: every parameter gradient bit for bit."""
    net, (B, S) = "D8W256_vd_skip", SHAPES[1]
    with_g = _points_result(dev, net, B, S)[2]
    without = _run_points(dev, net, B, S, pts_grad=False)[2]
    assert len(with_g) == len(without) and all(torch.equal(a, b) for a, b in zip(with_g, without))


def test_frozen_network_runs_the_dgrad_alone(dev, monkeypatch):
    """Every parameter at requires_grad=False: d_pts / d_viewdirs bit for bit those of the trainable network, and the full backward
    (ops.mlp_backward: dgrad + wgrad + reduction) is never launched."""
    from consistentnerf_amd import ops
    net, (B, S) = "D8W256_vd_skip", SHAPES[1]
    ref_pts, ref_dirs = _points_result(dev, net, B, S)[:2]
    calls = []
    real = ops.mlp_backward
    monkeypatch.setattr(ops, "mlp_backward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    d_pts, d_dirs, grads, _ = _run_points(dev, net, B, S, frozen=True)
    assert not calls and all(g is None for g in grads)
    assert torch.equal(d_pts, ref_pts) and torch.equal(d_dirs, ref_dirs)


def test_points_form_bf16x3(dev):
    """training_precision = "bf16x3" (its forward and dgrad write the same stash and workspace), D8/W256 at the ragged shape, at the
    same bound.  Measured on the MI355X: d_pts err 6.3e-7, d_viewdirs err 1.9e-7 (float32 oracle 5.7e-7 / 3.1e-7)."""
    net, (B, S) = "D8W256_vd_skip", SHAPES[1]
    d_pts, d_dirs, _, stash = _run_points(dev, net, B, S, precision="bf16x3")
    _check_points(dev, net, B, S, d_pts, d_dirs, stash)


# ------------------------------------------------------------------------------------------------ the rays form
RB, RNC, RNF, NEAR, FAR = 37, 16, 16, 2.0, 6.0
KCAM = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]     # (only the NDC warp reads the intrinsics)


def _ray_inputs(B=RB):
    b = I.ray_batch(B, seed=3)
    rs = np.random.RandomState(7)
    o, d = b[:, 0:3].copy(), (b[:, 3:6] * rs.uniform(0.5, 2.0, size=(B, 1))).astype(np.float32)     # |d| in [0.5, 2.6]
    G = {k: rs.normal(size=(B, 3) if k.startswith("rgb") else (B,)).astype(np.float32)
         for k in ("rgb_map", "depth_map", "acc_map", "rgb0", "depth0")}
    return o, d, G


def _ray_models(vd, dev, arch=None):
    D, W = arch or ((8, 128) if vd else (4, 128))      # (with a skip layer / without)
    (coarse, sdc), (fine, sdf) = make_model(D, W, vd, 5, 21, dev), make_model(D, W, vd, 5, 22, dev)
    return D, W, coarse, fine, sdc, sdf


def _loss(maps, G, conv):
    return sum((maps[k] * conv(G[k])).sum() for k in G)


def _run_rays(dev, vd, white, chunk, B=RB, Nc=RNC, Nf=RNF, arch=None):
    """render(rays=(o, d)) with both requiring grad + backward of the mixed loss -> (d_rays_o, d_rays_d)."""
    from consistentnerf_amd import run_nerf_view as V
    D, W, coarse, fine, _, _ = _ray_models(vd, dev, arch)
    o, d, G = _ray_inputs(B)
    to, td = T(o, dev).requires_grad_(True), T(d, dev).requires_grad_(True)
    rgb, disp, acc, depth, extras = V.render(1, 1, KCAM, chunk=chunk, rays=(to, td), ndc=False, near=NEAR, far=FAR, use_viewdirs=vd,
                                             **_kwargs(coarse, fine, Nc, Nf, 0.0, white, 0.0, False))
    maps = dict(extras, rgb_map=rgb, depth_map=depth, acc_map=acc)
    _loss(maps, G, lambda g: T(g, dev)).backward()
    return to.grad, td.grad


_RAYS_REF = {}


def _rays_reference(dev, vd, white, B=RB, Nc=RNC, Nf=RNF, arch=None):
    """(float64 oracle gradients, float32 oracle gradients) of the rays form, on the kernel's masks and fine depths; once per case."""
    key = (vd, white, B, Nc, Nf, arch)
    if key in _RAYS_REF:
        return _RAYS_REF[key]
    from consistentnerf_amd import ops, run_nerf_view as V
    D, W, coarse, fine, sdc, sdf = _ray_models(vd, dev, arch)
    o, d, G = _ray_inputs(B)
    # the kernel's own forward on the packed rows: ReLU patterns of both levels and the fine sample depths
    batch = ops.pack_rays(T(o, dev), T(d, dev), NEAR, FAR, vd, False)
    ret = V.render_rays(batch, retraw=True, _debug=True, **_kwargs(coarse, fine, Nc, Nf, 0.0, white, 0.0, False))
    masks_c = relu_masks(ret["_raw_coarse"].grad_fn.stash, B * Nc, D, W, vd)
    masks_f = relu_masks(ret["raw"].grad_fn.stash, B * (Nc + Nf), D, W, vd)
    z_fine = ret["_z_vals"].detach().cpu()

    def run(dtype, flips):
        to, td = T(o).to(dtype).requires_grad_(True), T(d).to(dtype).requires_grad_(True)
        cols = [to, td, torch.full((B, 1), NEAR, dtype=dtype), torch.full((B, 1), FAR, dtype=dtype)]
        if vd:
            cols.append(td / torch.norm(td, dim=-1, keepdim=True))
        out = O.render_rays(torch.cat(cols, -1), {k: T(v).to(dtype) for k, v in sdc.items()}, {k: T(v).to(dtype) for k, v in sdf.items()},
                            O.NetCfg(D, W, use_viewdirs=vd, output_ch=5), O.RenderCfg(Nc, Nf, 0.0, False, white, 0.0),
                            u=torch.linspace(0.0, 1.0, Nf, dtype=dtype).expand(B, Nf), z_fine=z_fine.to(dtype),
                            masks_coarse=masks_c, masks_fine=masks_f, flips=flips)
        _loss(out, G, lambda g: T(g).to(dtype)).backward()
        return to.grad.double(), td.grad.double()

    # The masks are the kernel's branch: the float32 oracle, which sees the positions the kernel saw (x = fl(o + fl(d z)), the same
    # bits), may differ from them only within round-off of zero (1e-5, as everywhere).  The float64 oracle evaluates the encoding at
    # the UNROUNDED o + d z: a position moves by dx <= 1.5 ulp(max|x|), column sin / cos(2^k x) by 2^k dx, a layer-0 pre-activation
    # by at most max|W_0| (6 (2^10 - 1) + 3) dx — pattern differences against it are held to that.
    flips32, flips64 = [], []
    g64, g32 = run(torch.float64, flips64), run(torch.float32, flips32)
    check_flips(flips32)
    xmax = float((T(o)[:, None, :] + T(d)[:, None, :] * z_fine[:, :, None]).abs().max())
    dx = 1.5 * 2.0 ** (np.floor(np.log2(xmax)) - 23)
    check_flips(flips64, tol=1e-5 + float(np.abs(sdc["pts_linears.0.weight"]).max()) * (6 * 1023 + 3) * dx)
    _RAYS_REF[key] = (g64, g32)
    return _RAYS_REF[key]


@pytest.mark.parametrize("chunk", [16, 4096])
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("vd", [True, False])
def test_rays_form_against_float64(dev, vd, white, chunk):
    """render(rays=(o, d)), 37 rays (chunk = 16: three slices), 16 + 16 samples, directions of length 0.5 .. 2.6; the loss mixes
    rgb_map, depth_map, acc_map, rgb0 and depth0.  Measured on the MI355X: d_rays_o err 2.6e-5 .. 3.1e-5, d_rays_d err 2.8e-5 ..
    5.4e-5, the float32 oracle within 1 % of the same figures (bounds 1.1e-4 .. 2.2e-4), chunk 16 and 4096 alike: both evaluate the
    encoding at x = fl(o + fl(d z)), the float64 oracle at the unrounded position, and the 2^9 band turns that ulp into 1e-5s."""
    (o64, d64), (o32, d32) = _rays_reference(dev, vd, white)
    d_o, d_d = _run_rays(dev, vd, white, chunk)
    assert d_o.shape == (RB, 3) and d_d.shape == (RB, 3)
    _check("d_rays_o", d_o, o64, o32)
    _check("d_rays_d", d_d, d64, d32)


def test_rays_form_needs_the_compositing_norm_term(dev, monkeypatch):
    """Without view directions rays_d reaches the maps through x = o + d z and through dists * |rays_d| only: with the second term
    dropped (ops.composite_norm_grad returning zeros) the check of d_rays_d must fail, while d_rays_o stays right."""
    from consistentnerf_amd import ops
    (o64, d64), (o32, d32) = _rays_reference(dev, False, False)
    monkeypatch.setattr(ops, "composite_norm_grad", lambda d_raw, raw, noise, rays: torch.zeros_like(rays))
    d_o, d_d = _run_rays(dev, False, False, 4096)
    _check("d_rays_o (norm term dropped)", d_o, o64, o32)
    err, bound = _err(d_d, d64), max(1e-5, 4.0 * _err(d32, d64))
    print(f"  d_rays_d with the norm term dropped: err {err:.3e} (bound {bound:.3e})")
    assert err > 10 * bound


def test_rays_form_is_deterministic(dev):
    a, b = _run_rays(dev, True, True, 16), _run_rays(dev, True, True, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ what must not change
def test_default_step_takes_none_of_the_new_paths(dev, monkeypatch):
    """A training render_rays step in which no input requires grad: none of the four new ops functions is called, and every parameter
    gradient equals, bit for bit, the one of the single-call C path (cnerf_render_fwd / cnerf_render_bwd), which holds none of the
    new code."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.run_nerf_helpers import sample_u
    calls = []
    for name in ("mlp_input_grad", "rays_input_grad", "composite_norm_grad", "pack_rays_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    D, W, B, Nc, Nf = 4, 128, 37, 16, 16
    coarse, _ = make_model(D, W, True, 5, 51, dev)
    fine, _ = make_model(D, W, True, 5, 52, dev)
    coarse.training_precision = fine.training_precision = "fp32"      # (the single-call C path is the exact-fp32 one)
    rays = T(I.ray_batch(B, seed=9), dev)
    ret = R.render_rays(rays, retraw=True, pytest=True, _with_depth=True, **_kwargs(coarse, fine, Nc, Nf, 0.0, True, 0.0, False))
    keys = ["rgb_map", "disp_map", "acc_map", "depth_map", "rgb0", "disp0", "acc0", "depth0"]
    rs = np.random.RandomState(4)
    gin = {k: T(rs.normal(size=tuple(ret[k].shape)).astype(np.float32), dev) for k in keys}
    sum((ret[k] * gin[k]).sum() for k in keys).backward()
    assert not calls, calls
    out, st = ops.render_forward(coarse.spec(), R._packed(coarse), fine.spec(), R._packed(fine), rays, Nc, Nf, t_rand=None,
                                 u=sample_u(B, Nf, True, True, dev), white_bkgd=True, train=True, retraw=True)
    gc = [torch.empty_like(p) for p in coarse.kernel_tensors()]
    gf = [torch.empty_like(p) for p in fine.kernel_tensors()]
    ops.render_backward(st, gin, gc, gf)
    for gs, model in ((gc, coarse), (gf, fine)):
        for got, p in zip(gs, model.kernel_tensors()):      # tensors the network does not use get zeros / no .grad
            assert torch.equal(got, p.grad) if p.grad is not None else not got.any()


def test_what_still_raises(dev):
    """Each case that has no input gradient raises CnerfError naming itself, at the forward."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    coarse, _ = make_model(2, 64, True, 5, 21, dev)
    kw = _kwargs(coarse, None, 8, 0, 0.0, False, 0.0, False)
    o, d, _ = _ray_inputs()
    to, td = T(o, dev).requires_grad_(True), T(d, dev)
    with pytest.raises(ops.CnerfError, match="ndc=True"):
        R.render(4, 4, KCAM, rays=(to, td), ndc=True, near=NEAR, far=FAR, use_viewdirs=True, **kw)
    rays = ops.pack_rays(to.detach(), td, NEAR, FAR, True, False)
    z = ops.coarse_z(rays, 8, None, False).requires_grad_(True)
    with pytest.raises(ops.CnerfError, match="z_vals"):
        R.run_network(R.RayPoints(rays, z), rays[:, -3:], coarse, get_embedder(10, 0)[0], get_embedder(4, 0)[0])
    c2w = torch.eye(4, device=dev)[:3].requires_grad_(True)
    with pytest.raises(ops.CnerfError, match="c2w"):
        R.render(4, 4, KCAM, c2w=c2w, ndc=False, near=NEAR, far=FAR, use_viewdirs=True, **kw)
    with pytest.raises(ops.CnerfError, match="render_loss"):
        R.render_loss(4, 4, KCAM, torch.rand(RB, 3, device=dev), rays=(to, td), ndc=False, near=NEAR, far=FAR, use_viewdirs=True, **kw)
