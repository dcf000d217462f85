"""GPU tests of the in-kernel standard-normal stream (csrc/rng.hpp CnRngDev::normal, csrc/noise.hip) and of its users: the density
noise of render_rays / raw2outputs (R:287-288, `raw_noise_std > 0`) drawn for both levels in one launch on the render_rays call's own
block of stream offsets, shards drawing their own rows only, the graphed step replaying the eager step's noise, and the
`--use_noise` label noise (V:1633-1638).  tests/_noise_ref.py is the float64 restatement the stream is compared with (1e-5
absolute: ~20 fp32 ulp at the bound 5.768; a numpy fp32 evaluation of the formula is 1.6e-6 away, tests/test_noise_ref.py);
everything between our own launches is bit for bit."""
import numpy as np
import pytest
import torch

import _inputs as I
import _noise_ref as N
from oracle import philox as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def same(a, b):
    """bit-equal, NaNs (disp of a ray that hits nothing: 0 / 0, R:302) in the same places"""
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def T(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


def make_model(D, W, seed, dev):
    from consistentnerf_amd.run_nerf_helpers import NeRF
    sd = I.nerf_state_dict(D, W, 10, 4, 5, True, seed)
    m = NeRF(D=D, W=W, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m.to(dev)


def _kwargs(coarse, fine, Nc, Nf, perturb, white=False, noise=1.0):
    from consistentnerf_amd.run_nerf import run_network
    from consistentnerf_amd.run_nerf_helpers import get_embedder
    e, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    q = lambda inputs, viewdirs, fn: run_network(inputs, viewdirs, fn, embed_fn=e, embeddirs_fn=ed)  # noqa: E731
    return dict(network_query_fn=q, perturb=perturb, N_importance=Nf, network_fine=fine, N_samples=Nc, network_fn=coarse,
                white_bkgd=white, raw_noise_std=noise, lindisp=False)


# ------------------------------------------------------------------------------------------------ 1: the stream
@pytest.mark.parametrize("offset_add", [2, 7])
@pytest.mark.parametrize("rows,cols,row0", [(1, 1, 0), (5, 33, 0), (5, 33, 11), (257, 192, 0), (257, 192, 11), (3, 4, 0), (3, 4, 2 ** 31)])
def test_normal_stream_equals_the_float64_restatement(dev, rows, cols, row0, offset_add):
    from consistentnerf_amd import ops
    seed, base = 2 ** 64 - 3, 2 ** 40 + 8
    rng = ops.RngStream(seed, base, None, row0)
    got = ops.normal_rng(rng, rows, cols, dev, offset_add)
    ref = N.normal(seed, base + offset_add, rows, cols, row0)
    g = got.cpu().numpy()
    d = float(np.abs(g.astype(np.float64) - ref).max())
    print(f"  [{rows}, {cols}] row0 {row0} offset +{offset_add}: max|d| {d:.3e}, max|n| {np.abs(g).max():.4f}")
    assert g.dtype == np.float32 and g.shape == (rows, cols) and np.isfinite(g).all() and np.abs(g).max() <= 5.7682
    assert d <= 1e-5
    # {seed, base offset} read from device memory (the form a hipGraph replays) == by value
    state = T(np.array([seed, base], dtype=np.uint64).view(np.int64), dev)
    assert torch.equal(ops.normal_rng(ops.RngStream(0, 0, state, row0), rows, cols, dev, offset_add), got)
    # rows [r0, r0 + n) of the call on [row0, ...) == the call that starts at row0 + r0 (through the stream and through `row0=`)
    r0, n = rows // 3, rows - rows // 3
    assert torch.equal(ops.normal_rng(ops.RngStream(seed, base, None, row0 + r0), n, cols, dev, offset_add), got[r0:])
    assert torch.equal(ops.normal_rng(rng, n, cols, dev, offset_add, row0=row0 + r0), got[r0:])
    # scale: ONE fp32 multiply after the product
    for s in (0.1, 3.0):
        assert torch.equal(ops.normal_rng(rng, rows, cols, dev, offset_add, scale=s), got * torch.tensor(s, dtype=torch.float32, device=dev))
    assert ops.normal_rng(rng, 0, cols, dev).shape == (0, cols)


# ------------------------------------------------------------------------------------------------ 2: both levels, one launch
@pytest.mark.parametrize("B,Nc,S1", [(5, 33, 133), (1, 4, 5), (96, 64, 192), (7, 16, 0)])
def test_density_noise_draws_both_levels_in_one_launch(dev, B, Nc, S1):
    from consistentnerf_amd import ops
    std = 0.75
    for rng in (ops.RngStream(1234, 8), ops.RngStream(77, 2 ** 33 + 4, None, 1000)):
        n0, n1 = ops.density_noise(rng, B, Nc, S1, std, dev)
        assert n0.shape == (B, Nc) and torch.equal(n0, ops.normal_rng(rng, B, Nc, dev, 2, scale=std))
        if S1 == 0:
            assert n1 is None
            continue
        assert n1.shape == (B, S1) and torch.equal(n1, ops.normal_rng(rng, B, S1, dev, 3, scale=std))
        m = min(Nc, S1)
        assert not torch.equal(n0[:, :m], n1[:, :m])
        assert not torch.equal(n0.flatten(), n1.flatten()[:B * Nc])       # (nor the same flat stream cut differently)
    assert ops.density_noise(ops.RngStream(1, 0), 0, Nc, S1, std, dev)[0].shape == (0, Nc)


# ------------------------------------------------------------------------------------------------ 3: moments
def test_normal_stream_moments(dev):
    """seed 1234, offset 6, [4096, 256]: each limit is five standard errors at N = 2^20 (tests/_noise_ref.py LIMITS; the
    restatement itself meets them, tests/test_noise_ref.py)."""
    from consistentnerf_amd import ops
    x = ops.normal_rng(ops.RngStream(1234, 4), 4096, 256, dev, 2).cpu().numpy()
    assert np.isfinite(x).all() and np.abs(x).max() <= 5.7682
    got = N.moments(x, P.uniform(1234, 4, 4096, 256))
    print({k: f"{v:.2e}" for k, v in got.items()})
    for k, lim in N.LIMITS.items():
        assert abs(got[k]) <= lim, (k, got[k], lim)


# ------------------------------------------------------------------------------------------------ 4: render_rays
@pytest.mark.parametrize("white", [False, True])
def test_render_rays_draws_its_noise_in_kernel_and_nothing_else(dev, white):
    """perturb = 1, raw_noise_std = 1, not pytest: the call advances the generator by exactly ops.RNG_STRIDE (a leftover
    torch.randn would advance it further) and every map / parameter gradient equals the single-call C path fed with the four
    materialised streams of that (seed, offset) bit for bit; with perturb = 0 the block is reserved for the noise alone and the
    coarse depths stay unjittered."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd.run_nerf_helpers import sample_u
    B, Nc, Nf = 45, 33, 100
    coarse, fine = make_model(4, 128, 51, dev), make_model(4, 128, 52, dev)
    rays = T(I.ray_batch(B, seed=9), dev)
    gen = torch.cuda.default_generators[0]
    keys = ["rgb_map", "disp_map", "acc_map", "depth_map", "rgb0", "disp0", "acc0", "depth0"]
    for perturb in (1.0, 0.0):
        for p in list(coarse.parameters()) + list(fine.parameters()):
            p.grad = None
        torch.manual_seed(4321)
        off = gen.get_offset()
        ret = R.render_rays(rays, retraw=True, _with_depth=True, _debug=True, **_kwargs(coarse, fine, Nc, Nf, perturb, white))
        assert gen.get_offset() == off + ops.RNG_STRIDE
        rs = np.random.RandomState(4)
        gin = {k: T(rs.normal(size=tuple(ret[k].shape)).astype(np.float32), dev) for k in keys}
        sum((ret[k] * gin[k]).sum() for k in keys).backward()
        rng = ops.RngStream(4321, off)
        n0, n1 = ops.density_noise(rng, B, Nc, Nc + Nf, 1.0, dev)
        if perturb > 0:
            t_rand, u = ops.uniform_rng(rng, B, Nc, dev, 0), ops.uniform_rng(rng, B, Nf, dev, 1)
        else:
            t_rand, u = None, sample_u(B, Nf, True, False, dev)
            assert torch.equal(ret["_z_coarse"], ops.coarse_z(rays, Nc, None, False))
        out, st = ops.render_forward(coarse.spec(), R._packed(coarse), fine.spec(), R._packed(fine), rays, Nc, Nf, t_rand=t_rand, u=u,
                                     noise0=n0, noise1=n1, white_bkgd=white, train=True, retraw=True)
        for k in keys + ["raw", "z_std"]:
            assert same(out[k], ret[k].detach()), (perturb, k)
        gc = [torch.empty_like(p) for p in coarse.kernel_tensors()]
        gf = [torch.empty_like(p) for p in fine.kernel_tensors()]
        ops.render_backward(st, gin, gc, gf)
        for gs, model in ((gc, coarse), (gf, fine)):
            for got, p in zip(gs, model.kernel_tensors()):   # tensors the network does not use get zeros / no .grad
                assert torch.equal(got, p.grad) if p.grad is not None else not got.any()
        assert any(p.grad is not None and p.grad.any() for p in coarse.parameters())


def test_raw2outputs_draws_its_noise_from_its_own_block(dev):
    """Stand-alone raw2outputs(raw_noise_std > 0): its own rng_draw block, the coarse level's stream (+2), cols = S."""
    from consistentnerf_amd import ops, run_nerf as R
    B, S = 19, 37
    g = torch.Generator(device=dev).manual_seed(2)
    raw = torch.randn(B, S, 4, device=dev, generator=g)
    z = torch.sort(torch.rand(B, S, device=dev, generator=g) * 4 + 2, -1).values
    rays_d = torch.randn(B, 3, device=dev, generator=g)
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(99)
    off = gen.get_offset()
    got = R.raw2outputs(raw, z, rays_d, raw_noise_std=0.5)
    assert gen.get_offset() == off + ops.RNG_STRIDE
    rays = torch.cat([torch.zeros_like(rays_d), rays_d], -1).contiguous()
    ref = ops.composite_forward(raw, z, rays, ops.normal_rng(ops.RngStream(99, off), B, S, dev, 2, scale=0.5), False)
    for a, b in zip(got, ref):
        assert same(a, b)
    assert not same(got[0], R.raw2outputs(raw, z, rays_d, raw_noise_std=0.0)[0])


# ------------------------------------------------------------------------------------------------ 5: shards
def test_a_shard_draws_its_own_rows_only(dev, monkeypatch):
    from consistentnerf_amd import ops, run_nerf as R
    coarse, fine = make_model(4, 128, 71, dev), make_model(4, 128, 72, dev)
    rays = T(I.ray_batch(384, seed=9), dev)
    kw = _kwargs(coarse, fine, 32, 48, 1.0)
    calls, draw = [], ops.density_noise

    def recorder(rng, B, Nc, S1, std, device):
        out = draw(rng, B, Nc, S1, std, device)
        calls.append((B, rng.row0, out))
        return out
    monkeypatch.setattr(ops, "density_noise", recorder)
    with torch.no_grad():
        torch.manual_seed(123)
        whole = R.render_rays(rays, _with_depth=True, **kw)
        torch.manual_seed(123)
        part = R.render_rays(rays[128:384], _with_depth=True, _global_rows=(128, 384), **kw)
    assert [(c[0], c[1]) for c in calls] == [(384, 0), (256, 128)]
    (n0w, n1w), (n0p, n1p) = calls[0][2], calls[1][2]
    assert n0p.shape == (256, 32) and n1p.shape == (256, 80)
    assert torch.equal(n0p, n0w[128:384]) and torch.equal(n1p, n1w[128:384])
    for k in ("rgb_map", "depth_map", "rgb0", "depth0", "z_std"):
        assert torch.equal(part[k], whole[k][128:384]), k


# ------------------------------------------------------------------------------------------------ 6: the graphed step
def test_graphed_step_with_density_noise_equals_eager_steps(dev):
    """GraphedStep on a two-level step with raw_noise_std = 1, perturb = 1: three replays from a seeded generator == three eager
    steps from the same seed, bit for bit in loss and weights (the noise reads {seed, offset} from device memory like the jitter)."""
    from consistentnerf_amd import run_nerf as R
    from consistentnerf_amd.graph import GraphedStep
    from consistentnerf_amd.optim import FusedAdam

    def build():
        coarse, fine = make_model(2, 64, 93, dev), make_model(2, 64, 94, dev)
        kw = _kwargs(coarse, fine, 16, 16, 1.0)
        opt = FusedAdam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)

        def step_fn(rays, tgt):
            out = R.render_rays(rays, **kw)
            opt.zero_grad()
            loss = R.img2mse(out["rgb_map"], tgt) + R.img2mse(out["rgb0"], tgt)
            loss.backward()
            opt.step()
            return loss
        return opt, step_fn
    g = torch.Generator(device=dev).manual_seed(8)
    batches = [(T(I.ray_batch(64, seed=40 + i), dev), torch.rand(64, 3, device=dev, generator=g)) for i in range(3)]
    opt_e, step_e = build()
    opt_e.make_capturable()
    torch.manual_seed(7)
    for _ in range(2):                               # the warm-up steps GraphedStep runs before it records
        step_e(*batches[0])
    torch.manual_seed(2024)
    le = [step_e(rays, tgt).item() for rays, tgt in batches]
    opt_g, step_g = build()
    torch.manual_seed(7)
    gs = GraphedStep(step_g, opt_g, batches[0], warmup=2)
    torch.manual_seed(2024)
    lg = [gs(rays, tgt).detach().clone() for rays, tgt in batches]       # (device-side copies: no host sync between replays)
    lg = [float(x) for x in lg]
    assert le == lg, (le, lg)
    assert torch.equal(opt_e.flat_param, opt_g.flat_param)
    assert len(set(le)) == 3


# ------------------------------------------------------------------------------------------------ 7: --use_noise
def test_label_noise_comes_from_one_block_of_normal_streams(dev):
    from consistentnerf_amd import ops, run_nerf_view as V
    B, std, far = 37, 0.1, 6.0
    g = torch.Generator(device=dev).manual_seed(5)
    rgb, dep = torch.rand(B, 3, device=dev, generator=g), torch.rand(B, device=dev, generator=g)
    ex = dict(rgb0=torch.rand(B, 3, device=dev, generator=g), depth0=torch.rand(B, device=dev, generator=g), z_std=torch.ones(B, device=dev))
    ex0 = dict(ex)
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(11)
    off = gen.get_offset()
    r2, d2, e2 = V.add_label_noise(rgb, dep, ex, std, far)
    assert gen.get_offset() == off + ops.RNG_STRIDE and e2 is ex
    rng = ops.RngStream(11, off)
    assert torch.equal(r2, rgb + ops.normal_rng(rng, B, 3, dev, 0, scale=std))
    assert torch.equal(d2, dep + far * ops.normal_rng(rng, B, 1, dev, 1, scale=std).view(B))
    assert torch.equal(ex["rgb0"], ex0["rgb0"] + ops.normal_rng(rng, B, 3, dev, 2, scale=std))
    assert torch.equal(ex["depth0"], ex0["depth0"] + far * ops.normal_rng(rng, B, 1, dev, 3, scale=std).view(B))
    assert ex["z_std"] is ex0["z_std"]
    # a shard's rows
    torch.manual_seed(11)
    r3, d3, _ = V.add_label_noise(rgb[10:], dep[10:], {}, std, far, row0=10)
    assert torch.equal(r3, r2[10:]) and torch.equal(d3, d2[10:])
    # a caller's generator keeps torch.randn
    off = gen.get_offset()
    r4, d4, _ = V.add_label_noise(rgb, dep, {}, std, far, generator=torch.Generator(device=dev).manual_seed(3))
    g3 = torch.Generator(device=dev).manual_seed(3)
    assert torch.equal(r4, rgb + torch.randn(rgb.shape, device=dev, generator=g3) * std)
    assert torch.equal(d4, dep + far * (torch.randn(dep.shape, device=dev, generator=g3) * std))
    assert gen.get_offset() == off
