"""The sampling and compositing kernels over the whole sample-count range they are compiled for (run on the MI355X: `pytest -m gpu`).

composite.hip dispatches on C = ceil(S / 64) in {1, 2, 3, 4, 8, 16} (S <= 1024), sampling.hip scans CDF rows of up to 255 weights
in 1 ... 4 chunks per lane and sorts Nc + Nf <= 1024 depths with a register bitonic network (<= 256) or an all-pairs rank sort
(above).  The rest of the suite stays in the corner Nc = 64, Nf <= 192, S <= 256; this file runs every instantiation, both sides of
every dispatch boundary and the padded sample counts in between, the limits included.

  compositing   forward and the backward of all four maps at once against oracle.composite in float64 (+ autograd), on a mild
                family and on a `surface` family (opaque runs, empty space, a zero-width interval: _inputs.composite_envelope_inputs);
                the stated project bounds, forward 2e-5 and gradient 1e-5 max|g|.  The fp32 oracle's own distance from float64 is
                printed next to the kernel's and asserted <= 2e-6, so that inputs whose conditioning ruins the bound show as that.
  resampling    indices against the reference's own sample_pdf (tests/golden/sample_pdf_lengths.npz) with ZERO mismatches, CDF
                ties included; the merged depths bit for bit against torch.sort; z_std within 4 ulp of float64.
  limits        Nc - 1 > 256, Nc + Nf > 1024, 257 bins, S > 1024 raise the library's error, also through run_nerf.render_rays.

The measured errors per (family, S) are printed, and written to $CNERF_RECORD_DIR/sample_envelope.json when that variable names a
directory (it is created); profiles/sample_envelope.json is the copy of the run on the MI355X this file was written against (kernel: forward <= 4.4e-7 of 2e-5, gradient <= 7.8e-7 max|g| of 1e-5; the fp32
oracle on that machine's CPU: <= 2.1e-7 and <= 5.6e-7).
"""
import json
import os

import numpy as np
import pytest
import torch

import _inputs as I
from conftest import golden
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

FAR = 6.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from consistentnerf_amd import ops
    ok, name, cus, lds = ops.device_info(0)
    print(f"device: {name} CUs={cus} LDS/CU={lds}")
    assert ok, f"not a gfx950 device: {name}"
    return torch.device("cuda:0")


def T(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


# ------------------------------------------------------------------------------------------------ 1. compositing
def composite_reference(raw, z, d, noise, white, g, dtype):
    """oracle.composite and the gradient of  sum g_rgb rgb + sum g_depth depth + sum g_acc acc + sum_{b>=1} g_disp disp  in `dtype`
    on the CPU -> (rgb, disp, acc, weights, depth, d_raw) as float64 numpy.  The disp term is evaluated on the rays b >= 1 alone:
    ray 0 has acc == 0, its disp is NaN and must not reach the sum (nor, as 0 * NaN, its gradient)."""
    g_rgb, g_disp, g_acc, g_depth = (T(a).to(dtype) for a in g)
    rawt = T(raw).to(dtype).requires_grad_(True)
    zt, dt = T(z).to(dtype), T(d).to(dtype)
    nt = None if noise is None else T(noise).to(dtype)
    rgb, disp, acc, w, depth = O.composite(rawt, zt, dt, nt, white)
    disp1 = O.composite(rawt[1:], zt[1:], dt[1:], None if nt is None else nt[1:], white)[1]
    loss = (rgb * g_rgb).sum() + (depth * g_depth).sum() + (acc * g_acc).sum() + (disp1 * g_disp[1:]).sum()
    (d_raw,) = torch.autograd.grad(loss, rawt)
    return tuple(a.detach().double().numpy() for a in (rgb, disp, acc, w, depth, d_raw))


def composite_errors(got, ref):
    """-> (forward, backward): the worst forward error in units where the stated bound is 2e-5 (rgb, acc, weights absolute, depth
    over far, disp over max(1, max|disp|) off the NaN rays) and max|d_raw - ref| / max|ref|.  The NaN patterns must agree."""
    rgb, disp, acc, w, depth, d_raw = (np.asarray(a, np.float64) for a in got)
    r_rgb, r_disp, r_acc, r_w, r_depth, r_d = ref
    assert np.array_equal(np.isnan(disp), np.isnan(r_disp)), "disp NaN pattern (acc == 0 rays)"
    assert np.isnan(r_disp[0]) and not np.isnan(r_disp[1:]).any()
    for a in (rgb, acc, w, depth, d_raw):
        assert np.isfinite(a).all()
    ok = ~np.isnan(r_disp)
    e_disp = np.abs(disp[ok] - r_disp[ok]).max() / max(1.0, np.abs(r_disp[ok]).max()) if ok.any() else 0.0
    fwd = {"rgb_map": np.abs(rgb - r_rgb).max(), "acc_map": np.abs(acc - r_acc).max(), "weights": np.abs(w - r_w).max(),
           "depth_map": np.abs(depth - r_depth).max() / FAR, "disp_map": e_disp}
    return fwd, float(np.abs(d_raw - r_d).max() / np.abs(r_d).max())


RECORD = {}


def _record(key, row):
    RECORD[key] = row
    out_dir = os.environ.get("CNERF_RECORD_DIR")
    if not out_dir:
        return
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sample_envelope.json"), "w") as f:
        json.dump({"bounds": {"forward": 2e-5, "backward_rel_max": 1e-5, "fp32_oracle": 2e-6},
                   "units": "forward: rgb / acc / weights absolute, depth / far, disp / max(1, max|disp|); backward: / max|d_raw|",
                   "cases": RECORD}, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("S", I.ENVELOPE_S)
@pytest.mark.parametrize("family", I.ENVELOPE_FAMILIES)
def test_composite_vs_float64(dev, family, S):
    """cnerf_composite_fwd / cnerf_composite_bwd (all four upstream gradients in one call) against float64, B = 9 rays (a partial
    last workgroup), both backgrounds (density noise with the white one), 4 and 5 raw channels, ray strides 11 and 8."""
    from consistentnerf_amd import ops
    raw, z, d, noise, *g = I.composite_envelope_inputs(family, S)
    B = raw.shape[0]
    rs = np.random.RandomState(S)
    worst = {"fwd": 0.0, "bwd": 0.0, "fwd32": 0.0, "bwd32": 0.0}
    for white in (False, True):
        nz = noise if white else None
        ref = composite_reference(raw, z, d, nz, white, g, torch.float64)
        f32, b32 = composite_errors(composite_reference(raw, z, d, nz, white, g, torch.float32), ref)
        for ch, stride in ((4, 11), (5, 8), (4, 8), (5, 11)):
            raw_k = raw if ch == 4 else np.concatenate([raw, rs.normal(size=(B, S, 1)).astype(np.float32)], -1)
            rays = rs.normal(size=(B, stride)).astype(np.float32)
            rays[:, 3:6] = d
            args = (T(raw_k, dev), T(z, dev), T(rays, dev), None if nz is None else T(nz, dev), white)
            rgb, disp, acc, w, depth = ops.composite_forward(*args)
            d_raw = ops.composite_backward(*args, *(T(a, dev) for a in g))
            assert d_raw.shape == (B, S, ch)
            if ch == 5:
                assert not d_raw[..., 4].any(), "the gradient of the unused fifth channel must be exactly 0"
            fk, bk = composite_errors([a.cpu().numpy() for a in (rgb, disp, acc, w, depth, d_raw[..., :4])], ref)
            print(f"  {family} S={S} white={white} ch={ch} stride={stride}: forward kernel {max(fk.values()):.2e} (fp32 oracle "
                  f"{max(f32.values()):.2e}, bound 2e-5); d_raw kernel {bk:.2e} (fp32 oracle {b32:.2e}, bound 1e-5) max|g|")
            worst = {"fwd": max(worst["fwd"], *fk.values()), "bwd": max(worst["bwd"], bk),
                     "fwd32": max(worst["fwd32"], *f32.values()), "bwd32": max(worst["bwd32"], b32)}
            _record(f"{family}_S{S}", {"kernel_forward": worst["fwd"], "kernel_backward": worst["bwd"],
                                       "fp32_oracle_forward": worst["fwd32"], "fp32_oracle_backward": worst["bwd32"]})
            assert max(f32.values()) <= 2e-6 and b32 <= 2e-6, "the inputs are ill-conditioned: the fp32 oracle itself is off"
            for k, e in fk.items():
                assert e <= 2e-5, f"{k}: {e:.3e} > 2e-5"
            assert bk <= 1e-5, f"d_raw: {bk:.3e} > 1e-5 max|g|"


# ------------------------------------------------------------------------------------------------ 2. resampling
def _margin(z, w, u):
    """min_k |u - cdf_k| with the CDF in float64 (from the fp32 inputs) -> [B, Nf]"""
    p = (w[:, 1:-1] + np.float32(1e-5)).astype(np.float64)
    cdf = np.concatenate([np.zeros((z.shape[0], 1)), np.cumsum(p / p.sum(-1, keepdims=True), -1)], -1)
    return np.abs(u.astype(np.float64)[:, :, None] - cdf[:, None, :]).min(-1)


@pytest.mark.parametrize("tag", ["det", "rand"])
@pytest.mark.parametrize("Nc,Nf", I.RESAMPLE_SHAPES)
def test_resample_lengths(dev, Nc, Nf, tag):
    """cnerf_resample / cnerf_sample_pdf on 13 rows (an all-zero row, a row with a flat CDF run) against the reference's own
    sample_pdf on the same inputs: every chunk count of build_cdf, every branch of aten_row_sum, both sorts."""
    from consistentnerf_amd import ops
    g = golden("sample_pdf_lengths")
    ref_i, ref_s = g[f"{Nc}_{Nf}_{tag}_inds"].astype(np.int64), g[f"{Nc}_{Nf}_{tag}_samples"]
    z, w = I.resample_envelope_inputs(Nc)
    B = z.shape[0]
    u = I.resample_envelope_u(tag, B, Nf)
    zt, wt, ut = T(z, dev), T(w, dev), T(u, dev)
    z_fine, z_std, samples, inds = ops.resample(zt, wt, ut, want_samples=True)
    bins = 0.5 * (zt[:, 1:] + zt[:, :-1])
    s2, i2 = ops.sample_pdf(bins, wt[:, 1:-1].contiguous(), ut, want_inds=True)
    assert torch.equal(s2, samples) and torch.equal(i2, inds), "cnerf_sample_pdf and cnerf_resample disagree"
    safe = _margin(z, w, u) > 1e-5
    mism = inds.cpu().numpy() != ref_i
    print(f"  Nc={Nc} Nf={Nf} {tag}: {int(mism.sum())} index mismatches of {mism.size} ({int((mism & safe).sum())} with margin > 1e-5, "
          f"{int((~safe).sum())} samples within 1e-5 of a CDF entry)")
    assert mism.sum() == 0, f"{int(mism.sum())} index mismatches, {int((mism & safe).sum())} of them with an fp64 margin > 1e-5"
    sk, bn = samples.cpu().numpy(), bins.cpu().numpy()
    ds = np.abs(sk.astype(np.float64) - ref_s)
    print(f"  samples: max|d| {ds[safe].max() if safe.any() else 0.0:.3e} away from ties (bound {2e-5 * FAR:.1e})")
    assert not safe.any() or ds[safe].max() <= 2e-5 * FAR
    assert np.all(sk >= bn.min(-1, keepdims=True)) and np.all(sk <= bn.max(-1, keepdims=True))
    # the kernel sorts values only: the merged depths are torch.sort's, bit for bit (both sorts, duplicates included)
    assert z_fine.shape == (B, Nc + Nf)
    assert torch.equal(z_fine, torch.sort(torch.cat([zt, samples], -1), -1).values)
    # population std (R:415): two passes in fp64 and one rounding
    want = sk.astype(np.float64).std(-1)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    dz = np.abs(z_std.cpu().numpy().astype(np.float64) - want)
    print(f"  z_std: worst {float((dz / ulp).max()):.2f} ulp")
    assert np.all(dz <= 4 * ulp)


@pytest.mark.parametrize("Nc,Nf", [(64, 192), (64, 193), (200, 824)])
def test_merged_depths_with_duplicates(dev, Nc, Nf):
    """Equal keys in both sorts: duplicated coarse depths, and rows of u that are constant (every new sample of the ray the same
    value), take two values, or hit u = 0 / u = 1 — the merged row is torch.sort's bit for bit and loses no element."""
    from consistentnerf_amd import ops
    z, w = I.resample_envelope_inputs(Nc)
    B = z.shape[0]
    z[:, 5:9] = z[:, 4:5]
    z[3] = z[3, 0]
    u = I.resample_envelope_u("rand", B, Nf)
    u[0], u[1], u[2] = 0.5, 0.0, 1.0
    u[4] = np.where(np.arange(Nf) % 2 == 0, u[4, 0], u[4, -1])
    zt = T(z, dev)
    z_fine, z_std, samples, _ = ops.resample(zt, T(w, dev), T(u, dev), want_samples=True)
    assert float(samples[0].min()) == float(samples[0].max()) and float(z_std[0]) == 0.0
    assert torch.equal(z_fine, torch.sort(torch.cat([zt, samples], -1), -1).values)


@pytest.mark.parametrize("Nc,Nf", [(64, 193), (200, 824)])
def test_resample_in_kernel_stream_equals_fed_stream(dev, Nc, Nf):
    """u drawn inside resample_k (rng.hpp) == the same stream drawn by cnerf_uniform_rng and fed as a tensor, on the rank-sort path."""
    from consistentnerf_amd import ops
    z, w = I.resample_envelope_inputs(Nc)
    zt, wt = T(z, dev), T(w, dev)
    rng = ops.RngStream(1234, 8)
    a = ops.resample(zt, wt, None, want_samples=True, rng=rng, Nf=Nf)
    b = ops.resample(zt, wt, ops.uniform_rng(rng, z.shape[0], Nf, dev, 1), want_samples=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("Nc", [1, 2, 3, 257, 1000])
def test_coarse_z_bit_exact_any_count(dev, Nc, perturb, lindisp):
    from consistentnerf_amd import ops
    B = 13
    rays = T(I.ray_batch(B, seed=9), dev)
    tr = O.pytest_uniform((B, Nc)) if perturb else None
    z = ops.coarse_z(rays, Nc, tr.to(dev) if perturb else None, lindisp)
    ref = O.coarse_z(rays[:, 6:7].cpu(), rays[:, 7:8].cpu(), Nc, lindisp, tr)
    assert torch.equal(z.cpu(), ref), f"max diff {float((z.cpu() - ref).abs().max())}"


# ------------------------------------------------------------------------------------------------ 3. the limits raise
def test_limits_raise(dev):
    """Past MAX_NB = 256 CDF entries, MAX_ALL = 1024 merged depths and 1024 samples per ray the entry points return
    CNERF_E_UNSUPPORTED from their argument checks, before any launch, and the Python surface raises."""
    from consistentnerf_amd import ops, run_nerf as R
    from consistentnerf_amd._lib import CnerfError
    from test_gpu_parity import _kwargs, make_model
    B = 5
    rs = np.random.RandomState(0)

    def zw(n):
        return T(np.sort(rs.uniform(2, 6, size=(B, n)), -1).astype(np.float32), dev), T(rs.uniform(size=(B, n)).astype(np.float32), dev)

    z, w = zw(257)                              # the largest admitted CDF: accepted
    assert ops.resample(z, w, torch.rand(B, 4, device=dev))[0].shape == (B, 261)
    z, w = zw(258)
    with pytest.raises(CnerfError, match="cnerf_resample"):
        ops.resample(z, w, torch.rand(B, 4, device=dev))
    with pytest.raises(CnerfError, match="cnerf_resample_rng"):
        ops.resample(z, w, None, rng=ops.RngStream(1, 0), Nf=4)
    z, w = zw(64)
    with pytest.raises(CnerfError, match="cnerf_resample"):
        ops.resample(z, w, torch.rand(B, 961, device=dev))
    with pytest.raises(CnerfError, match="cnerf_resample_rng"):
        ops.resample(z, w, None, rng=ops.RngStream(1, 0), Nf=961)
    bins, wb = zw(257)
    with pytest.raises(CnerfError, match="cnerf_sample_pdf"):
        ops.sample_pdf(bins, wb[:, :256].contiguous(), torch.rand(B, 4, device=dev))
    raw = torch.randn(B, 1025, 4, device=dev)
    z, _ = zw(1025)
    rays = T(I.ray_batch(B, seed=1), dev)
    with pytest.raises(CnerfError, match="cnerf_composite_fwd"):
        ops.composite_forward(raw, z, rays, None, False)
    gr = [torch.randn(B, 3, device=dev)] + [torch.randn(B, device=dev) for _ in range(3)]
    with pytest.raises(CnerfError, match="cnerf_composite_bwd"):
        ops.composite_backward(raw, z, rays, None, False, *gr)
    coarse, fine = make_model(2, 64, True, 5, 1, dev)[0], make_model(2, 64, True, 5, 2, dev)[0]
    with pytest.raises(CnerfError):
        R.render_rays(rays, retraw=True, pytest=True, **_kwargs(coarse, fine, 64, 961, 0.0, False, 0.0, False))
    torch.cuda.synchronize()
