"""The input- and camera-gradient kernels (csrc/mlp_igrad.hip, csrc/rays_grad.hip, csrc/camera_grad.hip) against float64 over the range
they admit: the paths the feature tests of test_gpu_input_grads / _pose_grads / _camera_grads / _rows_grad do not reach.
tests/_grad_env_ref.py holds the inputs, the float64 restatements, the bounds and the mutants; tests/test_grad_env_cpu.py shows on the
CPU that the restatements equal autograd and that each bound below rejects the mutants aimed at it.  u = 2^-24.

A  rays_igrad_k, composite_norm_k, their *_pair forms and pack_rays_bwd_k ALONE on random inputs, S = 1 ... 1024 (the lanes' strided
   loop: one to sixteen passes, ragged and whole), B = 1, 4, 5 (a ragged workgroup), every output form.  Reference: the float64 sum of
   the same fp32 inputs.  Bounds, elementwise and derived (h = ceil(S / 64) + 6 additions: the lane's chain, six butterfly levels):
     sum_s d_pts      1.01 h u sum|x|              sum_s z d_pts    1.01 (h + 1) u sum|z x|        (the product rounds once)
     composite_norm   1.01 (h + 2 + 8) u sum_s |d_raw relu(sigma + noise)| |d_k| / n^2: per term the roundings of sigma + noise and of
                      the product; the finish counted in the kernel (_grad_env_ref.norm_bound): n^2 is three products and two
                      additions of non-negative numbers (3), the square root halves that and rounds (2.5 on n), acc / n (+1), d_k / n
                      (2.5 + 1), their product (+1) = 8 with correctly rounded division and square root
     a pair           the sum of its two levels' bounds + u |result| (each level rounded, then one addition)
   Planted in the noisy form: sigma + noise exactly 0, negative, -0.0, and a ray whose every sample is gated off (exactly 0 out).
   pack_rays_bwd: float64 autograd of [o, d, near, far, d / |d|] with |d| over 1e-3 ... 1e3, the project's per-tensor measure.
B  mlp_igrad_k isolated from the dgrad in front of it: dZ read back from the workspace, the encodings from the stash, the contraction
   by tests/_igrad_ref.py in float64 on those bits.  |err_j| <= 1.01 (K + 24) u sum_c |coef_c gamma_partner_c| (|dZ| @ |W|)_c, K = W
   (2 W with the skip term: ONE accumulator chain runs through both GEMMs; W / 2 for the view branch); the Jacobian's count read
   from enc_jacobian is 1 + 21 + 1 = 23 <= 24 (_grad_env_ref.igrad_bound).  Encodings L = 10, 7, 5, 4, -1 (63, 45, 33, 27, 3 channels:
   both tile counts with their padding columns) x W = 64, 128, 256, Ld = 4, 2, -1 and none; every one is accepted by the library.
   d_raw scaled by 2^12 and 2^-20 scales every output by exactly that power.
C  gen_rays_at_bwd / camera_rows_bwd past one stage-2 pass (64, 65, 128, 129 chunks) and past the default stage-1 grid (4104 chunks: a
   513 x 512 image in full), with the intrinsics and sizes of real scenes, windows that end at the last pixel, views interleaved in
   every chunk and one left empty.  The project's bound per tensor, max(1e-5, 4 x the float32 restatement's error); each live entry of
   d_K also relative to itself; bits equal across a repeated call and grid = 1, 3, 1024, 2000; guarded buffers at B = 4097.
D  pose_compose / pose_compose_bwd around t2 = 1 (both sides hit), the half angle's threshold, pi, 2 pi, 10, and |w| = 1e-20 / 1e-30
   (t2 underflows; the value is I + K), N = 1, 64, 65, random and coordinate axes; R R^T - I <= 8 u.  pose_C is invisible to a
   per-tensor measure at small angles (its term is |C| t^2 of A v), so one case isolates it: R0 = I and an antisymmetric upstream
   gradient leave d_rot[1], d_rot[2] = C (w . v) w_k alone, held to 1.01 * 6 u elementwise on the series' side (six roundings, counted in
   _grad_env_ref.POSE_ISO_ROUNDINGS); on the closed form's side the figure is printed (its bound would rest on the accuracy of sinf / cosf).
E  test_rays_form_against_float64's comparison once at Nc = 64, Nf = 128 (S = 64 and 192 through the strided loops).

Every figure is printed, and written to $CNERF_RECORD_DIR/grad_envelope.json when that variable names a directory (error, bound,
ratio per entry).  profiles/grad_envelope.json is the MI355X run this file was written against (106 tests in 5.5 s).  The largest
err / bound per section there:
  A  0.21  composite_norm_grad, 5 channels, noise on, S = 1, B = 5 (7.2e-9 against 3.5e-8); rays_input_grad 0.14 (origins, S = 63,
           B = 4), the pairs 0.11 / 0.087 (S = 63 + 65); pack_rays_bwd 0.020 of the 1e-5 floor (2.0e-7, B = 1)
  B  0.034 d_dirs_pt of D2 / W64, L = 5, Ld = -1, M = 31 (6.9e-8 against 2.1e-6); the scalings are exact
  C  0.020 d_K[0][0] relative to itself, 4096 rays of the 378 x 504 camera, device K, ndc, view directions (3.3e-7 against 4 x the
           float32 restatement's 4.1e-6); per tensor at most 0.0067 of the floor (6.7e-8, d_c2w at B = 8256); every grid the same bits
  D  0.10  d_rot at |w| = 2 pi, N = 1 (1.0e-6 of the 1e-5 floor); R R^T - I at most 2.5 u of the 8 (|w| = 2 pi, coordinate axes, N = 65);
           pose_C isolated 0.41 at |w| = 1e-3, 0.40 at 0.5, 0.31 at 1 - 2^-12, and 0.59 .. 0.87 of the same figure on the closed
           form's side (printed)
  E  0.25  d_rays_o 1.19e-4 against 4 x the float32 oracle's 1.19e-4 (d_rays_d 7.9e-5 / 7.9e-5): the oracle's own rounding of o + d z
The thinnest cases are the single-sample and single-ray ones (S = 1, N = 1, B = 1): one element's luck against a bound that counts
every rounding at its worst.  What the bound of D found: with the value formed in fp32, R R^T - I reached 13.3 u at |w| = pi - 1e-3
(12.7 u at pi + 1e-3, 12.1 u at 10, random axes; 9.4 u on a coordinate axis) — E's diagonal 1 - Bc (y^2 + z^2) multiplies Bc's
relative error by up to 2; pose_compose_k now forms Exp(w) R0 in fp64 at the fp32 inputs and rounds once
(tests/test_grad_env_cpu.py::test_mutant_composition_carried_out_in_float32 reproduces both figures on the CPU)."""
import json
import os

import numpy as np
import pytest
import torch

import _camera_ref as CR
import _grad_env_ref as E
import _igrad_ref as IR
from test_gpu_input_grads import _rays_reference, _run_rays
from test_gpu_parity import T, dev, stash_blocks  # noqa: F401  (dev: the device fixture)

pytestmark = pytest.mark.gpu

GUARD, NAN = 64, float("nan")
F32 = np.float32

# ------------------------------------------------------------------------------------------------ the record
RECORD = {}


def _record(section, key, err, bound):
    ratio = 0.0 if err == 0 else (float("inf") if bound == 0 else err / bound)
    RECORD.setdefault(section, {})[key] = {"err": err, "bound": bound, "ratio": ratio}
    out_dir = os.environ.get("CNERF_RECORD_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        worst = {s: max(rows.items(), key=lambda kv: kv[1]["ratio"]) for s, rows in RECORD.items()}
        with open(os.path.join(out_dir, "grad_envelope.json"), "w") as f:
            json.dump({"units": "A, B, D-isolated: the largest elementwise |err| / bound with err and bound of that element; "
                                "C, D, E, pack_rays_bwd: max|g - g64| / max|g64| per tensor against max(1e-5, 4 x the float32 CPU figure)",
                       "worst_ratio": {s: {"case": k, **r} for s, (k, r) in worst.items()}, **RECORD}, f, indent=1, sort_keys=True)
    return ratio


def _elem(section, key, got, ref, bound):
    """Elementwise |got - ref| <= bound; records the element with the largest ratio."""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert got.shape == ref.shape == bound.shape, (key, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), key
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    i = np.unravel_index(np.argmax(r), r.shape)
    ratio = _record(section, key, float(err[i]), float(bound[i]))
    print(f"  {key}: worst element err {err[i]:.3e} / bound {bound[i]:.3e} = {ratio:.3f}")
    assert ratio <= 1.0, f"{key}: err {err[i]:.3e} > bound {bound[i]:.3e} at {i}"


def _tensor(section, key, got, g64, g32):
    """The project's per-tensor measure: max|g - g64| / max|g64| <= max(1e-5, 4 x the float32 CPU evaluation's)."""
    got = got.detach().double().cpu().numpy()
    g64, g32 = np.asarray(g64, np.float64), np.asarray(g32, np.float64)
    assert got.shape == g64.shape, (key, got.shape, g64.shape)
    assert np.isfinite(got).all(), key
    err, err32 = E.tensor_err(got, g64), E.tensor_err(g32, g64)
    bound = E.project_bound(err32)
    ratio = _record(section, key, err, bound)
    print(f"  {key}: err {err:.3e} | float32 CPU {err32:.3e} -> bound {bound:.3e} ({ratio:.3f})")
    assert err <= bound, f"{key}: err {err:.3e} > bound {bound:.3e}"


def _opt(a, dev):
    return None if a is None else T(a, dev)


# ================================================================================================ A. the per-ray kernels alone
@pytest.mark.parametrize("S", E.S_LIST)
def test_a_ray_sums_against_float64(dev, S):
    """ops.rays_input_grad in its three forms: ray_stride None (the per-ray sum of d_dirs alone), 8 (origins and directions) and 11
    (both, the view-direction sum in the last three columns); the near / far columns are written zero."""
    from consistentnerf_amd import ops
    for B in E.B_LIST:
        d_pts, d_dirs, z = E.ray_sum_inputs(B, S)
        so, mo, sd, md = E.rays_sums64(d_pts, z, B, S)
        sv, mv, _, _ = E.rays_sums64(d_dirs, None, B, S)
        tag = f"S {S} B {B}"
        out = ops.rays_input_grad(None, T(d_dirs, dev), None, B, S)
        assert out.shape == (B, 3)
        _elem("A", f"rays_input_grad stride None, {tag}", out, sv, E.bound_sum(S, mv))
        for stride in (8, 11):
            out = ops.rays_input_grad(T(d_pts, dev), T(d_dirs, dev) if stride == 11 else None, T(z, dev), B, S, stride)
            assert out.shape == (B, stride) and not out[:, 6:8].any()
            _elem("A", f"rays_input_grad stride {stride} origins, {tag}", out[:, 0:3], so, E.bound_sum(S, mo))
            _elem("A", f"rays_input_grad stride {stride} directions, {tag}", out[:, 3:6], sd, E.bound_zsum(S, md))
            if stride == 11:
                _elem("A", f"rays_input_grad stride 11 view directions, {tag}", out[:, 8:11], sv, E.bound_sum(S, mv))
        if S == 1:      # one sample: the sums are the inputs
            assert torch.equal(out[:, 0:3].cpu(), T(d_pts).reshape(B, 3))


@pytest.mark.parametrize("S", E.S_LIST)
def test_a_composite_norm_against_float64(dev, S):
    """ops.composite_norm_grad: raw of 4 and 5 channels, rows of 8 and 11 columns, noise off and on with the planted rows."""
    from consistentnerf_amd import ops
    for B in E.B_LIST:
        for ch, noisy, stride in ((4, False, 8), (5, True, 11), (4, True, 8), (5, False, 11)):
            raw, d_raw, noise, rays = E.norm_inputs(B, S, ch, noisy, stride)
            ref, mass = E.norm64(raw, d_raw, noise, rays)
            out = ops.composite_norm_grad(T(d_raw, dev), T(raw, dev), _opt(noise, dev), T(rays, dev))
            assert out.shape == (B, stride) and not out[:, 0:3].any() and not out[:, 6:].any()
            _elem("A", f"composite_norm_grad ch {ch} noise {noisy} stride {stride}, S {S} B {B}", out[:, 3:6], ref, E.norm_bound(S, mass))
            if noisy and B > 1:
                assert not out[B - 1].any() and not ref[B - 1].any(), "a ray whose every sample is gated off"


@pytest.mark.parametrize("S0,S1", E.PAIRS)
def test_a_pairs_against_float64(dev, S0, S1):
    """The *_pair forms against float64 directly (their bit-for-bit comparison with the singles is test_gpu_rows_grad's)."""
    from consistentnerf_amd import ops
    for B in (1, 5):
        p0, v0, z0 = E.ray_sum_inputs(B, S0)
        p1, v1, z1 = E.ray_sum_inputs(B, S1, seed=1)
        a, b = E.rays_sums64(p0, z0, B, S0), E.rays_sums64(p1, z1, B, S1)
        va, vb = E.rays_sums64(v0, None, B, S0), E.rays_sums64(v1, None, B, S1)
        tag = f"S {S0} + {S1} B {B}"
        for stride in (8, 11):
            dirs = stride == 11
            out = ops.rays_input_grad_pair(T(p0, dev), T(v0, dev) if dirs else None, T(z0, dev), T(p1, dev), T(v1, dev) if dirs else None,
                                           T(z1, dev), stride)
            assert out.shape == (B, stride) and not out[:, 6:8].any()
            ref = a[0] + b[0]
            _elem("A", f"rays_input_grad_pair stride {stride} origins, {tag}", out[:, 0:3], ref,
                  E.bound_sum(S0, a[1]) + E.bound_sum(S1, b[1]) + E.U * np.abs(ref))
            ref = a[2] + b[2]
            _elem("A", f"rays_input_grad_pair stride {stride} directions, {tag}", out[:, 3:6], ref,
                  E.bound_zsum(S0, a[3]) + E.bound_zsum(S1, b[3]) + E.U * np.abs(ref))
            if dirs:
                ref = va[0] + vb[0]
                _elem("A", f"rays_input_grad_pair view directions, {tag}", out[:, 8:11], ref,
                      E.bound_sum(S0, va[1]) + E.bound_sum(S1, vb[1]) + E.U * np.abs(ref))
        for noisy0, noisy1, stride in ((False, True, 8), (True, True, 11), (False, False, 11)):
            raw0, g0, n0, rays = E.norm_inputs(B, S0, 4, noisy0, stride)
            raw1, g1, n1, _ = E.norm_inputs(B, S1, 5, noisy1, stride, seed=1)
            (r0, m0), (r1, m1) = E.norm64(raw0, g0, n0, rays), E.norm64(raw1, g1, n1, rays)
            out = ops.composite_norm_grad_pair(T(g0, dev), T(raw0, dev), _opt(n0, dev), T(g1, dev), T(raw1, dev), _opt(n1, dev), T(rays, dev))
            assert out.shape == (B, stride) and not out[:, 0:3].any() and not out[:, 6:].any()
            _elem("A", f"composite_norm_grad_pair noise {noisy0}/{noisy1} stride {stride}, {tag}", out[:, 3:6], r0 + r1,
                  E.norm_bound(S0, m0) + E.norm_bound(S1, m1) + E.U * np.abs(r0 + r1))


@pytest.mark.parametrize("vd", [True, False])
@pytest.mark.parametrize("B", [1, 256, 257])
def test_a_pack_rays_bwd_against_float64(dev, B, vd):
    from consistentnerf_amd import ops
    o, d, G = E.pack_rays_inputs(B, vd)
    (o64, d64), (o32, d32) = E.pack_rays_ref(o, d, G, vd, torch.float64), E.pack_rays_ref(o, d, G, vd, torch.float32)
    d_o, d_d = ops.pack_rays_bwd(T(G, dev), T(d, dev), vd)
    assert torch.equal(d_o.cpu(), T(G)[:, 0:3])
    _tensor("A.pack_rays_bwd", f"d_rays_d, B {B} viewdirs {vd}", d_d, d64, d32)


# ================================================================================================ B. mlp_igrad_k isolated
def _ws_blocks(ws, M, D, W, vd):
    """The dZ blocks a dgrad leaves in its workspace (csrc/geom.hip: logically [Mp][g_rows], tile-major like the stash; columns dZ_0 ..
    dZ_{D-1} of W each, then with view directions dF of W and dZv of W / 2, then 32 for the copy of d_raw) -> {z0 .., hv} float64."""
    Mp, rows = (M + 31) // 32 * 32, D * W + ((W + W // 2) if vd else 0) + 32
    full = ws[:Mp * rows].reshape(Mp // 32, rows // 8, 32, 8).permute(0, 2, 1, 3).reshape(Mp, rows).double().cpu()
    out = {f"z{l}": full[:M, l * W:(l + 1) * W].numpy() for l in range(D)}
    if vd:
        out["hv"] = full[:M, D * W + W:D * W + W + W // 2].numpy()
    assert all(np.isfinite(v).all() for v in out.values())
    return out


def _igrad_run(dev, spec, packed, B, S, stash, G, vd):
    from consistentnerf_amd import ops
    ws = ops.mlp_bwd_workspace(spec, B, S, dev)
    ops.mlp_dgrad(spec, packed, G, B, S, stash, ws)
    return ws, ops.mlp_input_grad(spec, packed, B, S, stash, ws, want_dirs=vd)


@pytest.mark.parametrize("case", E.IGRAD_CASES, ids=lambda c: "D{}W{}_L{}_Ld{}_{}_och{}_M{}".format(c[0], c[1], c[2], c[3], "vd" if c[4] else "novd", c[5], c[6]))
def test_b_mlp_igrad_isolated_against_float64(dev, case):
    from consistentnerf_amd import ops
    D, W, L, Ld, vd, och, M = case
    B, S = E.IGRAD_SHAPES[M]
    spec = ops.NetSpec(D=D, W=W, multires=L, multires_views=Ld, use_viewdirs=vd, output_ch=och, skip=4)
    shapes = E.igrad_tensor_shapes(D, W, L, Ld, vd, och)
    assert [tuple(s) for s in spec.tensor_shapes()] == shapes      # (the library accepts the encoding and sizes its tensors so)
    params = E.igrad_params(shapes)
    packed = ops.pack_weights(spec, [T(p, dev) for p in params])
    pts, dirs = E.igrad_points(B, S)
    raw, stash = ops.mlp_forward(spec, packed, B, S, pts=T(pts, dev), dirs=T(dirs, dev) if vd else None, want_stash=True)
    G = T(np.random.RandomState(17).normal(size=tuple(raw.shape)).astype(F32), dev)
    ws, (d_pts, d_dirs) = _igrad_run(dev, spec, packed, B, S, stash, G, vd)
    assert d_pts.shape == (M, 3) and (d_dirs is None) == (not vd)
    in_ch, in_chp, skip = E.embed_dim(L), (E.embed_dim(L) + 31) // 32 * 32, (5 if D > 5 else None)
    blk, dz = stash_blocks(stash, M, D, W, vd, in_chp=in_chp), _ws_blocks(ws, M, D, W, vd)
    enc = blk["enc"].numpy()
    kw, dZs, Ws = {}, [dz["z0"]], [params[0]]
    if skip is not None:
        kw.update(dZ_skip=dz[f"z{skip}"], W_skip_x=params[2 * skip][:, :in_ch])
        dZs.append(dz[f"z{skip}"]), Ws.append(params[2 * skip][:, :in_ch])
    if vd:
        dir_ch = E.embed_dim(Ld)
        kw.update(dZ_v=dz["hv"], W_v_d=params[2 * D][:, W:W + dir_ch], denc=blk["denc"].numpy(), n_freqs_views=Ld)
    p64, v64 = IR.input_grads(dz["z0"], params[0], enc, L, **kw)
    assert np.abs(p64).max() > 0
    tag = f"D {D} W {W} L {L} Ld {Ld if vd else None} M {M}"
    _elem("B", f"d_pts, {tag}", d_pts, p64, E.igrad_bound(dZs, Ws, enc, in_ch))
    if vd:
        assert np.abs(v64).max() > 0
        _elem("B", f"d_dirs_pt, {tag}", d_dirs, v64, E.igrad_bound([dz["hv"]], [params[2 * D][:, W:W + dir_ch]], blk["denc"].numpy(), dir_ch))
    for e in (12, -20):      # the gates are exact and nothing clamps: a power of two goes straight through
        _, (sp, sv) = _igrad_run(dev, spec, packed, B, S, stash, G * 2.0 ** e, vd)
        assert torch.equal(sp, d_pts * 2.0 ** e), f"d_pts under d_raw * 2^{e}"
        assert not vd or torch.equal(sv, d_dirs * 2.0 ** e), f"d_dirs_pt under d_raw * 2^{e}"


# ================================================================================================ C. the camera reductions
_CAM = {}


def _camera(name):
    if name not in _CAM:
        _CAM[name] = E.camera_case(name)
    return _CAM[name]


_CAM_REF = {}


def _camera_ref(name, vd, ndc, coef_paths):
    """(d_c2w, d_K) float64 autograd of _camera_ref in float64 and in float32, once per module."""
    key = (name, vd, ndc, coef_paths)
    if key not in _CAM_REF:
        H, W, K, n_views, coords, view, first, B, c2w = _camera(name)
        cc, cv = torch.from_numpy(coords), (None if view is None else torch.from_numpy(view))
        if ndc:
            dz = CR.min_abs_dz(H, W, K, c2w, cc, cv)
            assert dz >= 0.5, f"{name}: min |d_z| = {dz:.3f}"
        G = E.camera_upstream(B, 11 if vd else 8)
        _CAM_REF[key] = tuple(tuple(t.numpy() for t in CR.grads(H, W, K, c2w, cc, cv, G, vd, ndc, dt, coef_paths=coef_paths)[1:])
                              for dt in (torch.float64, torch.float32))
    return _CAM_REF[key]


def _pixel_args(dev, name):
    """The device arguments of a case: a window goes in as first / B, a list as coords."""
    H, W, K, n_views, coords, view, first, B, c2w = _camera(name)
    dc = T(coords, dev) if first is None else None
    return dc, _opt(view, dev), (0 if first is None else first), T(c2w.reshape(n_views, 12), dev)


GRIDS = (1, 3, 1024, 2000)


@pytest.mark.parametrize("name", list(E.CAMERA_CASES))
def test_c_camera_rows_bwd_past_one_stage_2_pass(dev, name):
    from consistentnerf_amd import ops
    from consistentnerf_amd.run_nerf_helpers import ndc_coefficients
    H, W, K, n_views, coords, view, first, B, c2w = _camera(name)
    empty = E.CAMERA_CASES[name][4]
    dc, dv, f0, d12 = _pixel_args(dev, name)
    for host_K, ndc, vd in E.CAMERA_MODES[name]:
        (c64, k64), (c32, k32) = _camera_ref(name, vd, ndc, not host_K)
        G = T(E.camera_upstream(B, 11 if vd else 8), dev)
        Kin = K if host_K else T(np.asarray(K, F32), dev)
        coef = ndc_coefficients(H, W, K[0][0]) if (host_K and ndc) else (0., 0.)
        run = lambda grid=0: ops.camera_rows_bwd(G, H, W, Kin, d12, dc, dv, vd, ndc, coef, f0, grid=grid)  # noqa: E731
        d_c2w, d_K = run()
        assert d_c2w.shape == (n_views, 12) and d_K.shape == (3, 3)
        tag = f"{name}, {'host' if host_K else 'device'} K, ndc {ndc}, viewdirs {vd}"
        _tensor("C", f"camera_rows_bwd d_c2w ({tag})", d_c2w, c64, c32)
        _tensor("C", f"camera_rows_bwd d_K ({tag})", d_K, k64, k32)
        got = d_K.double().cpu().numpy()
        for r, c in E.K_LIVE:      # each live entry relative to itself
            err, err32 = abs(got[r, c] - k64[r, c]) / abs(k64[r, c]), abs(k32[r, c] - k64[r, c]) / abs(k64[r, c])
            ratio = _record("C", f"camera_rows_bwd d_K[{r}][{c}] ({tag})", err, E.project_bound(err32))
            print(f"  d_K[{r}][{c}] relative to itself: err {err:.3e} | float32 CPU {err32:.3e} ({ratio:.3f})")
            assert err <= E.project_bound(err32), (tag, r, c)
        dead = np.ones((3, 3), bool)
        for r, c in E.K_LIVE:
            dead[r, c] = False
        assert not got[dead].any() and not k64[dead].any()
        if empty is not None:
            assert not d_c2w[empty].any() and not c64[empty].any() and d_c2w[empty - 1].any()
        again = run()
        assert torch.equal(d_c2w, again[0]) and torch.equal(d_K, again[1])
        for grid in GRIDS:
            a, b = run(grid)
            assert torch.equal(d_c2w, a) and torch.equal(d_K, b), f"grid {grid} changed the bits"


@pytest.mark.parametrize("name", list(E.CAMERA_CASES))
def test_c_gen_rays_at_bwd_past_one_stage_2_pass(dev, name):
    """cnerf_gen_rays_at_bwd = the pose gradient of the rows without NDC and view directions (the origin and direction columns)."""
    from consistentnerf_amd import ops
    H, W, K, n_views, coords, view, first, B, c2w = _camera(name)
    empty = E.CAMERA_CASES[name][4]
    dc, dv, f0, _ = _pixel_args(dev, name)
    (c64, _), (c32, _) = _camera_ref(name, False, False, True)
    G = E.camera_upstream(B, 8)
    G_o, G_d = T(G[:, 0:3], dev), T(G[:, 3:6], dev)
    run = lambda grid=0: ops.gen_rays_at_bwd(G_o, G_d, H, W, K, n_views, dc, dv, f0, grid)  # noqa: E731
    got = run()
    _tensor("C", f"gen_rays_at_bwd d_c2w ({name})", got, c64, c32)
    if empty is not None:
        assert not got[empty].any() and got[empty - 1].any()
    assert torch.equal(got, run())
    for grid in GRIDS:
        assert torch.equal(got, run(grid)), f"grid {grid} changed the bits"


def test_c_guarded_buffers_at_4097(dev):
    """Both C entry points at B = 4097 (65 chunks: the first record of a lane's second pass is the last of the workspace) on outputs
    and a workspace of exactly the queried size inside NaN guard bands: the guards stay NaN, everything between is written, and the
    results equal the ops wrappers'."""
    from consistentnerf_amd import _lib, ops
    from consistentnerf_amd.ops import _p, _stream
    name = "b4097_llff_coords_v3_empty"
    H, W, K, n_views, coords, view, first, B, c2w = _camera(name)
    dc, dv, f0, d12 = _pixel_args(dev, name)
    lib = _lib.load()

    def guarded(n):
        buf = torch.full((GUARD + n + GUARD,), NAN, device=dev)
        return buf, buf[GUARD:GUARD + n]

    def intact(buf, n, what):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{what}: a write outside the buffer"

    Kd = T(np.asarray(K, F32), dev)
    G = T(E.camera_upstream(B, 11), dev)
    nws = lib.cnerf_camera_rows_bwd_ws_floats(B, n_views)
    assert nws == 2 * (12 * n_views + 4) * 65
    (ws_b, ws), (c_b, d_c2w), (k_b, d_K) = guarded(nws), guarded(n_views * 12), guarded(9)
    _lib.check(lib.cnerf_camera_rows_bwd(H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, _p(Kd), _p(d12), n_views, _p(dc), _p(dv), f0, B, 1, 1, _p(G),
                                         _p(d_c2w), _p(d_K), _p(ws), 0, _stream()), "cnerf_camera_rows_bwd")
    intact(ws_b, nws, "workspace"), intact(c_b, n_views * 12, "d_c2w"), intact(k_b, 9, "d_K")
    assert not torch.isnan(ws.view(torch.float64)).any(), "a record that was not written"
    want = ops.camera_rows_bwd(G, H, W, Kd, d12, dc, dv, True, True, (0., 0.), f0)
    assert torch.equal(d_c2w.view(n_views, 12), want[0]) and torch.equal(d_K.view(3, 3), want[1])
    nws = lib.cnerf_gen_rays_at_bwd_ws_floats(B, n_views)
    assert nws == 2 * 12 * n_views * 65
    (ws_b, ws), (c_b, d_c2w) = guarded(nws), guarded(n_views * 12)
    G_o, G_d = G[:, 0:3].contiguous(), G[:, 3:6].contiguous()
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    _lib.check(lib.cnerf_gen_rays_at_bwd(H, W, fx, fy, cx, cy, _p(G_o), _p(G_d), n_views, _p(dc), _p(dv), f0, B, _p(d_c2w), _p(ws), 0,
                                         _stream()), "cnerf_gen_rays_at_bwd")
    intact(ws_b, nws, "workspace"), intact(c_b, n_views * 12, "d_c2w")
    assert not torch.isnan(ws.view(torch.float64)).any(), "a record that was not written"
    assert torch.equal(d_c2w.view(n_views, 12), ops.gen_rays_at_bwd(G_o, G_d, H, W, K, n_views, dc, dv, f0))


@pytest.mark.parametrize("cam", ["llff_378x504", "blender_800x800"])
def test_c_forward_equals_gen_rays_at_real_image_sizes(dev, cam):
    """camera_rows (host K, every {ndc} x {use_viewdirs}) and gen_rays_at against gen_rays of the same pose, bit for bit: the 8256
    pixels up to the last one of the image as a window, and a list with (0, 0) and (H - 1, W - 1) in it, over three views."""
    from consistentnerf_amd import ops
    from consistentnerf_amd.run_nerf_helpers import ndc_coefficients
    H, W, K = E.REAL_CAMERAS[cam]
    n_views, B = 3, 8256
    c2w = CR.forward_poses(n_views, 8)
    d12 = T(c2w.reshape(n_views, 12), dev)
    rs = np.random.RandomState(3)
    coords = np.stack([rs.randint(0, H, size=B), rs.randint(0, W, size=B)], -1).astype(np.int64)
    coords[0], coords[B - 1] = (0, 0), (H - 1, W - 1)
    view = T(rs.randint(0, n_views, size=B).astype(np.int64), dev)
    coef = ndc_coefficients(H, W, K[0][0])
    first = H * W - B
    for dc, f0 in ((None, first), (T(coords, dev), 0)):
        flat = torch.arange(first, first + B, device=dev) if dc is None else dc[:, 0] * W + dc[:, 1]
        for ndc, vd in ((True, True), (False, False), (True, False), (False, True)):
            rows = ops.camera_rows(H, W, K, d12, dc, view, 0.25, 1.5, vd, ndc, coef if ndc else (0., 0.), f0, B)
            o, d = ops.gen_rays_at(H, W, K, d12, dc, view, f0, B)
            for n in range(n_views):
                full = ops.gen_rays(H, W, K, c2w[n], 0.25, 1.5, vd, ndc, dev, coef if ndc else (0., 0.))
                sel = view == n
                assert sel.any() and torch.equal(rows[sel], full[flat[sel]]), (cam, ndc, vd, n)
                if not ndc:
                    assert torch.equal(o[sel], full[flat[sel], 0:3]) and torch.equal(d[sel], full[flat[sel], 3:6]), (cam, n)


# ================================================================================================ D. the pose composition
@pytest.mark.parametrize("axes", ["random", "aligned"])
@pytest.mark.parametrize("name", E.ANGLES)
def test_d_pose_compose_at_its_switch_points(dev, name, axes):
    from consistentnerf_amd import ops
    for N in (1, 64, 65):
        c2w0, rot, trans, G = E.pose_inputs(N, name, axes)
        t2 = E.t2_32(rot)
        if name == "1-2^-12":
            assert (t2 < 1).all(), "the series' side"
        if name == "1+2^-12":
            assert (t2 >= 1).all(), "the closed form's side"
        if name in ("1e-20", "1e-30"):
            assert (t2 < 2.0 ** -126).all() and (np.abs(rot).max(-1) > 0).all()      # t2 underflows, w != 0
        v64, r64, t64 = E.pose_compose_ref(c2w0, rot, trans, G, torch.float64)
        v32, r32, t32 = E.pose_compose_ref(c2w0, rot, trans, G, torch.float32)
        d0, drot = T(c2w0, dev), T(rot, dev)
        c2w = ops.pose_compose(d0, drot, T(trans, dev))
        g_rot, g_trans = ops.pose_compose_bwd(d0, drot, T(G, dev))
        assert c2w.shape == (N, 3, 4) and g_rot.shape == (N, 3) and g_trans.shape == (N, 3)
        tag = f"|w| {name} ({int((t2 < 1).sum())} of {N} on the series' side), {axes} axes, N {N}"
        _tensor("D", f"c2w, {tag}", c2w, v64, v32)
        _tensor("D", f"rotation, {tag}", c2w[:, :, :3], v64[:, :, :3], v32[:, :, :3])
        _tensor("D", f"d_rot, {tag}", g_rot, r64, r32)
        assert torch.equal(g_trans.cpu(), T(G)[:, :, 3])
        R = c2w[:, :, :3].double().cpu()
        ortho = float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max())
        R0 = T(c2w0)[:, :, :3].double()
        ratio = _record("D.orthogonality", tag, ortho, 8 * E.U)
        print(f"  max|R R^T - I| = {ortho:.3e} = {ortho / E.U:.2f} u ({ratio:.3f} of 8 u; R0 itself: "
              f"{float((R0 @ R0.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) / E.U:.2f} u)")
        assert ortho <= 8 * E.U


@pytest.mark.parametrize("name", ["1e-20", "1e-30"])
def test_d_tiny_rotation_is_identity_plus_generator(dev, name):
    """t2 underflows while w != 0: the series branch, not the identity branch.  With R0 = I the value is Exp(w) itself: ones on the
    diagonal and K = [w]x off it, to rounding (A = 1, and Bc x y underflows); d_rot is finite and passes the per-tensor check."""
    from consistentnerf_amd import ops
    c2w0, rot, G = E.pose_isolating_inputs(name, N=65)
    G = (G + np.random.RandomState(5).normal(size=G.shape)).astype(F32)
    c2w = ops.pose_compose(T(c2w0, dev), T(rot, dev), torch.zeros(65, 3, device=dev)).cpu().double().numpy()
    K = E.P.hat(torch.from_numpy(rot).double()).numpy()
    want = np.eye(3)[None] + K
    assert np.isfinite(c2w).all() and (np.abs(c2w[:, :, :3] - want) <= 2 * E.U * np.abs(K)).all()
    assert (c2w[:, [0, 1, 2], [0, 1, 2]] == 1).all() and (np.abs(c2w[:, :, :3] - np.eye(3)[None]).max((1, 2)) > 0).all()
    g_rot, _ = ops.pose_compose_bwd(T(c2w0, dev), T(rot, dev), T(G, dev))
    _, r64, _ = E.pose_compose_ref(c2w0, rot, np.zeros_like(rot), G, torch.float64)
    _, r32, _ = E.pose_compose_ref(c2w0, rot, np.zeros_like(rot), G, torch.float32)
    _tensor("D", f"d_rot at R0 = I, |w| {name}", g_rot, r64, r32)


@pytest.mark.parametrize("name", ["1e-3", "0.5", "1-2^-12", "1+2^-12", "2", "pi", "10"])
def test_d_pose_C_isolated(dev, name):
    """d_rot[1], d_rot[2] = C (w . v) w_k on the isolating inputs, elementwise against float64.  Asserted where t2 < 1 (the series; the
    mutant that takes the closed form at |w| = 1e-3 is off by 2e5 bounds: test_grad_env_cpu.py); printed on the closed form's side."""
    from consistentnerf_amd import ops
    c2w0, rot, G = E.pose_isolating_inputs(name, N=65)
    ref = E.pose_iso_ref(rot, G)
    bound = 1.01 * E.POSE_ISO_ROUNDINGS * E.U * np.abs(ref)
    g_rot, _ = ops.pose_compose_bwd(T(c2w0, dev), T(rot, dev), T(G, dev))
    if (E.t2_32(rot) < 1).all():
        _elem("D.pose_C", f"d_rot[1:3] = C (w . v) w_k, |w| {name}", g_rot[:, 1:3], ref, bound)
    else:
        assert (E.t2_32(rot) >= 1).all()
        got = g_rot[:, 1:3].double().cpu().numpy()
        assert np.isfinite(got).all()
        print(f"  |w| {name} (closed form): worst |err| / (6.06 u |ref|) = {float((np.abs(got - ref) / bound).max()):.3f} (not asserted)")


# ================================================================================================ E. the chain at the workload's sample counts
def test_e_rays_form_at_the_workload_sample_counts(dev):
    """test_rays_form_against_float64's comparison at Nc = 64, Nf = 128: 5 rays, D4 / W128 with view directions, white off, no
    noise — S = 64 and S = 192 through mlp_igrad_k, rays_igrad_k and composite_norm_k, against the oracle on the kernel's masks and
    fine depths, at that test's bound."""
    B, Nc, Nf, arch = 5, 64, 128, (4, 128)
    (o64, d64), (o32, d32) = _rays_reference(dev, True, False, B, Nc, Nf, arch)
    d_o, d_d = _run_rays(dev, True, False, 4096, B, Nc, Nf, arch)
    assert d_o.shape == (B, 3) and d_d.shape == (B, 3)
    _tensor("E", "d_rays_o, Nc 64 Nf 128", d_o, o64, o32)
    _tensor("E", "d_rays_d, Nc 64 Nf 128", d_d, d64, d32)
