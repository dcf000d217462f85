"""tests/_grad_env_ref.py on the CPU: every float64 restatement tests/test_gpu_grad_envelope.py compares a kernel with equals autograd
of the oracle / tests/_pose_ref.py / tests/_camera_ref.py in float64; the fp32 emulations of the per-ray kernels' summation orders
stay inside the derived bounds of section A on that section's inputs (the worst ratio is printed); and every mutant is rejected by
the bound of the section that targets it, on that section's own inputs.  No GPU.

Section B's inputs on the GPU are what the dgrad left in the workspace; here random dZ blocks of the same shapes stand in
(_grad_env_ref.igrad_synthetic)."""
import numpy as np
import pytest
import torch

import _camera_ref as CR
import _grad_env_ref as E
import _igrad_ref as IR
import _pose_ref as P
from oracle import nerf_oracle as O

F32 = np.float32


def _exceeds(got, ref, bound):
    """Largest |got - ref| / bound over the elements (a zero bound with a zero error counts as 0)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


# ================================================================================================ restatements = autograd
def test_ray_sums_restatement_equals_autograd():
    B, S = 3, 70
    d_pts, _, z = E.ray_sum_inputs(B, S)
    o, d = torch.zeros(B, 3, dtype=torch.float64, requires_grad=True), torch.ones(B, 3, dtype=torch.float64, requires_grad=True)
    x = o[:, None, :] + d[:, None, :] * torch.from_numpy(z).double()[:, :, None]
    (x * torch.from_numpy(d_pts).double().reshape(B, S, 3)).sum().backward()
    so, _, sd, _ = E.rays_sums64(d_pts, z, B, S)
    assert np.abs(so - o.grad.numpy()).max() <= 1e-12 * np.abs(so).max() and np.abs(sd - d.grad.numpy()).max() <= 1e-12 * np.abs(sd).max()


@pytest.mark.parametrize("noisy", [False, True])
def test_norm_restatement_equals_autograd_of_the_oracle(noisy):
    """d rays_d of O.composite through dists * |rays_d| = norm64 of the d_raw the same backward produced."""
    B, S = 4, 9
    raw, _, noise, rays = E.norm_inputs(B, S, 4, noisy, 8)
    rays[:, 3:6] = np.random.RandomState(1).uniform(0.3, 1.5, size=(B, 3)).astype(F32)
    rs = np.random.RandomState(2)
    z = torch.from_numpy(np.sort(rs.uniform(2, 2.5, size=(B, S)), -1))
    traw, td = torch.from_numpy(raw).double().requires_grad_(True), torch.from_numpy(rays[:, 3:6]).double().requires_grad_(True)
    rgb, _, acc, _, depth = O.composite(traw, z, td, None if noise is None else torch.from_numpy(noise).double())
    ((rgb * torch.from_numpy(rs.normal(size=(B, 3)))).sum() + (acc * torch.from_numpy(rs.normal(size=B))).sum()
     + (depth * torch.from_numpy(rs.normal(size=B))).sum()).backward()
    got, _ = E.norm64(raw, traw.grad.numpy(), noise, rays)
    ref = td.grad.numpy()
    assert np.abs(ref).max() > 0 and np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()
    if noisy:
        assert not got[B - 1].any() and not ref[B - 1].any()      # the ray whose every sample is gated off


@pytest.mark.parametrize("vd", [True, False])
def test_pack_rays_restatement_equals_autograd(vd):
    o, d, G = E.pack_rays_inputs(257, vd)
    a_o, a_d = E.pack_rays_ref(o, d, G, vd, torch.float64)
    c_o, c_d = E.pack_rays_closed64(d, G, vd)
    assert np.abs(c_o - a_o.numpy()).max() == 0 and np.abs(c_d - a_d.numpy()).max() <= 1e-12 * np.abs(c_d).max()


@pytest.mark.parametrize("ndc,vd,device_K", [(True, True, True), (True, False, False), (False, True, True), (False, False, False)])
def test_camera_restatement_equals_autograd(ndc, vd, device_K):
    """The per-ray records of camera_rows_bwd_k, reduced per view, against float64 autograd of _camera_ref (with host intrinsics the
    coefficient paths are cut: _camera_ref.rows(coef_paths=False)); gen_rays_at_bwd_k's against _pose_ref."""
    H, W, K, n_views, coords, view, first, B, c2w = E.camera_case("b4097_llff_coords_v3_empty")
    coords, view, B = coords[:300], view[:300], 300
    G = E.camera_upstream(B, 11 if vd else 8)
    _, c64, k64 = CR.grads(H, W, K, c2w, torch.from_numpy(coords), torch.from_numpy(view), G, vd, ndc, torch.float64, coef_paths=device_K)
    t, k = E.camera_contrib64(H, W, K, c2w, coords, view, G, vd, ndc, device_K)
    d_c2w, d_K = E.reduce_views(t, view, n_views), E.k_matrix(k.sum(0))
    assert np.abs(d_c2w - c64.numpy()).max() <= 1e-12 * np.abs(d_c2w).max()
    assert np.abs(d_K - k64.numpy()).max() <= 1e-12 * np.abs(d_K).max()
    assert not d_c2w[1].any()      # the empty view
    if not (ndc or vd):
        pose = torch.from_numpy(c2w).double().requires_grad_(True)
        o, d = P.get_rays_at(H, W, K, pose, torch.from_numpy(coords), torch.from_numpy(view))
        ((o * torch.from_numpy(G[:, 0:3]).double()).sum() + (d * torch.from_numpy(G[:, 3:6]).double()).sum()).backward()
        got = E.reduce_views(E.rays_at_contrib64(H, W, K, coords, G[:, 0:3], G[:, 3:6]), view, n_views)
        assert np.abs(got - pose.grad.reshape(n_views, 12).numpy()).max() <= 1e-12 * np.abs(got).max()


def test_the_two_float64_pose_forms_agree():
    """so3_exp_series against _pose_ref.so3_exp (closed form) over |w| = 1e-3 .. 1e-1: value and autograd within 1e-12."""
    worst = 0.0
    for mag in (1e-3, 3e-3, 1e-2, 3e-2, 1e-1):
        rs = np.random.RandomState(int(mag * 1e4))
        ax = rs.normal(size=(5, 3))
        rot = ax / np.linalg.norm(ax, axis=-1, keepdims=True) * mag
        c2w0, _, trans, G = E.pose_inputs(5, "1", "random")
        a = E.pose_compose_ref(c2w0.astype(np.float64), rot, trans.astype(np.float64), G.astype(np.float64), torch.float64, "series")
        b = E.pose_compose_ref(c2w0.astype(np.float64), rot, trans.astype(np.float64), G.astype(np.float64), torch.float64, "closed")
        for x, y in zip(a, b):
            worst = max(worst, float((x - y).abs().max() / y.abs().max()))
    print(f"  series vs closed form, value and autograd, 1e-3 .. 1e-1: {worst:.3e}")
    assert worst <= 1e-12


def test_pose_isolating_reference_equals_autograd():
    """On the isolating inputs d_rot[:, 1:3] of float64 autograd is C (w . v) w_k."""
    for name in ("0.5", "2", "1e-3"):
        c2w0, rot, G = E.pose_isolating_inputs(name)
        _, r64, _ = E.pose_compose_ref(c2w0, rot, np.zeros_like(rot), G, torch.float64, "closed")
        ref = E.pose_iso_ref(rot, G)
        assert np.abs(r64.numpy()[:, 1:3] - ref).max() <= 1e-9 * np.abs(ref).max(), name


@pytest.mark.parametrize("L,W,D", [(10, 64, 2), (7, 128, 8), (5, 256, 8), (4, 64, 2), (-1, 64, 8)])
def test_igrad_bound_holds_for_a_float32_evaluation(L, W, D):
    """_igrad_ref.input_grads in float64 against the same contraction carried out in float32 (numpy's order, not the kernel's: any
    order of K + 24 additions obeys the bound) on the synthetic blocks."""
    dZ0, W0, enc, dZs, Ws = E.igrad_synthetic(D, W, L, 97)
    ch = E.embed_dim(L)
    ref, _ = IR.input_grads(dZ0, W0, enc, L, dZ_skip=dZs, W_skip_x=Ws)
    d_g = dZ0 @ W0 + (dZs @ Ws if dZs is not None else F32(0))
    got = np.zeros((97, 3), F32)
    for c, (j, pc, coef) in enumerate(E.enc_coef_partner(ch)):
        got[:, j] += (F32(coef) * (enc[:, pc] if pc >= 0 else F32(1))) * d_g[:, c]
    bound = E.igrad_bound([dZ0] + ([dZs] if dZs is not None else []), [W0] + ([Ws] if Ws is not None else []), enc, ch)
    r = _exceeds(got, ref, bound)
    print(f"  L {L} W {W}: float32 evaluation at {r:.3f} of the bound")
    assert r <= 1.0


# ================================================================================================ A: emulations inside, mutants outside
def test_emulated_summation_orders_stay_inside_the_derived_bounds():
    worst = {"sum": 0.0, "zsum": 0.0, "norm": 0.0}
    for S in E.S_LIST:
        for B in E.B_LIST:
            d_pts, d_dirs, z = E.ray_sum_inputs(B, S)
            so64, mo, sd64, md = E.rays_sums64(d_pts, z, B, S)
            so, sd = E.rays_sums32(d_pts, z)
            worst["sum"] = max(worst["sum"], _exceeds(so, so64, E.bound_sum(S, mo)))
            worst["zsum"] = max(worst["zsum"], _exceeds(sd, sd64, E.bound_zsum(S, md)))
            for ch, noisy, rs_ in ((4, False, 8), (5, True, 11)):
                raw, d_raw, noise, rays = E.norm_inputs(B, S, ch, noisy, rs_)
                ref, mass = E.norm64(raw, d_raw, noise, rays)
                got = E.norm32(raw, d_raw, noise, rays)
                worst["norm"] = max(worst["norm"], _exceeds(got, ref, E.norm_bound(S, mass)))
                if noisy and B > 1:
                    assert not got[B - 1].any() and not ref[B - 1].any()
    print("  emulation / bound, worst over S x B: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("S", [s for s in E.S_LIST if s > 64])
def test_mutant_sum_stops_after_64_samples(S):
    B = 5
    d_pts, _, z = E.ray_sum_inputs(B, S)
    so64, mo, sd64, md = E.rays_sums64(d_pts, z, B, S)
    so, sd = E.rays_sums32(d_pts, z, upto=64)
    assert _exceeds(so, so64, E.bound_sum(S, mo)) > 1.0 and _exceeds(sd, sd64, E.bound_zsum(S, md)) > 1.0
    raw, d_raw, noise, rays = E.norm_inputs(B, S, 4, True, 8)
    ref, mass = E.norm64(raw, d_raw, noise, rays)
    assert _exceeds(E.norm32(raw, d_raw, noise, rays, upto=64), ref, E.norm_bound(S, mass)) > 1.0


@pytest.mark.parametrize("drop", [192, 64, 0])
def test_mutant_one_sample_dropped_at_193(drop):
    """Sample 192 is the only one of the lanes' fourth pass; every ray must show it (a bound that one ray slips through is loose)."""
    B, S = 5, 193
    d_pts, _, z = E.ray_sum_inputs(B, S)
    so64, mo, sd64, md = E.rays_sums64(d_pts, z, B, S)
    so, sd = E.rays_sums32(d_pts, z, drop=drop)
    assert (np.abs(so - so64) > E.bound_sum(S, mo)).any(-1).all() and (np.abs(sd - sd64) > E.bound_zsum(S, md)).any(-1).all()
    raw, d_raw, noise, rays = E.norm_inputs(B, S, 5, False, 11)
    ref, mass = E.norm64(raw, d_raw, noise, rays)
    live = raw[:, drop, 3] > 0      # (a gated-off sample contributes nothing to drop)
    assert live.any() and (np.abs(E.norm32(raw, d_raw, noise, rays, drop=drop) - ref) > E.norm_bound(S, mass)).any(-1)[live].all()


@pytest.mark.parametrize("S", [1, 65, 192])
def test_mutant_noise_ignored_in_the_relu_gate(S):
    B = 5
    raw, d_raw, noise, rays = E.norm_inputs(B, S, 4, True, 8)
    ref, mass = E.norm64(raw, d_raw, noise, rays)
    assert _exceeds(E.norm32(raw, d_raw, noise, rays, gate="sigma"), ref, E.norm_bound(S, mass)) > 1.0


# ================================================================================================ B: mutants
def _igrad_case(L, W, D, M=97):
    dZ0, W0, enc, dZs, Ws = E.igrad_synthetic(D, W, L, M)
    ch = E.embed_dim(L)
    ref, _ = IR.input_grads(dZ0, W0, enc, L, dZ_skip=dZs, W_skip_x=Ws)
    bound = E.igrad_bound([dZ0] + ([dZs] if dZs is not None else []), [W0] + ([Ws] if Ws is not None else []), enc, ch)
    return dZ0, W0, enc, dZs, Ws, ref, bound


@pytest.mark.parametrize("L", [5, 7])
def test_mutant_padding_columns_not_masked(L):
    dZ0, W0, enc, dZs, Ws, ref, bound = _igrad_case(L, 128, 4)
    assert _exceeds(E.igrad_mutant("pad", dZ0, W0, enc, L, dZs, Ws), ref, bound) > 1.0


@pytest.mark.parametrize("L,band", [(10, 9), (10, 0), (7, 3), (5, 4), (4, 0)])
def test_mutant_cos_coefficient_sign_flipped_in_one_band(L, band):
    dZ0, W0, enc, dZs, Ws, ref, bound = _igrad_case(L, 64, 2)
    assert _exceeds(E.igrad_mutant("cos", dZ0, W0, enc, L, dZs, Ws, band=band), ref, bound) > 1.0


@pytest.mark.parametrize("L,W", [(10, 256), (4, 64), (-1, 64)])
def test_mutant_skip_term_omitted(L, W):
    dZ0, W0, enc, dZs, Ws, ref, bound = _igrad_case(L, W, 8)
    assert _exceeds(E.igrad_mutant("skip", dZ0, W0, enc, L, dZs, Ws), ref, bound) > 1.0


# ================================================================================================ C: mutants
def _camera_setup(name, mode=0):
    H, W, K, n_views, coords, view, first, B, c2w = E.camera_case(name)
    host_K, ndc, vd = E.CAMERA_MODES[name][mode]
    G = E.camera_upstream(B, 11 if vd else 8)
    cc, cv = torch.from_numpy(coords), (None if view is None else torch.from_numpy(view))
    if ndc:
        assert CR.min_abs_dz(H, W, K, c2w, cc, cv) >= 0.5
    _, c64, k64 = CR.grads(H, W, K, c2w, cc, cv, G, vd, ndc, torch.float64, coef_paths=not host_K)
    _, c32, k32 = CR.grads(H, W, K, c2w, cc, cv, G, vd, ndc, torch.float32, coef_paths=not host_K)
    t, k = E.camera_contrib64(H, W, K, c2w, coords, view, G, vd, ndc, not host_K)
    bc, bk = E.project_bound(E.tensor_err(c32, c64)), E.project_bound(E.tensor_err(k32, k64))
    return n_views, view, t, k, c64.numpy(), k64.numpy(), bc, bk


@pytest.mark.parametrize("name", ["b4097_llff_coords_v3_empty", "b8256_blender_coords_v3"])
def test_mutant_stage_2_reads_only_the_first_64_chunks(name):
    """B = 4097 is one chunk past a stage-2 pass: the mutant loses ONE ray, and the project's bound still rejects it."""
    n_views, view, t, k, c64, k64, bc, bk = _camera_setup(name)
    assert E.tensor_err(E.reduce_views(t, view, n_views), c64) <= 1e-12
    assert E.tensor_err(E.reduce_views(t, view, n_views, "first64"), c64) > bc
    assert E.tensor_err(E.k_matrix(E.reduce_views(k, None, 1, "first64")[0]), k64) > bk


@pytest.mark.parametrize("chunk", [0, 64, 127])
def test_mutant_one_chunk_record_dropped_at_8191(chunk):
    n_views, view, t, k, c64, k64, bc, bk = _camera_setup("b8191_blender_tail_v5")
    assert E.tensor_err(E.reduce_views(t, view, n_views, "drop", chunk), c64) > bc
    assert E.tensor_err(E.k_matrix(E.reduce_views(k, None, 1, "drop", chunk)[0]), k64) > bk


@pytest.mark.parametrize("ray", [0, 4095, 8190])
def test_mutant_a_ray_credited_to_the_neighbouring_view(ray):
    n_views, view, t, k, c64, k64, bc, bk = _camera_setup("b8191_blender_tail_v5")
    assert E.tensor_err(E.reduce_views(t, view, n_views, "neighbour", ray), c64) > bc


def test_mutant_ndc_coefficient_path_cut():
    """_camera_ref.rows(coef_paths=False): d_K[0][0] relative to itself, the check of section C that targets it."""
    H, W, K, n_views, coords, view, first, B, c2w = E.camera_case("b4096_llff_tail_v1")
    G = E.camera_upstream(B, 11)
    cc = torch.from_numpy(coords)
    _, _, k64 = CR.grads(H, W, K, c2w, cc, None, G, True, True, torch.float64)
    _, _, k32 = CR.grads(H, W, K, c2w, cc, None, G, True, True, torch.float32)
    _, _, kcut = CR.grads(H, W, K, c2w, cc, None, G, True, True, torch.float64, coef_paths=False)
    rel = lambda a: abs(float(a[0, 0]) - float(k64[0, 0])) / abs(float(k64[0, 0]))      # noqa: E731
    assert rel(kcut) > E.project_bound(rel(k32))


# ================================================================================================ D: the mutant
def test_mutant_pose_C_closed_form_below_the_threshold():
    """|w| = 1e-3 on the isolating inputs: the emulation of pose_compose_bwd_k stays inside 6 u of C (w . v) w_k, the same with
    pose_C's closed form does not (cos t - sin t / t cancels to a few ulps of 1 over t^2 / 3 = 3e-7)."""
    c2w0, rot, G = E.pose_isolating_inputs("1e-3")
    ref = E.pose_iso_ref(rot, G)
    bound = 1.01 * E.POSE_ISO_ROUNDINGS * E.U * np.abs(ref)
    good, bad = E.pose_bwd32(c2w0, rot, G)[:, 1:3], E.pose_bwd32(c2w0, rot, G, closed_below=True)[:, 1:3]
    print(f"  emulation at {_exceeds(good, ref, bound):.3f} of the bound, closed-form mutant at {_exceeds(bad, ref, bound):.3g}")
    assert _exceeds(good, ref, bound) <= 1.0 < _exceeds(bad, ref, bound)
    # the per-tensor measure, for the record: it cannot see the mutant (the reason for the isolating inputs)
    c2w0, rot, _, G = E.pose_inputs(3, "1e-3", "random")
    _, r64, _ = E.pose_compose_ref(c2w0, rot, np.zeros_like(rot), G, torch.float64)
    print(f"  per-tensor err on random inputs: kernel order {E.tensor_err(E.pose_bwd32(c2w0, rot, G), r64):.2e}, "
          f"mutant {E.tensor_err(E.pose_bwd32(c2w0, rot, G, closed_below=True), r64):.2e} (bound 1e-5)")


def test_mutant_composition_carried_out_in_float32():
    """R R^T - I <= 8 u holds for the float64 composition rounded to float32 once at every angle of section D, and rejects the same
    formula carried out in float32 throughout (what the kernel did before this bound was put on it) near theta = pi and at 10."""
    once, all32 = {}, {}
    for name in E.ANGLES:
        for axes in ("random", "aligned"):
            c2w0, rot, trans, G = E.pose_inputs(65, name, axes)
            v64, _, _ = E.pose_compose_ref(c2w0, rot, trans, G, torch.float64)
            once[name] = max(once.get(name, 0.0), E.orthogonality(v64[:, :, :3].float().numpy()) / E.U)
            all32[name] = max(all32.get(name, 0.0), E.orthogonality(E.pose_fwd32(c2w0, rot)) / E.U)
    print("  max|R R^T - I| / u, rounded once | float32 throughout: " + ", ".join(f"{k}: {once[k]:.1f} | {all32[k]:.1f}" for k in E.ANGLES))
    assert max(once.values()) <= 8.0
    assert max(all32[k] for k in ("pi-1e-3", "pi", "pi+1e-3", "10")) > 8.0


def test_the_threshold_angles_land_on_both_sides():
    """In float32, t2 of |w| = 1 - 2^-12 is below 1 (series) and that of 1 + 2^-12 is not (closed form), on random and on coordinate axes."""
    for axes in ("random", "aligned"):
        below = E.t2_32(E.pose_inputs(65, "1-2^-12", axes)[1])
        above = E.t2_32(E.pose_inputs(65, "1+2^-12", axes)[1])
        assert (below < 1).all() and (above >= 1).all()
        for name in ("1e-20", "1e-30"):
            rot = E.pose_inputs(65, name, axes)[1]
            t2 = E.t2_32(rot)      # (1e-40 is a float32 subnormal, 1e-60 is zero)
            assert ((t2 == 0).all() if name == "1e-30" else (t2 < 2.0 ** -126).all()) and (np.abs(rot).max(-1) > 0).all()
