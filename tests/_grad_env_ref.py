"""What tests/test_gpu_grad_envelope.py and tests/test_grad_env_cpu.py share: the inputs of every section, float64 restatements of the
input- and camera-gradient kernels (csrc/mlp_igrad.hip, csrc/rays_grad.hip, csrc/camera_grad.hip), fp32 emulations of the per-ray
kernels' summation orders, the derived bounds, and the mutants those bounds must reject.  numpy / torch on the CPU only.

u = 2^-24 is the unit round-off of fp32 (half an ulp, relative) throughout."""
import math

import numpy as np
import torch

import _camera_ref as CR
import _pose_ref as P

U = 2.0 ** -24
F32 = np.float32

# ================================================================================================ A. the per-ray kernels
S_LIST = [1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 1023, 1024]
B_LIST = [1, 4, 5]            # one workgroup is four rays: 5 leaves a ragged one
PAIRS = [(64, 192), (63, 65), (1, 1024), (129, 193), (1023, 1)]


def chain_len(S):
    """h: the additions an element of a per-ray sum passes through at most: the lane's chain of ceil(S / 64) samples (the first one
    onto the zero the accumulator starts with), then the six butterfly levels."""
    return (S + 63) // 64 + 6


def ray_sum_inputs(B, S, seed=0):
    """d_pts, d_dirs [B * S, 3] ~ N(0, 1) with a spread of magnitudes (x 2^U(-6, 6)), z [B, S] in [0.5, 6) -> float32."""
    rs = np.random.RandomState(1000 * S + 10 * B + seed)
    scale = lambda: 2.0 ** rs.uniform(-6, 6, size=(B * S, 1))      # noqa: E731
    d_pts, d_dirs = rs.normal(size=(B * S, 3)) * scale(), rs.normal(size=(B * S, 3)) * scale()
    return d_pts.astype(F32), d_dirs.astype(F32), np.sort(rs.uniform(0.5, 6.0, size=(B, S)), -1).astype(F32)


def norm_inputs(B, S, ch, noisy, ray_stride, seed=0):
    """raw, d_raw [B, S, ch], noise [B, S] | None, rays [B, ray_stride] whose directions have lengths 10^U(-3, 3) -> float32.
    Planted in the noisy form: on ray 0, samples 0 / 1 / 2 (and 64 / 65 / 66, the lanes' second pass) have sigma + noise exactly 0,
    negative, and -0.0 (sigma = noise = -0.0); every sample of the last ray (B > 1) is gated off."""
    rs = np.random.RandomState(2000 * S + 20 * B + 2 * ch + int(noisy) + seed)
    raw, d_raw = rs.normal(size=(B, S, ch)).astype(F32), rs.normal(size=(B, S, ch)).astype(F32)
    noise = rs.normal(size=(B, S)).astype(F32) if noisy else None
    rays = rs.normal(size=(B, ray_stride)).astype(F32)
    d = rs.normal(size=(B, 3))
    rays[:, 3:6] = (d / np.linalg.norm(d, axis=-1, keepdims=True) * 10.0 ** rs.uniform(-3, 3, size=(B, 1))).astype(F32)
    if noisy:
        for s0 in (0, 64):
            if s0 < S:
                raw[0, s0, 3], noise[0, s0] = F32(0.625), F32(-0.625)
            if s0 + 1 < S:
                raw[0, s0 + 1, 3], noise[0, s0 + 1] = F32(0.25), F32(-1.5)
            if s0 + 2 < S:
                raw[0, s0 + 2, 3], noise[0, s0 + 2] = F32(-0.0), F32(-0.0)
        if B > 1:
            raw[B - 1, :, 3] = -np.abs(raw[B - 1, :, 3])
            noise[B - 1] = -np.abs(noise[B - 1])
    return raw, d_raw, noise, rays


def chain32(x, upto=None, drop=None):
    """[B, S] float32 -> [B] float32: the kernels' order.  Lane l adds samples l, l + 64, .. onto 0 in fp32, then six xor-butterfly
    levels (every lane ends with the same bits; the level order does not enter the bound).  Mutants: upto = the loop stops after that
    many samples; drop = one sample index is left out."""
    x = np.asarray(x, F32)
    B, S = x.shape
    if upto is not None:
        x, S = x[:, :upto], min(S, upto)
    if drop is not None:
        x = x.copy()
        x[:, drop] = 0
    pad = np.zeros((B, (S + 63) // 64 * 64), F32)
    pad[:, :S] = x
    acc = np.zeros((B, 64), F32)
    for k in range(pad.shape[1] // 64):
        acc = (acc + pad[:, 64 * k:64 * k + 64]).astype(F32)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, lanes ^ m]).astype(F32)
    return acc[:, 0]


def rays_sums32(d, z=None, **mut):
    """The emulation of rays_level_sums: d [B * S, 3], z [B, S] -> (sum_s d [B, 3], sum_s fl(z d) [B, 3] | None) in float32."""
    B, S = (z.shape if z is not None else mut.pop("shape"))
    d = np.asarray(d, F32).reshape(B, S, 3)
    so = np.stack([chain32(d[:, :, j], **mut) for j in range(3)], -1)
    sd = None if z is None else np.stack([chain32((z * d[:, :, j]).astype(F32), **mut) for j in range(3)], -1)
    return so, sd


def rays_sums64(d, z, B, S):
    """-> (sum, its bound's mass sum|x|, z-sum, its mass sum|z x|), float64 sums of the same fp32 inputs."""
    d = np.asarray(d, np.float64).reshape(B, S, 3)
    zz = None if z is None else np.asarray(z, np.float64)[:, :, None] * d
    return d.sum(1), np.abs(d).sum(1), (None if zz is None else zz.sum(1)), (None if zz is None else np.abs(zz).sum(1))


def bound_sum(S, mass):
    return 1.01 * chain_len(S) * U * mass


def bound_zsum(S, mass):
    return 1.01 * (chain_len(S) + 1) * U * mass      # (+ the rounding of z * x)


NORM_FINISH = 8      # roundings of composite_norm_k's finish, see norm_bound


def norm64(raw, d_raw, noise, rays):
    """-> (d rays_d [B, 3], the bound's mass sum_s |d_raw relu(sigma + noise)| |d_k| / n^2), float64 on the fp32 inputs."""
    sg = np.asarray(raw, np.float64)[:, :, 3] + (0.0 if noise is None else np.asarray(noise, np.float64))
    terms = np.asarray(d_raw, np.float64)[:, :, 3] * np.maximum(sg, 0.0)
    d = np.asarray(rays, np.float64)[:, 3:6]
    n2 = (d * d).sum(-1, keepdims=True)
    return terms.sum(1)[:, None] * d / n2, np.abs(terms).sum(1)[:, None] * np.abs(d) / n2


def norm_bound(S, mass):
    """composite_norm_k, relative to sum_s |d_raw relu(.)| |d_k| / n^2.  Each term carries the roundings of sigma + noise and of the
    product (2) in front of the h additions.  The finish: n^2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) is a sum of non-negative
    numbers, at most 3 roundings on any of them; the square root halves that (1.5) and rounds once (2.5 on n); acc / n rounds once
    (3.5), d_k / n carries n's 2.5 again and rounds once (3.5), the product rounds once: 8.  (Division and square root are
    correctly rounded: the kernels are compiled without the fast-math relaxations.)"""
    return 1.01 * (chain_len(S) + 2 + NORM_FINISH) * U * mass


def norm32(raw, d_raw, noise, rays, gate="sum", **mut):
    """The emulation of norm_level_sum + composite_norm_k's finish in float32.  gate = "sigma": the mutant that forms sigma + noise
    for the value but takes the ReLU decision from sigma alone."""
    sig = np.asarray(raw, F32)[:, :, 3]
    sg = sig if noise is None else (sig + np.asarray(noise, F32)).astype(F32)
    on = (sig if gate == "sigma" else sg) > 0
    acc = chain32((np.asarray(d_raw, F32)[:, :, 3] * np.where(on, sg, F32(0))).astype(F32), **mut)
    d = np.asarray(rays, F32)[:, 3:6]
    n = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + d[:, 2] * d[:, 2]).astype(F32)).astype(F32)
    gn = (acc / n).astype(F32)
    return ((d / n[:, None]).astype(F32) * gn[:, None]).astype(F32)


def pack_rays_ref(o, d, G, vd, dtype):
    """Autograd of sum(G * [o, d, near, far (, d / |d|)]) in `dtype` -> (d_o, d_d) float64."""
    to, td = torch.from_numpy(o).to(dtype).requires_grad_(True), torch.from_numpy(d).to(dtype).requires_grad_(True)
    B = o.shape[0]
    cols = [to, td, torch.full((B, 1), 2.0, dtype=dtype), torch.full((B, 1), 6.0, dtype=dtype)]
    if vd:
        cols.append(td / torch.norm(td, dim=-1, keepdim=True))
    (torch.cat(cols, -1) * torch.from_numpy(G).to(dtype)).sum().backward()
    return to.grad.double(), td.grad.double()


def pack_rays_inputs(B, vd, seed=0):
    rs = np.random.RandomState(3000 + B + seed)
    d = rs.normal(size=(B, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * 10.0 ** rs.uniform(-3, 3, size=(B, 1))
    return rs.normal(size=(B, 3)).astype(F32), d.astype(F32), rs.normal(size=(B, 11 if vd else 8)).astype(F32)


def pack_rays_closed64(d, G, vd):
    """The float64 restatement of pack_rays_bwd_k: d_o = g[0:3], d_d = g[3:6] + (g_v - v (v . g_v)) / |d|."""
    d, G = np.asarray(d, np.float64), np.asarray(G, np.float64)
    out = G[:, 3:6].copy()
    if vd:
        n = np.linalg.norm(d, axis=-1, keepdims=True)
        v = d / n
        out += (G[:, 8:11] - v * (v * G[:, 8:11]).sum(-1, keepdims=True)) / n
    return G[:, 0:3].copy(), out


# ================================================================================================ B. mlp_igrad_k
def embed_dim(L):
    return 3 if L < 0 else 3 + 6 * L


# (D, W, L, Ld, use_viewdirs, output_ch, M).  Every L in {10, 7, 5, 4, -1} meets every W in {64, 128, 256} (the one- and two-tile
# Jacobians behind GEMMs of 8, 16 and 32 K-groups), every Ld in {4, 2, -1} and "no view directions" is met, (8, 256) and (8, 64)
# carry the skip term, and every M in {1, 31, 32, 33, 481} occurs; not the full product.
IGRAD_CASES = [
    (2, 64, 10, 4, True, 4, 33), (2, 64, 7, 2, True, 4, 481), (2, 64, 5, -1, True, 4, 31), (2, 64, 4, 4, False, 5, 32), (2, 64, -1, 2, True, 4, 1),
    (4, 128, 10, 2, True, 4, 31), (4, 128, 7, -1, True, 4, 33), (4, 128, 5, 4, True, 4, 481), (4, 128, 4, 2, True, 4, 1), (4, 128, -1, 4, False, 4, 32),
    (8, 256, 10, -1, True, 4, 32), (8, 256, 7, 4, True, 4, 1), (8, 256, 5, 2, True, 4, 33), (8, 256, 4, -1, True, 4, 481), (8, 256, -1, 4, True, 4, 31),
    (8, 64, 10, 4, True, 4, 481), (8, 64, 7, 4, False, 4, 33), (8, 64, 5, 2, True, 4, 32), (8, 64, 4, 4, True, 4, 31), (8, 64, -1, -1, True, 4, 1),
]
IGRAD_SHAPES = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 481: (37, 13)}      # M -> (B, S), S > 1 where M allows


def igrad_tensor_shapes(D, W, L, Ld, vd, och, skip=4):
    """The parameter shapes in the C-ABI order (include/cnerf.h), as cnerf_tensor_shape gives them."""
    in_ch, dir_ch = embed_dim(L), (embed_dim(Ld) if vd else 0)
    out = []
    for l in range(D):
        out += [(W, in_ch if l == 0 else (W + in_ch if (0 <= skip and skip + 1 < D and l == skip + 1) else W)), (W,)]
    out += [(W // 2, W + dir_ch), (W // 2,)]
    out += ([(W, W), (W,), (1, W), (1,), (3, W // 2), (3,)] if vd else [(och, W), (och,)])
    return out


def igrad_params(shapes, seed=11):
    """He-uniform weights, biases ~ U(-0.1, 0.1), float32."""
    rs = np.random.RandomState(seed)
    return [(rs.uniform(-1, 1, size=s) * (np.sqrt(6.0 / s[1]) if len(s) == 2 else 0.1)).astype(F32) for s in shapes]


def igrad_points(B, S, seed=5):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-3, 3, size=(B, S, 3)).astype(F32)
    dirs = rs.normal(size=(B, 3))
    return pts, (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(F32)


def enc_coef_partner(ch):
    """Per encoding column c < ch: (coordinate j, partner column | -1, coefficient): enc_col of the kernel."""
    out = []
    for c in range(ch):
        if c < 3:
            out.append((c, -1, 1.0))
        else:
            k, r = divmod(c - 3, 6)
            out.append((r, c + 3, 2.0 ** k) if r < 3 else (r - 3, c - 3, -(2.0 ** k)))
    return out


IGRAD_JAC = 24      # roundings of enc_jacobian on top of the GEMM chain, see igrad_bound


def igrad_bound(dZs, Ws, gamma, ch):
    """Elementwise bound of d_x[j] for one encoding: dZs / Ws = the one or two (dZ [M, K], W [K, ch]) pairs whose products add up to
    d gamma, gamma [M, >= ch] the stashed encoding.
        |err_j| <= 1.01 (K_total + 24) u sum_c |coef_c gamma_partner_c| (|dZ| @ |W|)_c
    d gamma[c] is ONE fp32 MFMA accumulator chain over all K_total = sum K contracted features (the skip GEMM continues on the
    accumulators of the layer-0 GEMM): K_total additions of exact-product terms.  enc_jacobian: per column the two products
    coef * gamma (exact: a power of two) * d gamma (1 rounding), then the lane's chain — a coordinate owns at most 21 columns of
    the 63, split over the two half-waves, every one of the 32 register slots of a lane adds (a zero for the other coordinates, which
    rounds nothing): at most 21 roundings on a term, and the half-wave add: 1 + 21 + 1 = 23 <= 24, the count the bound is stated with."""
    mass = np.zeros((gamma.shape[0], ch))
    K = 0
    for dZ, W in zip(dZs, Ws):
        mass += np.abs(np.asarray(dZ, np.float64)) @ np.abs(np.asarray(W, np.float64))
        K += W.shape[0]
    out = np.zeros((gamma.shape[0], 3))
    g = np.abs(np.asarray(gamma, np.float64))
    for c, (j, pc, coef) in enumerate(enc_coef_partner(ch)):
        out[:, j] += abs(coef) * (g[:, pc] if pc >= 0 else 1.0) * mass[:, c]
    return 1.01 * (K + IGRAD_JAC) * U * out


def igrad_mutant(kind, dZ0, W0, enc, L, dZ_skip=None, W_skip_x=None, band=0):
    """d_pts of a wrong kernel, float64.  enc: the stashed block at its padded width in_chp (what the kernel can address).
      "pad"   the Jacobian runs over all in_chp columns (`on = c < ch` missing) and the padding columns of d gamma are not zero:
              they hold what a GEMM over an unpadded W_0 row would read there, the head of the next row
      "cos"   the sign of the cos-column coefficient is flipped in band `band`
      "skip"  the skip layer's term W_{skip+1}[:, :in_ch]^T dZ_{skip+1} is left out"""
    import _igrad_ref as R
    f = lambda a: np.asarray(a, np.float64)      # noqa: E731
    ch, chp = embed_dim(L), enc.shape[1]
    d_g = f(dZ0) @ f(W0)
    if dZ_skip is not None and kind != "skip":
        d_g = d_g + f(dZ_skip) @ f(W_skip_x)
    if kind == "cos":
        c = 3 + 6 * band + 3
        d_g = d_g.copy()
        d_g[:, c:c + 3] *= -1.0
        return R.enc_jacobian(d_g, f(enc)[:, :ch], L)
    if kind == "skip":
        return R.enc_jacobian(d_g, f(enc)[:, :ch], L)
    assert kind == "pad" and chp > ch
    flat = np.concatenate([f(W0).reshape(-1), np.zeros(chp)])
    over = np.stack([flat[r * ch:r * ch + chp] for r in range(W0.shape[0])])      # [W, in_chp]: row r read past its end
    d_full = f(dZ0) @ over
    d_full[:, :ch] = d_g
    d = R.enc_jacobian(d_g, f(enc)[:, :ch], L)
    gam = np.concatenate([f(enc), np.ones((enc.shape[0], 8))], 1)                  # (a partner past the block: some other column)
    for c in range(ch, chp):
        k, r = divmod(c - 3, 6)
        j, pc, coef = (r, c + 3, 2.0 ** k) if r < 3 else (r - 3, c - 3, -(2.0 ** k))
        d[:, j] += coef * gam[:, min(pc, gam.shape[1] - 1)] * d_full[:, c]
    return d


def igrad_synthetic(D, W, L, M, seed=3):
    """CPU stand-ins for what the GPU test reads back: dZ_0 (and dZ_{skip+1}) ~ N(0, 1) with half the units masked off, W_0 and
    W_{skip+1}[:, :in_ch] He-uniform, the encoding of points in [-3, 3]^3 rounded to float32 at its padded width (zeros behind)."""
    rs = np.random.RandomState(seed + 7 * L + W)
    ch = embed_dim(L)
    chp = (ch + 31) // 32 * 32
    x = rs.uniform(-3, 3, size=(M, 3))
    cols = [x] + [fn(x * 2.0 ** k) for k in range(max(L, 0)) for fn in (np.sin, np.cos)]
    enc = np.zeros((M, chp), F32)
    enc[:, :ch] = np.concatenate(cols, -1)
    dz = lambda: (rs.normal(size=(M, W)) * (rs.uniform(size=(M, W)) < 0.5)).astype(F32)      # noqa: E731
    w = lambda: (rs.uniform(-1, 1, size=(W, ch)) * np.sqrt(6.0 / ch)).astype(F32)             # noqa: E731
    skip = D > 5
    return dz(), w(), enc, (dz() if skip else None), (w() if skip else None)


# ================================================================================================ C. the camera reductions
REAL_CAMERAS = {
    "llff_378x504": (378, 504, [[407.6, 0.0, 250.75], [0.0, 407.6, 190.25], [0.0, 0.0, 1.0]]),
    "blender_800x800": (800, 800, [[1111.1, 0.0, 398.5], [0.0, 1111.1, 401.25], [0.0, 0.0, 1.0]]),
    "full_513x512": (513, 512, [[555.5, 0.0, 254.25], [0.0, 555.5, 257.5], [0.0, 0.0, 1.0]]),
    "k1_19x29": (CR.H1, CR.W1, CR.K1),
}
# name -> (camera, B, n_views, pixels, empty view | None).  pixels: "tail" = the row-major window that ends at the last pixel
# (first = H W - B), "coords" = random pixels with (0, 0) and (H - 1, W - 1) among them, "full" = the whole image.
# B = 4096 / 4097 / 8191 / 8256 are 64 / 65 / 128 / 129 chunks of 64 rays: the last size inside one stage-2 pass, the first one past
# it, and the same around two passes; 513 x 512 is 4104 chunks, past the 4096 the default stage-1 grid covers in one step.
CAMERA_CASES = {
    "b4096_llff_tail_v1": ("llff_378x504", 4096, 1, "tail", None),
    "b4097_llff_coords_v3_empty": ("llff_378x504", 4097, 3, "coords", 1),
    "b8191_blender_tail_v5": ("blender_800x800", 8191, 5, "tail", None),
    "b8256_blender_coords_v3": ("blender_800x800", 8256, 3, "coords", None),
    "b4097_k1_coords_v1": ("k1_19x29", 4097, 1, "coords", None),
    "full_513x512_v5_empty": ("full_513x512", 513 * 512, 5, "full", 3),
}
# (host K?, ndc, use_viewdirs) per case: both K routes, ndc on and off, view directions on and off all occur
CAMERA_MODES = {
    "b4096_llff_tail_v1": [(False, True, True), (True, False, False)],
    "b4097_llff_coords_v3_empty": [(False, True, False), (True, True, True)],
    "b8191_blender_tail_v5": [(False, False, True), (True, True, False)],
    "b8256_blender_coords_v3": [(False, True, True)],
    "b4097_k1_coords_v1": [(False, True, True)],
    "full_513x512_v5_empty": [(False, True, True)],
}


def camera_case(name):
    """-> H, W, K (host lists), n_views, coords [B, 2] int64 (always; the window cases also give first), view [B] | None, first | None, B,
    c2w [n_views, 3, 4] float32 (forward facing)."""
    cam, B, n_views, pixels, empty = CAMERA_CASES[name]
    H, W, K = REAL_CAMERAS[cam]
    rs = np.random.RandomState(sum(map(ord, name)))
    first = None
    if pixels == "coords":
        coords = np.stack([rs.randint(0, H, size=B), rs.randint(0, W, size=B)], -1).astype(np.int64)
        coords[0], coords[B - 1], coords[B // 2] = (0, 0), (H - 1, W - 1), (H - 1, W - 1)
    else:
        first = 0 if pixels == "full" else H * W - B
        coords = P.pixel_coords(H, W, first, B).numpy()
    view = None
    if n_views > 1:      # a random view per ray: the views interleave inside every chunk
        view = rs.choice([q for q in range(n_views) if q != empty], size=B).astype(np.int64)
    return H, W, K, n_views, coords, view, first, B, CR.forward_poses(n_views, 5 + n_views)


def camera_upstream(B, cols, seed=9):
    G = np.random.RandomState(seed).normal(size=(B, cols)).astype(F32)
    G[:, 6:8] = 0
    return G


def rays_at_contrib64(H, W, K, coords, G_o, G_d):
    """gen_rays_at_bwd_k per ray in float64: [B, 12], t[4 r + k] = g_d[r] dir_k, t[4 r + 3] = g_o[r]."""
    jj, ii = coords[:, 0].astype(np.float64), coords[:, 1].astype(np.float64)
    dirs = np.stack([(ii - K[0][2]) / K[0][0], -(jj - K[1][2]) / K[1][1], -np.ones_like(ii)], -1)
    t = np.zeros((coords.shape[0], 3, 4))
    t[:, :, :3] = np.asarray(G_d, np.float64)[:, :, None] * dirs[:, None, :]
    t[:, :, 3] = np.asarray(G_o, np.float64)
    return t.reshape(-1, 12)


def camera_contrib64(H, W, K, c2w, coords, view, G, vd, ndc, device_K=True):
    """camera_rows_bwd_k per ray in float64, the kernel's written formulas (cn_finish_ray_bwd) -> (t [B, 12], k [B, 4] = the
    contributions to d fx, d fy, d cx, d cy).  device_K: the NDC coefficients are functions of K[0][0] and their gradients flow into
    d fx; otherwise (host intrinsics) they are constants."""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ax, ay = -1.0 / (W / (2.0 * fx)), -1.0 / (H / (2.0 * fx))
    B = coords.shape[0]
    pose = np.asarray(c2w, np.float64).reshape(-1, 3, 4)[np.zeros(B, np.int64) if view is None else view]
    R, o = pose[:, :, :3], pose[:, :, 3]
    jj, ii = coords[:, 0].astype(np.float64), coords[:, 1].astype(np.float64)
    dirs = np.stack([(ii - cx) / fx, -(jj - cy) / fy, -np.ones(B)], -1)
    d = (R * dirs[:, None, :]).sum(-1)
    G = np.asarray(G, np.float64)
    g_o, g_d = G[:, 0:3], G[:, 3:6]
    y_o, y_d = g_o.copy(), g_d.copy()
    y_ax = y_ay = np.zeros(B)
    if ndc:
        t = -(1.0 + o[:, 2]) / d[:, 2]
        px, py, pz = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1], o[:, 2] + t * d[:, 2]
        qx, qy = px / pz, py / pz
        y_ax = g_o[:, 0] * qx + g_d[:, 0] * (d[:, 0] / d[:, 2] - qx)
        y_ay = g_o[:, 1] * qy + g_d[:, 1] * (d[:, 1] / d[:, 2] - qy)
        g_px, g_py = ax * (g_o[:, 0] - g_d[:, 0]) / pz, ay * (g_o[:, 1] - g_d[:, 1]) / pz
        g_t = g_px * d[:, 0] + g_py * d[:, 1]
        y_o = np.stack([g_px, g_py, -g_t / d[:, 2]], -1)
        y_d = np.stack([g_px * t + g_d[:, 0] * ax / d[:, 2], g_py * t + g_d[:, 1] * ay / d[:, 2],
                        -g_t * t / d[:, 2] - (g_d[:, 0] * ax * d[:, 0] + g_d[:, 1] * ay * d[:, 1]) / (d[:, 2] * d[:, 2])], -1)
    if vd:
        n = np.linalg.norm(d, axis=-1, keepdims=True)
        v = d / n
        y_d = y_d + (G[:, 8:11] - v * (v * G[:, 8:11]).sum(-1, keepdims=True)) / n
    t12 = np.zeros((B, 3, 4))
    t12[:, :, :3] = y_d[:, :, None] * dirs[:, None, :]
    t12[:, :, 3] = y_o
    g_dir = (R * y_d[:, :, None]).sum(1)      # g_dir[k] = sum_r R[r][k] y_d[r]
    k4 = np.stack([-g_dir[:, 0] * dirs[:, 0] / fx, -g_dir[:, 1] * dirs[:, 1] / fy, -g_dir[:, 0] / fx, g_dir[:, 1] / fy], -1)
    if ndc and device_K:
        k4[:, 0] += (y_ax * ax + y_ay * ay) / fx
    return t12.reshape(B, 12), k4


def reduce_views(t, view, n_views, mutant=None, arg=None):
    """Per-ray records [B, n] -> [n_views, n] (view None: one view), float64.  Mutants of the two-stage reduction:
      "first64"   stage 2 reads only the first 64 chunks (no second pass of the lanes)
      "drop"      the record of chunk `arg` is lost
      "neighbour" ray `arg` is credited to the next view"""
    B = t.shape[0]
    view = np.zeros(B, np.int64) if view is None else view.copy()
    keep = np.ones(B, bool)
    if mutant == "first64":
        keep[64 * 64:] = False
    elif mutant == "drop":
        keep[64 * arg:64 * arg + 64] = False
    elif mutant == "neighbour":
        view[arg] = (view[arg] + 1) % n_views
    out = np.zeros((n_views, t.shape[1]))
    np.add.at(out, view[keep], t[keep])
    return out


def k_matrix(k4):
    """[4] (fx, fy, cx, cy) -> d_K [3, 3]."""
    out = np.zeros((3, 3))
    out[0, 0], out[1, 1], out[0, 2], out[1, 2] = k4
    return out


K_LIVE = [(0, 0), (1, 1), (0, 2), (1, 2)]


def tensor_err(g, g64):
    """The project's measure: max|g - g64| / max|g64|."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def project_bound(err32):
    return max(1e-5, 4.0 * err32)


# ================================================================================================ D. the pose composition
def so3_exp_series(w):
    """Exp(w) with A = sin t / t and B = (1 - cos t) / t^2 as power series in t2 = w . w (12 terms: exact to float64 for t <= 0.1,
    where the first dropped term is below 1e-24 / 25!), for value and autograd at angles at which the closed form's t = sqrt(t2)
    is 0 / 0 or underflows.  Any float dtype."""
    t2 = (w * w).sum(-1)
    A, Bc, term = torch.zeros_like(t2), torch.zeros_like(t2), torch.ones_like(t2)
    for n in range(12):
        A = A + term / float(math.factorial(2 * n + 1))
        Bc = Bc + term / float(math.factorial(2 * n + 2))
        term = term * (-t2)
    K = P.hat(w)
    return torch.eye(3, dtype=w.dtype) + A[:, None, None] * K + Bc[:, None, None] * (K @ K)


SERIES_BELOW = 1e-2      # |w| below this: the series form; the two agree to 1e-12 over 1e-3 .. 1e-1 (test_grad_env_cpu.py)


def pose_compose_ref(c2w0, rot, trans, G, dtype, form=None):
    """-> (c2w, d_rot, d_trans) float64 by autograd in `dtype`; form "series" / "closed", None: by the angle."""
    r, t = torch.from_numpy(rot).to(dtype).requires_grad_(True), torch.from_numpy(trans).to(dtype).requires_grad_(True)
    if form is None:
        form = "series" if float(np.linalg.norm(rot.astype(np.float64), axis=-1).max()) < SERIES_BELOW else "closed"
    E = so3_exp_series(r) if form == "series" else P.so3_exp(r)
    c0 = torch.from_numpy(c2w0).to(dtype)
    c2w = torch.cat([E @ c0[:, :, :3], (c0[:, :, 3] + t)[:, :, None]], -1)
    (c2w * torch.from_numpy(G).to(dtype)).sum().backward()
    return c2w.detach().double(), r.grad.double(), t.grad.double()


def angle32(name):
    """The angles |w| of section D as float32 values."""
    one = np.float32(1.0)
    table = {"1-2^-12": one - F32(2.0 ** -12), "1": one, "1+2^-12": one + F32(2.0 ** -12), "0.5": F32(0.5), "2": F32(2.0),
             "pi-1e-3": F32(math.pi - 1e-3), "pi": F32(math.pi), "pi+1e-3": F32(math.pi + 1e-3), "2pi": F32(2 * math.pi), "10": F32(10.0),
             "1e-3": F32(1e-3), "1e-20": F32(1e-20), "1e-30": F32(1e-30)}
    return table[name]


ANGLES = ["1-2^-12", "1", "1+2^-12", "0.5", "2", "pi-1e-3", "pi", "pi+1e-3", "2pi", "10", "1e-3", "1e-20", "1e-30"]


def t2_32(rot):
    """t2 as pose_compose_k forms it: fl(fl(x x + y y) + z z) per row, float32."""
    r = np.asarray(rot, F32)
    return ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]).astype(F32) + r[:, 2] * r[:, 2]).astype(F32)


def pose_inputs(N, name, axes):
    """c2w0 [N, 3, 4] (random rotations rounded to float32), rot [N, 3] of length angle32(name) along random or coordinate axes, trans,
    G [N, 3, 4] -> float32."""
    rs = np.random.RandomState(100 * N + ANGLES.index(name) + (50 if axes == "aligned" else 0))
    if axes == "aligned":
        ax = np.zeros((N, 3))
        ax[np.arange(N), rs.randint(0, 3, size=N)] = rs.choice([-1.0, 1.0], size=N)
    else:
        ax = rs.normal(size=(N, 3))
        ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    rot = (ax * float(angle32(name))).astype(F32)
    c2w0 = np.stack([np.concatenate([np.linalg.qr(rs.normal(size=(3, 3)))[0], rs.uniform(-2, 2, size=(3, 1))], 1) for _ in range(N)]).astype(F32)
    return c2w0, rot, rs.uniform(-1, 1, size=(N, 3)).astype(F32), rs.normal(size=(N, 3, 4)).astype(F32)


def pose_A32(t2, closed_below=False):
    t2 = F32(t2)
    if t2 < 1 and not closed_below:
        acc = F32(-1.0 / 39916800.0)
        for c in (1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
            acc = F32(F32(c) + F32(t2 * acc))
        return acc
    th = np.sqrt(t2, dtype=F32)
    return F32(np.sin(th, dtype=F32) / th)


def pose_C32(t2, closed_below=False):
    """pose_C of the kernel in float32; closed_below: the mutant that takes the closed form on the series' side too."""
    t2 = F32(t2)
    if t2 < 1 and not closed_below:
        acc = F32(-1.0 / 3991680.0)
        for c in (1.0 / 45360.0, -1.0 / 840.0, 1.0 / 30.0, -1.0 / 3.0):
            acc = F32(F32(c) + F32(t2 * acc))
        return acc
    th = np.sqrt(t2, dtype=F32)
    return F32(F32(np.cos(th, dtype=F32) - F32(np.sin(th, dtype=F32) / th)) / t2)


def pose_bwd32(c2w0, rot, G, closed_below=False):
    """The emulation of pose_compose_bwd_k's d_rot in float32 (its order of operations)."""
    N = rot.shape[0]
    out = np.zeros((N, 3), F32)
    f = F32
    for n in range(N):
        Pm, Gm, w = np.asarray(c2w0[n], F32), np.asarray(G[n], F32), np.asarray(rot[n], F32)
        t2 = f(f(f(w[0] * w[0]) + f(w[1] * w[1])) + f(w[2] * w[2]))
        dE = np.zeros(9, F32)
        for r in range(3):
            for j in range(3):
                dE[3 * r + j] = f(f(f(Gm[r, 0] * Pm[j, 0]) + f(Gm[r, 1] * Pm[j, 1])) + f(Gm[r, 2] * Pm[j, 2]))
        A, Ah = pose_A32(t2, closed_below), pose_A32(f(f(0.25) * t2), closed_below)
        Bc = f(f(f(0.5) * Ah) * Ah)
        C, D = pose_C32(t2, closed_below), f(f(f(0.25) * Ah) * pose_C32(f(f(0.25) * t2), closed_below))
        v = [f(dE[7] - dE[5]), f(dE[2] - dE[6]), f(dE[3] - dE[1])]
        tr = f(f(dE[0] + dE[4]) + dE[8])
        sw = [f(f(f(f(dE[3 * k] + dE[k]) * w[0]) + f(f(dE[3 * k + 1] + dE[3 + k]) * w[1])) + f(f(dE[3 * k + 2] + dE[6 + k]) * w[2]))
              for k in range(3)]
        wv = f(f(f(w[0] * v[0]) + f(w[1] * v[1])) + f(w[2] * v[2]))
        wEw = f(f(0.5) * f(f(f(w[0] * sw[0]) + f(w[1] * sw[1])) + f(w[2] * sw[2])))
        s = f(f(f(C * wv) + f(D * f(wEw - f(t2 * tr)))) - f(f(f(2.0) * Bc) * tr))
        for k in range(3):
            out[n, k] = f(f(f(A * v[k]) + f(Bc * sw[k])) + f(s * w[k]))
    return out


def pose_fwd32(c2w0, rot):
    """The rotation block of a composition carried out in float32 throughout, E = I + A K + Bc (w w^T - t2 I) with Bc through the half
    angle and R = E R0 — the arithmetic pose_compose_k had before it formed the value in fp64 and rounded once.  The mutant of the
    orthogonality bound: 1 - Bc (y^2 + z^2) multiplies Bc's relative error by up to 2 near theta = pi."""
    f = F32
    out = np.zeros((rot.shape[0], 3, 3), F32)
    for n in range(rot.shape[0]):
        x, y, z = (f(v) for v in rot[n])
        t2 = f(f(f(x * x) + f(y * y)) + f(z * z))
        A, Ah = pose_A32(t2), pose_A32(f(f(0.25) * t2))
        Bc = f(f(f(0.5) * Ah) * Ah)
        d = lambda a, b: f(f(1.0) - f(Bc * f(f(a * a) + f(b * b))))                  # noqa: E731
        o = lambda a, b, c, sg: f(f(f(Bc * a) * b) + f(sg) * f(A * c))                  # noqa: E731
        Em = np.array([[d(y, z), o(x, y, z, -1), o(x, z, y, 1)], [o(x, y, z, 1), d(x, z), o(y, z, x, -1)],
                       [o(x, z, y, -1), o(y, z, x, 1), d(x, y)]], F32)
        Pm = np.asarray(c2w0[n], F32)[:, :3]
        for r in range(3):
            for k in range(3):
                out[n, r, k] = f(f(f(Em[r, 0] * Pm[0, k]) + f(Em[r, 1] * Pm[1, k])) + f(Em[r, 2] * Pm[2, k]))
    return out


def orthogonality(R):
    """max |R R^T - I| over a stack of rotations, float64."""
    R = np.asarray(R, np.float64)
    return float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())


def pose_isolating_inputs(name, N=3):
    """Inputs on which d_rot[:, 1] and d_rot[:, 2] are C (w . v) w_k and nothing else: R0 = I, the rotation part of G antisymmetric with
    the single generator v = (v0, 0, 0) (dE + dE^T, tr dE and w^T dE w are exact zeros), w with three non-zero components.  A per-tensor
    measure cannot see pose_C below |w| ~ 0.1 (its whole term is |C| t^2 of A v); these two elements are proportional to it.
    -> c2w0, rot, G float32."""
    rs = np.random.RandomState(7 + ANGLES.index(name))
    ax = rs.uniform(0.4, 1.0, size=(N, 3)) * rs.choice([-1.0, 1.0], size=(N, 3))
    rot = (ax / np.linalg.norm(ax, axis=-1, keepdims=True) * float(angle32(name))).astype(F32)
    c2w0 = np.zeros((N, 3, 4), F32)
    c2w0[:, :, :3] = np.eye(3, dtype=F32)
    G = np.zeros((N, 3, 4), F32)
    v0 = rs.uniform(0.5, 2.0, size=N).astype(F32)
    G[:, 2, 1], G[:, 1, 2] = v0, -v0      # dE[7] - dE[5] = 2 v0
    return c2w0, rot, G


# |err| <= 1.01 * 6 u |C (w . v) w_k| on the series' side: the constant -1/3 (1), the series' last addition (1; the terms behind it are
# below t2 / 10 of the sum and their roundings below u / 4 together), v_0 = dE[7] - dE[5] (exact: both are one product with 1 and two
# additions of zero; their difference of v0 and -v0 is a doubling), w . v (1 product; the other two are zeros), C (w . v) (1), s w_k
# (1), A * 0 + Bc * 0 + . (exact), and 1 for the series' truncation and inner terms.
POSE_ISO_ROUNDINGS = 6


def pose_iso_ref(rot, G):
    """float64: C (w . v) w_k for k = 1, 2 with C from its series below SERIES_BELOW^2 and its closed form above."""
    w = np.asarray(rot, np.float64)
    t2 = (w * w).sum(-1)
    th = np.sqrt(t2)
    with np.errstate(all="ignore"):
        closed = (np.cos(th) - np.sin(th) / th) / t2
    series = sum((-1.0) ** (m + 1) * (2 * m + 2) * t2 ** m / math.factorial(2 * m + 3) for m in range(10))
    C = np.where(th < 0.1, series, closed)
    v0 = 2.0 * np.asarray(G, np.float64)[:, 2, 1]
    return (C * w[:, 0] * v0)[:, None] * w[:, 1:3]
