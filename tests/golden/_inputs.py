"""Deterministic, numpy-only input builders shared by the golden-vector generator
(`make_golden.py`, runs only where /root/reference exists) and by the tests (run anywhere).

Everything here is derived from `np.random.RandomState(seed)` (the frozen legacy MT19937
streams), so fixtures only need to store the *outputs* the reference produced.
"""
import numpy as np

SKIPS = (4,)


def embed_channels(multires):
    return 3 + 6 * multires


def nerf_param_shapes(D, W, input_ch, input_ch_views, output_ch, use_viewdirs, skips=SKIPS):
    """(name, shape) list in the reference's state_dict order (run_nerf_helpers.py:67-104)."""
    shapes = [("temp_rgb", (1,)), ("temp_depth", (1,)), ("depth_scale", (1,))]
    shapes += [("pts_linears.0.weight", (W, input_ch)), ("pts_linears.0.bias", (W,))]
    for i in range(D - 1):
        k = W + input_ch if i in skips else W
        shapes += [(f"pts_linears.{i+1}.weight", (W, k)), (f"pts_linears.{i+1}.bias", (W,))]
    shapes += [("views_linears.0.weight", (W // 2, input_ch_views + W)), ("views_linears.0.bias", (W // 2,))]
    if use_viewdirs:
        shapes += [("feature_linear.weight", (W, W)), ("feature_linear.bias", (W,)),
                   ("alpha_linear.weight", (1, W)), ("alpha_linear.bias", (1,)),
                   ("rgb_linear.weight", (3, W // 2)), ("rgb_linear.bias", (3,))]
    else:
        shapes += [("output_linear.weight", (output_ch, W)), ("output_linear.bias", (output_ch,))]
    return shapes


def nerf_state_dict(D, W, multires=10, multires_views=4, output_ch=4, use_viewdirs=True, seed=0,
                    gain=1.0):
    """He-uniform weights (keeps activations O(1) through 8 layers so ReLU masks, sigmoids and
    densities are all exercised), small uniform biases. float32 numpy arrays keyed like the
    reference state_dict."""
    rs = np.random.RandomState(seed)
    input_ch = embed_channels(multires)
    input_ch_views = embed_channels(multires_views) if use_viewdirs else 0
    sd = {}
    for name, shape in nerf_param_shapes(D, W, input_ch, input_ch_views, output_ch, use_viewdirs):
        if name == "temp_rgb" or name == "temp_depth":
            sd[name] = np.full(shape, -0.7, np.float32)
        elif name == "depth_scale":
            sd[name] = np.full(shape, 1.0, np.float32)
        elif name.endswith(".weight"):
            bound = gain * np.sqrt(6.0 / shape[1])
            sd[name] = rs.uniform(-bound, bound, size=shape).astype(np.float32)
        else:
            sd[name] = rs.uniform(-0.1, 0.1, size=shape).astype(np.float32)
    return sd


def ray_batch(B, seed, near=2.0, far=6.0, use_viewdirs=True):
    """[B, 11] = o(3) d(3) near far viewdirs(3) like run_nerf.py:119-125. Cameras on a shell of
    radius ~4 looking roughly at the origin; d is NOT unit length (get_rays-style, |d|>=1)."""
    rs = np.random.RandomState(seed)
    o = rs.normal(size=(B, 3))
    o = 4.0 * o / np.linalg.norm(o, axis=-1, keepdims=True)
    tgt = rs.uniform(-0.8, 0.8, size=(B, 3))
    d = tgt - o
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rs.uniform(1.0, 1.3, size=(B, 1))
    o = o.astype(np.float32)
    d = d.astype(np.float32)
    cols = [o, d, np.full((B, 1), near, np.float32), np.full((B, 1), far, np.float32)]
    if use_viewdirs:
        # float32 arithmetic, exactly like render(): viewdirs = d / ||d|| (run_nerf.py:109)
        import torch
        td = torch.from_numpy(d)
        cols.append((td / torch.norm(td, dim=-1, keepdim=True)).numpy())
    return np.concatenate(cols, -1).astype(np.float32)


def raw2outputs_inputs(B, S, seed, near=2.0, far=6.0):
    rs = np.random.RandomState(seed)
    raw = (rs.normal(size=(B, S, 4)) * 3.0).astype(np.float32)
    # a few rays with all-negative sigma -> acc == 0 -> disp NaN (reference behaviour, R:302)
    raw[:2, :, 3] = -np.abs(raw[:2, :, 3]) - 0.1
    z = np.sort(rs.uniform(near, far, size=(B, S)), -1).astype(np.float32)
    d = rs.normal(size=(B, 3)).astype(np.float32)
    return raw, z, d


def sample_pdf_inputs(B, Nc, seed, near=2.0, far=6.0):
    rs = np.random.RandomState(seed)
    z = np.sort(rs.uniform(near, far, size=(B, Nc)), -1).astype(np.float32)
    bins = (0.5 * (z[:, 1:] + z[:, :-1])).astype(np.float32)            # [B, Nc-1]
    weights = (rs.uniform(size=(B, Nc - 2)) ** 8).astype(np.float32)     # peaky
    weights[:3] = 0.0                                                    # all-zero rows: pdf = uniform via the 1e-5 floor
    return bins, weights


def camera_pose(theta_deg, phi_deg, radius):
    """c2w [3,4] looking at the origin (OpenGL convention: camera looks down -z, y up)."""
    th, ph = np.deg2rad(theta_deg), np.deg2rad(phi_deg)
    c = radius * np.array([np.cos(ph) * np.sin(th), np.sin(ph), np.cos(ph) * np.cos(th)])
    fwd = -c / np.linalg.norm(c)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0])); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    R = np.stack([right, up, -fwd], 1)
    return np.concatenate([R, c[:, None]], 1).astype(np.float32)


def intrinsics(H, W, focal):
    return np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]], np.float32)


def analytic_scene(H, W, K, c2w, sphere_r=1.0, plane_z=-1.5):
    """Depth prior + colours of a unit sphere in front of a plane, seen from c2w.
    Returns depth (distance along the un-normalised get_rays direction, i.e. camera-z depth),
    rgb[H,W,3]. Pure numpy float64 -> float32."""
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(i - K[0, 2]) / K[0, 0], -(j - K[1, 2]) / K[1, 1], -np.ones_like(i)], -1)
    rd = dirs @ c2w[:3, :3].astype(np.float64).T
    ro = c2w[:3, 3].astype(np.float64)
    a = (rd * rd).sum(-1); b = 2 * (rd * ro).sum(-1); c = (ro * ro).sum() - sphere_r ** 2
    disc = b * b - 4 * a * c
    t_s = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    t_s = np.where(t_s > 0, t_s, np.inf)
    # plane y = plane_z (a floor)
    t_p = np.where(np.abs(rd[..., 1]) > 1e-9, (plane_z - ro[1]) / rd[..., 1], np.inf)
    t_p = np.where(t_p > 0, t_p, np.inf)
    t = np.minimum(t_s, t_p)
    t = np.where(np.isfinite(t), t, 8.0)
    P = ro + t[..., None] * rd
    rgb = 0.5 + 0.5 * np.sin(3.0 * P + np.array([0.0, 1.0, 2.0]))
    return t.astype(np.float32), rgb.astype(np.float32)


# ---- the sample-count envelope of the compositing and resampling kernels (tests/test_gpu_sample_envelope.py) -------------------
# every dispatch of composite.hip (C = ceil(S / 64) in {1, 2, 3, 4, 8, 16}), both sides of each boundary, the padded counts between
ENVELOPE_S = (1, 2, 63, 64, 65, 127, 129, 193, 256, 257, 300, 512, 513, 777, 1024)
ENVELOPE_FAMILIES = ("mild", "surface")
# (Nc, Nf): weight rows Nc - 2 on both sides of 8 and of 64 / 128 / 192 (the chunk counts of build_cdf) up to the maximum 255,
# Nc + Nf on both sides of 256 (register bitonic sort / rank sort) up to the maximum 1024
RESAMPLE_SHAPES = ((3, 1), (4, 5), (9, 64), (10, 63), (17, 128), (33, 223), (34, 222), (64, 192), (64, 193), (65, 191), (66, 256),
                   (67, 128), (128, 128), (129, 128), (130, 65), (194, 300), (200, 824), (257, 767), (257, 1))


def composite_envelope_inputs(family, S, B=9, near=2.0, far=6.0):
    """Seeded per (family, S): raw [B,S,4], z [B,S], rays_d [B,3], density noise [B,S] in [0,1) (used with a white background),
    and the four upstream gradients g_rgb [B,3], g_disp / g_acc / g_depth [B] ~ N(0,1).
      mild     raw ~ 3 N(0,1), z sorted uniform in [near, far], rays_d ~ N(0,1)  (raw2outputs_inputs), one density per ray made
               positive so that a ray of one or two samples is not empty
      surface  what a trained network produces: empty space (sigma = -5|N(0,1)| - 0.1) around ONE opaque run per ray of random
               start and length 1 .. max(2, S/4) with sigma = 10^U(0, 3.5) (alpha == 1 in fp32, so the transmittance factor is the
               bare 1e-10), and a zero-width interval z[S/2] == z[S/2 - 1] (what resampling at a CDF tie creates) for S > 3
    Ray 0 has negative density everywhere, noise included: acc == 0 and disp is NaN (R:302); g_disp[0] = 0."""
    assert family in ENVELOPE_FAMILIES
    rs = np.random.RandomState(1000 * (1 + ENVELOPE_FAMILIES.index(family)) + S)
    raw = rs.normal(size=(B, S, 4)) * 3.0
    z = np.sort(rs.uniform(near, far, size=(B, S)), -1)
    d = rs.normal(size=(B, 3))
    if family == "surface":
        raw[..., 3] = -5.0 * np.abs(rs.normal(size=(B, S))) - 0.1
        for b in range(1, B):
            start, length = rs.randint(0, S), rs.randint(1, max(2, S // 4) + 1)
            raw[b, start:start + length, 3] = 10.0 ** rs.uniform(0.0, 3.5, size=raw[b, start:start + length, 3].shape)
        if S > 3:
            z[:, S // 2] = z[:, S // 2 - 1]
    else:
        for b in range(1, B):          # no ray but ray 0 is empty, at any S
            raw[b, b % S, 3] = np.abs(raw[b, b % S, 3]) + 0.1
    raw[0, :, 3] = -np.abs(raw[0, :, 3]) - 1.1
    noise = rs.uniform(size=(B, S))
    g = [rs.normal(size=(B, 3))] + [rs.normal(size=(B,)) for _ in range(3)]
    g[1][0] = 0.0
    return tuple(a.astype(np.float32) for a in [raw, z, d, noise] + g)


def resample_envelope_inputs(Nc, B=13, near=2.0, far=6.0):
    """z [B,Nc] sorted uniform in [near, far] and coarse weights [B,Nc] = uniform^8 (peaky), seeded per Nc; the resampler reads
    weights[:, 1:-1] over the Nc - 1 midpoints of z.  Row 0 is all zero (a uniform pdf through the 1e-5 floor), row 1 is zero on
    [1, Nc//2): a flat run of the CDF whose every entry ties with its neighbour's."""
    rs = np.random.RandomState(5000 + Nc)
    z = np.sort(rs.uniform(near, far, size=(B, Nc)), -1).astype(np.float32)
    w = (rs.uniform(size=(B, Nc)) ** 8).astype(np.float32)
    w[0] = 0.0
    w[1, 1:Nc // 2] = 0.0
    return z, w


def resample_envelope_u(tag, B, Nf):
    """The two streams of the reference's sample_pdf(..., pytest=True): det = linspace(0, 1, Nf) in float64 cast to fp32 (H:224-226,
    u = 1 ties with the last CDF entry on every row), rand = np.random.seed(0); np.random.rand(B, Nf) (H:227-229)."""
    if tag == "det":
        return np.broadcast_to(np.linspace(0., 1., Nf), (B, Nf)).astype(np.float32).copy()
    np.random.seed(0)
    return np.random.rand(B, Nf).astype(np.float32)


# ---- the input range of the warp, hard-mask and encoding kernels (tests/test_gpu_geometry_envelope.py, test_geometry_inputs.py) --
# (H, W, focal): the smallest scenes with several workgroups per pair, ragged last chunks and chunks without an in-bounds pixel
GEOMETRY_SCENES = ((24, 32, 36.0), (37, 53, 58.0), (48, 64, 70.0))
GEOMETRY_TRAIN = (0, 1, 2)            # view 3 is held out: its mask stays zero
# every threshold ladder the tests climb: the default, a fine one, one that stops every chunk at level 0, one that needs more than
# 64 doublings (2^-80 * 2^k reaches the differences of these scenes at k = 68 ... 89, pixel by pixel)
GEOMETRY_THR0 = (0.1, 1e-6, 1e3, 2.0 ** -80)
KMAX = 300                            # warp.hip: the ladder ends there (thr0 * 2^k is +inf in fp32 long before)
NO_LEVEL = KMAX + 1                   # the level of a pixel that is out of bounds or whose |z - D_ref| is not finite
U32 = 2.0 ** -24                      # unit round-off of fp32


def geometry_poses():
    """Four c2w [3,4]: three close views and one 75 degrees round, from which most target pixels project outside the image."""
    return np.stack([camera_pose(0.0, -15.0, 4.0), camera_pose(13.0, -11.0, 4.1), camera_pose(75.0, -14.0, 3.9),
                     camera_pose(-17.0, -19.0, 4.0)])


def geometry_scene(H, W, focal, poses=None, bias_view=1, bias=0.35, fy_ratio=1.07, c_off=(1.37, -0.81)):
    """analytic_scene seen through a camera with fy != fx and a principal point off the centre by a non-integer amount; the depth
    prior of `bias_view` is biased (make_golden.fx_hardmask's trick) so that chunks need threshold doublings.
    -> K [3,3] fp32, poses [N,3,4] fp32, depths [N,H,W] fp32."""
    poses = geometry_poses() if poses is None else np.asarray(poses, np.float32)
    K = np.array([[focal, 0, 0.5 * W + c_off[0]], [0, focal * fy_ratio, 0.5 * H + c_off[1]], [0, 0, 1]], np.float32)
    depths = np.stack([analytic_scene(H, W, K.astype(np.float64), p)[0] for p in poses])
    depths[bias_view] = depths[bias_view] + np.float32(bias)
    return K, poses, depths


def ladder(thr0):
    """thr0 * 2^k for k = 0 .. KMAX, doubled in fp32 as warp.hip and the reference (V:1026-1029) form them -> float64 [KMAX + 1]."""
    r = np.empty(KMAX + 1, np.float32)
    t = np.float32(thr0)
    with np.errstate(over="ignore"):
        for k in range(KMAX + 1):
            r[k] = t
            t = np.float32(2.0) * t
    return r.astype(np.float64)


def ladder_level(diff, thr0):
    """smallest k with diff < thr0 * 2^k; NO_LEVEL where diff is NaN or +inf (no rung, not even +inf, lets it pass)."""
    return np.searchsorted(ladder(thr0), diff, side="right")      # NaN sorts behind +inf


def _w2c64(c2w):
    m = np.eye(4)
    m[:3, :4] = np.asarray(c2w, np.float64)[:3, :4]
    return np.linalg.inv(m)


def project_f64(P, w2c, K, H, W, flip=True):
    """The warp (oracle.warp_points, warp.hip `project`) in float64 -> dict: Xc [N,3], px, py (BEFORE rounding), x, y (rounded
    half to even), inb (strict bounds on the rounded pixel), and err: a first-order bound on the distance of an fp32 evaluation of
    px / py from these (4 roundings per camera coordinate, 3 for K's row, one for the division), used to decide which rows two
    fp32 evaluations may round differently."""
    P, w2c, K = np.asarray(P, np.float64), np.asarray(w2c, np.float64), np.asarray(K, np.float64)
    R, t = w2c[:3, :3], w2c[:3, 3]
    Xc = P @ R.T + t
    S = np.abs(P) @ np.abs(R).T + np.abs(t)                      # sum of |terms| per camera coordinate
    if flip:
        Xc = Xc * np.array([1.0, -1.0, -1.0])
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        zc = Xc[:, 2]
        px, py = (Xc[:, 0] * fx + zc * cx) / zc, (Xc[:, 1] * fy + zc * cy) / zc
        ex = (4 * (fx * S[:, 0] + abs(cx) * S[:, 2]) + 2 * (np.abs(Xc[:, 0]) * fx + np.abs(zc * cx))) / np.abs(zc) \
            + np.abs(px) * (4 * S[:, 2] / np.abs(zc) + 2)
        ey = (4 * (fy * S[:, 1] + abs(cy) * S[:, 2]) + 2 * (np.abs(Xc[:, 1]) * fy + np.abs(zc * cy))) / np.abs(zc) \
            + np.abs(py) * (4 * S[:, 2] / np.abs(zc) + 2)
        x, y = np.rint(px), np.rint(py)
        inb = (x > 0) & (x < W - 1) & (y > 0) & (y < H - 1)
    return dict(Xc=Xc, S=S, px=px, py=py, x=x, y=y, inb=inb, err=U32 * np.maximum(ex, ey))


def pixel_margin(px, py, H, W):
    """Distance in pixels of (px, py) from the nearest rounding tie (x.5) and from the strict border (0.5, W - 1.5, 0.5, H - 1.5)."""
    with np.errstate(all="ignore"):
        tie = np.minimum(np.abs(px - np.floor(px) - 0.5), np.abs(py - np.floor(py) - 0.5))
        edge = np.minimum(np.minimum(np.abs(px - 0.5), np.abs(px - (W - 1.5))), np.minimum(np.abs(py - 0.5), np.abs(py - (H - 1.5))))
    return np.minimum(tie, edge)


def hard_mask_pair_f64(H, W, K, c2w_tgt, c2w_ref, depth_tgt, depth_ref, thr0):
    """The hard-mask rule (V:1008-1041) for ONE (target, reference) pair in float64, per target pixel in row-major order -> dict:
    px, py (projected pixel before rounding), inb, diff = |z - D_ref| (NaN where out of bounds), level (ladder_level, NO_LEVEL
    where out of bounds or not finite) and margin (pixel_margin)."""
    K64 = np.asarray(K, np.float64)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(i - K64[0, 2]) / K64[0, 0], -(j - K64[1, 2]) / K64[1, 1], -np.ones_like(i)], -1).reshape(-1, 3)
    c2w = np.asarray(c2w_tgt, np.float64)
    P = c2w[:3, 3] + np.asarray(depth_tgt, np.float64).reshape(-1, 1) * (dirs @ c2w[:3, :3].T)
    p = project_f64(P, _w2c64(c2w_ref), K64, H, W, True)
    inb = p["inb"]
    diff = np.full(H * W, np.nan)
    yi, xi = p["y"][inb].astype(np.int64), p["x"][inb].astype(np.int64)
    with np.errstate(invalid="ignore"):
        diff[inb] = np.abs(p["Xc"][inb, 2] - np.asarray(depth_ref, np.float64).reshape(H, W)[yi, xi])
    level = np.where(inb, ladder_level(diff, thr0), NO_LEVEL)
    return dict(px=p["px"], py=p["py"], inb=inb, diff=diff, level=level, margin=pixel_margin(p["px"], p["py"], H, W), z=p["Xc"][:, 2])


def chunk_levels(level, chunk):
    """Per chunk of `chunk` consecutive pixels: the smallest level in it (NO_LEVEL: nothing in it can pass) -> int [nchunks]."""
    return np.minimum.reduceat(level, np.arange(0, level.shape[0], chunk))


def hard_masks_f64(H, W, K, poses, depths, i_train, thr0, chunk):
    """oracle.hard_masks restated on hard_mask_pair_f64 -> (masks [N,H,W] bool, {(t, r): fp32 [nchunks] thresholds, NaN for a chunk
    in which nothing can pass}, the largest level any chunk climbed to).  A pixel is set when its level is its chunk's minimum."""
    N = len(poses)
    rungs = ladder(thr0).astype(np.float32)
    masks, thr, deepest = np.zeros((N, H * W), bool), {}, 0
    for t in i_train:
        for r in i_train:
            if r == t:
                continue
            lv = hard_mask_pair_f64(H, W, K, poses[t], poses[r], depths[t], depths[r], thr0)["level"]
            km = chunk_levels(lv, chunk)
            live = km < NO_LEVEL
            masks[t] |= live.repeat(chunk)[:H * W] & (lv == km.repeat(chunk)[:H * W])
            thr[(t, r)] = np.where(live, rungs[np.minimum(km, KMAX)], np.float32(np.nan)).astype(np.float32)
            deepest = max(deepest, int(km[live].max()) if live.any() else 0)
    return masks.reshape(N, H, W), thr, deepest


# |z - D_ref| of two fp32 evaluations differs by the roundings of the target ray (3), the point (2), the camera coordinate (4) and
# the host's fp32 matrix inverse: below 32 u times the scene's extent (camera distance 4 + depth <= 8 -> 12), whatever the rung
DIFF_ABS_MARGIN = 32 * U32 * 12.0


def _undecided(H, W, K, poses, depths, t, r, thr0s):
    q = hard_mask_pair_f64(H, W, K, poses[t], poses[r], depths[t], depths[r], thr0s[0])
    bad = q["margin"] < 1e-3
    for thr0 in thr0s:
        rungs = ladder(thr0)
        rungs = rungs[np.isfinite(rungs)]
        d = np.where(q["inb"], q["diff"], np.inf)
        near = np.abs(d[:, None] - rungs[None, :]) < np.maximum(1e-4 * rungs[None, :], DIFF_ABS_MARGIN)
        bad |= near.any(-1)
    return bad


def condition_hard_mask_inputs(H, W, K, poses, depths, i_train=GEOMETRY_TRAIN, thr0s=GEOMETRY_THR0, max_iter=8, max_share=0.02):
    """The kernel's scalar arithmetic and ATen's matmul are two fp32 evaluations of the same formulas and may disagree on a pixel
    that sits on a decision boundary.  The depth prior is free input: a target pixel's prior is multiplied by 1 + 3e-3 while, for
    any reference view and in float64, its projection is within 1e-3 px of a rounding tie or of the strict border, or its
    |z - D_ref| is within 1e-4 relative (or DIFF_ABS_MARGIN absolute, which matters for rungs below it) of a rung of any ladder in
    `thr0s`.  All pairs at once, to a fixed point: a nudged prior is also the reference prior of the other views.
    -> (depths fp32, dict(iterations, nudged_share per view)); raises if the fixed point needs more than `max_iter` iterations or
    more than `max_share` of a view's pixels are touched."""
    depths = np.array(depths, np.float32)
    touched = np.zeros((len(poses), H * W), bool)
    for it in range(max_iter + 1):
        bad = np.zeros_like(touched)
        for t in i_train:
            for r in i_train:
                if r != t:
                    bad[t] |= _undecided(H, W, K, poses, depths, t, r, thr0s)
        if not bad.any():
            share = touched.mean(-1)
            if share.max() > max_share:
                raise AssertionError(f"conditioning touched {share.max():.2%} of a view's pixels (cap {max_share:.0%})")
            return depths, dict(iterations=it, nudged_share=[float(s) for s in share])
        touched |= bad
        flat = depths.reshape(len(poses), -1)
        flat[bad] = flat[bad] * np.float32(1.0 + 3e-3)
    raise AssertionError(f"conditioning did not reach a fixed point within {max_iter} iterations")


_GEOMETRY_CASES = {}


def geometry_case(idx):
    """Scene `idx` of GEOMETRY_SCENES, conditioned (cached) -> dict(H, W, K, poses, depths, raw_depths, info)."""
    if idx not in _GEOMETRY_CASES:
        H, W, focal = GEOMETRY_SCENES[idx]
        K, poses, raw = geometry_scene(H, W, focal)
        depths, info = condition_hard_mask_inputs(H, W, K, poses, raw)
        _GEOMETRY_CASES[idx] = dict(H=H, W=W, K=K, poses=poses, depths=depths, raw_depths=raw, info=info)
    return _GEOMETRY_CASES[idx]


def geometry_chunks(H, W):
    return (1, 7, 255, 256, 257, 1000, H * W - 1, H * W, H * W + 5, 5120)


def hard_mask_cases():
    """(scene, i_train, chunk, thr0) of the oracle comparison: every chunk size x the two ordinary ladders on every scene (chunk = 1
    only on the smallest scene with two training views: one oracle iteration per pixel and pair), plus the level-0 and the deep
    ladder at a ragged chunk size."""
    out = []
    for s, (H, W, _) in enumerate(GEOMETRY_SCENES):
        for chunk in geometry_chunks(H, W):
            for thr0 in GEOMETRY_THR0[:2]:
                if chunk == 1 and s != 0:
                    continue
                out.append((s, (0, 1) if chunk == 1 else GEOMETRY_TRAIN, chunk, thr0))
        for thr0 in GEOMETRY_THR0[2:]:
            out.append((s, GEOMETRY_TRAIN, 257, thr0))
    return out


WARP_N = (0, 1, 255, 256, 257, 100003)


# shares of the random kinds among the rows that are not scene points.  Around a camera 4 units from the origin, a point 1e-2 away
# is ill-conditioned IN FP32 WORLD COORDINATES (P R^T + t cancels to 1e-2 of its terms: the pixel of a third of them is uncertain
# by more than its distance to a tie), so that kind is kept small: the rows no fp32 evaluation can decide must stay below 2 %
WARP_SCALES = ((1e-2, 0.005), (1.0, 0.05), (1e2, 0.45), (1e4, 0.495))


def warp_envelope_points(case, n=WARP_N[-1], seed=7, view=0, ref=1):
    """World points for warp_points_k, shuffled so that every prefix holds several kinds: the back-projected pixels of `view` of a
    geometry_case, the same mirrored through the reference camera's centre (behind it, yet with the same pixel: the reference
    tests no depth sign), and random points c_ref + s N(0, 1) at the scales s of WARP_SCALES around the reference camera.
    -> P [n,3] fp32, the reference camera's c2w [3,4] fp32 (the caller inverts it in fp32, as the host code does)."""
    H, W, K, poses = case["H"], case["W"], case["K"].astype(np.float64), case["poses"]
    rs = np.random.RandomState(seed)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(i - K[0, 2]) / K[0, 0], -(j - K[1, 2]) / K[1, 1], -np.ones_like(i)], -1).reshape(-1, 3)
    c2w = poses[view].astype(np.float64)
    scene = c2w[:3, 3] + case["depths"][view].reshape(-1, 1).astype(np.float64) * (dirs @ c2w[:3, :3].T)
    c_ref = poses[ref][:3, 3].astype(np.float64)
    parts = [scene, 2 * c_ref - scene]
    rest = max(0, n - 2 * scene.shape[0])
    parts += [c_ref + s * rs.normal(size=(int(np.ceil(rest * share)), 3)) for s, share in WARP_SCALES]
    P = np.concatenate(parts)[:n]
    return P[rs.permutation(P.shape[0])].astype(np.float32), poses[ref]


def warp_decided_rows(P, w2c, K, H, W, flip):
    """project_f64 of the fp32 inputs and the rows on which every fp32 evaluation must round like it: the pixel is further than
    max(1e-3 px, the fp32 error bound of that row) from a tie and from the border.  -> (dict, keep [N] bool)"""
    p = project_f64(P, np.asarray(w2c, np.float64)[:3, :4], K, H, W, flip)
    with np.errstate(invalid="ignore"):
        keep = pixel_margin(p["px"], p["py"], H, W) > np.maximum(1e-3, p["err"])
    return p, keep


# coordinate scales of the encoding range (sample positions up to 4094 are in range) and what goes with every scale
EMBED_SCALES = (1e-3, 1.0, 64.0, 1024.0, 4094.0, 1e5)


def embed_envelope_inputs(scale, L, n=4096, seed=11):
    """[n + edge rows, 3] fp32: uniform in [-scale, scale], plus +-0, subnormals, and the fp32 neighbours of multiples of
    pi/2 * 2^-l (l < L) up to the scale, where sin or cos of the 2^l-fold argument crosses zero or peaks."""
    rs = np.random.RandomState(seed + L)
    x = rs.uniform(-scale, scale, size=(n, 3)).astype(np.float32)
    edge = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38]
    for l in range(L):
        kmax = max(1, int(scale / (np.pi / 2 * 2.0 ** -l)))
        for k in sorted(set([1, 2, 3, 4, kmax // 2 + 1, kmax])):
            v = np.float32(k * np.pi / 2 * 2.0 ** -l)
            edge += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf)), -v]
    e = np.array(edge + [0.0] * (-len(edge) % 3), np.float32).reshape(-1, 3)
    return np.concatenate([x, e])


def embed_f64(x, L):
    """gamma(x) in float64 on the exact arguments: x * 2^l is exact in fp32 (and in float64)."""
    x = np.asarray(x, np.float64)
    parts = [x]
    for l in range(L):
        parts += [np.sin(x * 2.0 ** l), np.cos(x * 2.0 ** l)]
    return np.concatenate(parts, -1)
