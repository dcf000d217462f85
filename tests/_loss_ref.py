"""Float64 statements of the kernels at the end of the step (csrc/loss.hip + loss_terms.hpp, csrc/adam.hip), the bounds derived for
them, and the input families that tests/test_loss_ref_cpu.py (default run) and tests/test_gpu_loss_envelope.py (MI355X) share.

Every statement takes the kernel's float32 inputs and promotes them exactly; scalars that cross the C ABI as `float` (coef, clip,
grad_scale, temperatures) are float32 values here too (`f32()`), so a reference never differs from its kernel by the rounding of an
argument.  Roundings are counted with u = 2^-24 (one correctly rounded fp32 operation: relative error <= u); k of them in a row are
bounded by gamma(k) = k u / (1 - k u) (Higham's gamma_k >= (1 + u)^k - 1: the count of the derivation, with its second-order terms
inside).  The kernels' sums over rays run in fp64 over fp32 terms: 2^-53 per addition, nothing visible next to u.  An operation whose
result falls under 2^-126 is rounded to a multiple of 2^-149 instead: TINY is that absolute cap, added once per seed element.
"""
import math

import numpy as np
import torch

from oracle import nerf_oracle as O

U = 2.0 ** -24
TINY = 2.0 ** -149
F32_MAX = float(np.finfo(np.float32).max)
F = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(x):
    """A python scalar as the float the C ABI hands to the kernel."""
    return float(np.float32(x))


def f64(a):
    return np.asarray(a, dtype=np.float64)


NEAR, FAR = 1.2, 6.0
COEF = f32(0.2)
SPIKES = (0, 1023, 1024, 16383, 16384)      # + B - 1: rays whose residuals are 10x the typical one (one-ray mutants stay visible at large B)


def spike_rows(B):
    return sorted({i for i in SPIKES if i < B} | {B - 1})


# ================================================================================================ masked colour / depth pair
MASK_KINDS = ("mixed", "ones", "zeros", "odd", None)


def masked_inputs(B, mask_kind, seed=0):
    """-> dict(rgb, tgt [B, 3], depth, prior [B], mask [B] | None) in float32.  Colour residuals N(0, 0.1), depth residuals N(0, 0.15);
    the spike rows carry +-1.0 and +-1.5 and sit in the m == 1 set.  "odd": a tenth of the rays at 0.5 and a tenth at 2.0 (neither set)."""
    rs = np.random.RandomState(7000 + 13 * seed + B % 9973)
    tgt = rs.uniform(size=(B, 3))
    res = rs.normal(0, 0.1, size=(B, 3))
    prior = rs.uniform(NEAR, FAR, size=B)
    dres = rs.normal(0, 0.15, size=B)
    rows = spike_rows(B)
    sign = np.where(np.arange(len(rows)) % 2 == 0, 1.0, -1.0)
    res[rows] = sign[:, None] * np.array([1.0, -1.0, 1.0])
    dres[rows] = 1.5 * sign
    pick = rs.uniform(size=B)
    if mask_kind is None:
        mask = None
    elif mask_kind == "ones":
        mask = np.ones(B)
    elif mask_kind == "zeros":
        mask = np.zeros(B)
    else:
        mask = (pick < 0.55).astype(np.float64)
        if mask_kind == "odd":
            odd = rs.uniform(size=B)
            mask[odd < 0.1] = 0.5
            mask[odd > 0.9] = 2.0
        mask[rows] = 1.0
    return dict(rgb=(tgt + res).astype(F), tgt=tgt.astype(F), depth=(prior + dres).astype(F), prior=prior.astype(F),
                mask=None if mask is None else mask.astype(F))


def global_counts(mask, B):
    """(n1, n0) of a pretended larger batch this one is a shard of: the local set sizes + (1000, 500), as float32."""
    m = np.ones(B) if mask is None else mask
    return np.array([(m == 1).sum() + 1000, (m == 0).sum() + 500], dtype=F)


MASKED_MUTANTS = ("drop_last", "dup_16384", "drop_chunk", "local_counts", "N_for_3N", "w0_no_coef", "depth_seed_m0")


def masked64(rgb, tgt, depth, prior, mask, far=FAR, coef=COEF, counts=None, g_scale=1.0, mutant=None):
    """loss_terms.hpp's statement in float64 -> dict(img, dep, d_rgb [B, 3], d_depth [B] | None, N1, N0):
      img = sum_{m=1} e / (3 N1) [+ coef sum_{m=0} e / (3 N0) iff N0 > 0],  e_i = sum_c (rgb_ic - tgt_ic)^2
      dep = sum_{m=1} r^2 / N1,  r_i = (depth_i - prior_i) / far
      d_rgb_ic = w_m (rgb_ic - tgt_ic), w_1 = g_scale 2 / (3 N1), w_0 = g_scale coef 2 / (3 N0) (0 without N0 > 0), 0 for any other m
      d_depth_i = g_scale (2 / N1) / far r_i on m == 1, else 0.
    N1, N0 = the sizes of the sets {m == 1}, {m == 0}, or `counts` (global: a sharded batch).  0 / 0 and x / 0 give NaN / inf as IEEE
    does.  mutant: one of MASKED_MUTANTS, a wrong kernel the bounds must tell from the right one (test_loss_ref_cpu.py)."""
    B = rgb.shape[0]
    x, y = f64(rgb), f64(tgt)
    m = np.ones(B) if mask is None else f64(mask)
    s1, s0 = m == 1, m == 0
    e = ((x - y) ** 2).sum(1)
    cnt = np.ones(B)                       # how often a ray enters the sums
    if mutant == "drop_last":
        cnt[B - 1] = 0
    elif mutant == "dup_16384":
        cnt[16384] = 2
    elif mutant == "drop_chunk":
        cnt[16384:32768] = 0
    if counts is not None and mutant != "local_counts":
        N1, N0 = np.float64(counts[0]), np.float64(counts[1])
    else:
        N1, N0 = (cnt * s1).sum(), (cnt * s0).sum()
    three = 1.0 if mutant == "N_for_3N" else 3.0
    out = dict(N1=float(N1), N0=float(N0))
    with np.errstate(all="ignore"):
        img = (cnt * s1 * e).sum() / (three * N1)
        if N0 > 0:
            img = img + coef * ((cnt * s0 * e).sum() / (three * N0))
        w1 = np.float64(g_scale) * 2.0 / (three * N1)
        w0 = np.float64(g_scale) * (1.0 if mutant == "w0_no_coef" else coef) * 2.0 / (three * N0) if N0 > 0 else 0.0
        w = np.where(s1, w1, np.where(s0, w0, 0.0))
        d_rgb = w[:, None] * (x - y)
        if mutant == "drop_last":
            d_rgb[B - 1] = 0
        out.update(img=float(img), d_rgb=d_rgb, dep=0.0, d_depth=None)
        if depth is not None:
            r = (f64(depth) - f64(prior)) / far
            wd = np.float64(g_scale) * 2.0 / N1 / far
            sel = (s1 | s0) if mutant == "depth_seed_m0" else s1
            d_depth = np.where(sel, wd * r, 0.0)
            if mutant == "drop_last":
                d_depth[B - 1] = 0
            out.update(dep=float((cnt * s1 * r * r).sum() / N1), d_depth=d_depth)
    return out


def masked_bounds(rgb, tgt, depth, prior, mask, far=FAR, coef=COEF, counts=None, g_scale=1.0):
    """The largest distance of the kernel's four outputs from masked64, same keys.

    img, relative (a mean of non-negative terms keeps the relative bound of its terms): d_c = fl(x - y) [1]; d_c^2 carries it twice
    and rounds [3]; e = (d_0^2 + d_1^2) + d_2^2 adds two roundings of non-negative sums [5]; the fp64 quotient is cast once [6 u].
    With the m == 0 branch the product coef * mean and the sum of the two means round once each [8 u].
    d_rgb, relative per element: w_1 = fl(g_scale * fl(2 / (3 N1))) [2], w_0 = fl(fl(g_scale * coef) * fl(2 / (3 N0))) [3]; x - y [1];
    the product [1]: 5 u (4 u on the m == 1 rays; one bound for both).
    dep cancels: r^ = fl(fl(depth / far) - fl(prior / far)), and each quotient is off by u |.| / far ABSOLUTELY, whatever is left of
    the difference.  |r^ - r| <= a = u (|depth| + |prior|) / far (1 + u) + u |r|.  The term fl(r^ r^) is then within
    t = (2 |r| a + a^2)(1 + u) + u r^2 of r^2; the mean of the t_i over m == 1, (1 + u) for the cast's effect on it, + u dep for the
    cast of the mean itself.
    d_depth per m == 1 ray: wd = fl(fl(g_scale * fl(2 / N1)) / far) [3], the product [1]: |wd| (a (1 + gamma_4) + gamma_4 |r|).
    Off the set the seed is an exact 0: bound 0."""
    ref = masked64(rgb, tgt, depth, prior, mask, far, coef, counts, g_scale)
    B = rgb.shape[0]
    m = np.ones(B) if mask is None else f64(mask)
    s1 = m == 1
    out = dict(img=gamma(8 if ref["N0"] > 0 else 6) * abs(ref["img"]), d_rgb=gamma(5) * np.abs(ref["d_rgb"]) + TINY, dep=0.0, d_depth=None)
    if depth is not None:
        with np.errstate(all="ignore"):
            d, p = f64(depth), f64(prior)
            r = np.abs(d - p) / far
            a = U * (np.abs(d) + np.abs(p)) / far * (1 + U) + U * r
            t = (2 * r * a + a * a) * (1 + U) + U * r * r
            out["dep"] = float((s1 * t).sum() / ref["N1"] * (1 + U) + U * ref["dep"])
            wd = abs(g_scale * 2.0 / np.float64(ref["N1"]) / far)
            out["d_depth"] = np.where(s1, wd * (a * (1 + gamma(4)) + gamma(4) * r) + TINY, 0.0)
    return out


MASKED_ORDERS = ("kernel", "channels_reversed", "depth_sub_first", "w_fp32")


def masked32(rgb, tgt, depth, prior, mask, far=FAR, coef=COEF, counts=None, g_scale=1.0, order="kernel"):
    """The same in numpy float32 (sums of the fp32 terms in float64, as the kernel's), in the kernel's order of operations or one of
    three others a correct kernel might have chosen: e summed from the last channel, r = (depth - prior) / far, and the seed as
    (x - y) * w with w = 2 / (3 N) formed in fp32.  The derived bounds must admit all of them."""
    B = rgb.shape[0]
    m = np.ones(B, F) if mask is None else mask
    s1, s0 = m == 1, m == 0
    d = rgb - tgt
    sq = d * d
    e = (sq[:, 2] + sq[:, 1]) + sq[:, 0] if order == "channels_reversed" else (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    N1, N0 = (np.float64(counts[0]), np.float64(counts[1])) if counts is not None else (np.float64(s1.sum()), np.float64(s0.sum()))
    g, c, fa = F(g_scale), F(coef), F(far)
    with np.errstate(all="ignore"):
        if order == "w_fp32":
            w3 = lambda N: F(2) / (F(3) * F(N))  # noqa: E731
            wN = lambda N: F(2) / F(N)  # noqa: E731
        else:
            w3 = lambda N: F(2.0 / (3.0 * N))  # noqa: E731
            wN = lambda N: F(2.0 / N)  # noqa: E731
        img = F(f64(e)[s1].sum() / (3.0 * N1))
        if N0 > 0:
            img = img + c * F(f64(e)[s0].sum() / (3.0 * N0))
        w = np.where(s1, g * w3(N1), np.where(s0, g * c * w3(N0) if N0 > 0 else F(0), F(0))).astype(F)
        out = dict(img=float(img), d_rgb=d * w[:, None], dep=0.0, d_depth=None)
        if depth is not None:
            r = (depth - prior) / fa if order == "depth_sub_first" else depth / fa - prior / fa
            out["dep"] = float(F(f64(r * r)[s1].sum() / N1))
            out["d_depth"] = np.where(s1, (g * wN(N1) / fa) * r, F(0)).astype(F)
    return out


# ================================================================================================ MSE
MSE_MUTANTS = ("drop_last", "dup_16384", "drop_chunk")


def mse_inputs(n, seed=0):
    """x, y [n] float32: residuals N(0, 0.1), the spike elements (spike_rows) at +-1.0."""
    rs = np.random.RandomState(8000 + 17 * seed + n % 9973)
    y = rs.uniform(size=n)
    res = rs.normal(0, 0.1, size=n)
    rows = spike_rows(n)
    res[rows] = np.where(np.arange(len(rows)) % 2 == 0, 1.0, -1.0)
    return (y + res).astype(F), y.astype(F)


def mse64(x, y, mutant=None):
    """img2mse (H:9): (mean((x - y)^2), the seed 2 (x - y) / n)."""
    d = f64(x).reshape(-1) - f64(y).reshape(-1)
    n = d.size
    cnt = np.ones(n)
    if mutant == "drop_last":
        cnt[n - 1] = 0
    elif mutant == "dup_16384":
        cnt[16384] = 2
    elif mutant == "drop_chunk":
        cnt[16384:32768] = 0
    return float((cnt * d * d).sum() / n), 2.0 * d / n * (cnt > 0)


def mse_bounds(x, y):
    """value: d = fl(x - y) [1], fl(d d) [3], the cast of the fp64 mean [4 u], relative (non-negative terms).
    seed: w = fl(2 / n) [1], d [1], the product [1]: 3 u relative per element."""
    v, s = mse64(x, y)
    return gamma(4) * v, gamma(3) * np.abs(s) + TINY


MSE_ORDERS = ("kernel", "sub_reversed", "w_fp32")


def mse32(x, y, order="kernel"):
    x, y = x.reshape(-1), y.reshape(-1)
    n = x.size
    d = y - x if order == "sub_reversed" else x - y
    w = F(2) / F(n) if order == "w_fp32" else F(2.0 / n)
    seed = -(d * w) if order == "sub_reversed" else w * d
    return float(F(f64(d * d).sum() / n)), seed


# ================================================================================================ soft-Lp and softmask
SOFT_SIZES = (1, 2, 1023, 1024, 1025, 5000)
SOFT_COEFS = (0.5, 1.0, 2.0)
SOFT_TEMPS = (f32(0.05), f32(0.3), 5.0)


def soft_inputs(n, seed=0):
    """x, y [n] float32 with residuals in [-1, 1] and a block of EXACT zeros (a tenth of the elements from n // 3 on; none at n < 10)."""
    rs = np.random.RandomState(9000 + 19 * seed + n)
    y = rs.uniform(size=n).astype(F)
    x = (y + rs.uniform(-1, 1, size=n)).astype(F)
    lo = n // 3
    x[lo:lo + n // 10] = y[lo:lo + n // 10]
    return x, y


def softlp64(x, y, coef):
    """V:58: L = sum(w d^2) / sum(w), w = |d|^coef + 1, the sum of weights detached -> (L, dL/dx = d (coef |d|^coef + 2 w) / sum(w))."""
    d = f64(x) - f64(y)
    p = np.abs(d) ** coef
    w = p + 1
    Dn = w.sum()
    return float((w * d * d).sum() / Dn), d * (coef * p + 2 * w) / Dn


SOFTMASK_MUTANTS = ("den_not_detached", "no_L2")


def softmask64(x, y, t, mutant=None):
    """V:50 / V:55: L = N / Dn, N = sum(w d^2), Dn = sum(w), w = exp(d^2 / t); Dn detached in d, not in t
    -> (L, dL/dx = w (2 d + 2 d^3 / t) / Dn, dL/dt = -(sum(w d^4) / Dn - L^2) / t^2)."""
    d = f64(x) - f64(y)
    with np.errstate(all="ignore"):
        w = np.exp(d * d / t)
        Dn, N, s4 = w.sum(), (w * d * d).sum(), (w * d ** 4).sum()
        L = N / Dn
        seed = w * (2 * d + 2 * d ** 3 / t) / Dn
        if mutant == "den_not_detached":
            seed = seed - L * (w * 2 * d / t) / Dn
        dt = -(s4 / Dn - (0.0 if mutant == "no_L2" else L * L)) / (t * t)
    return float(L), seed, float(dt)


def softlp_aten(x, y, coef, dtype):
    """The literal line (oracle.mse_soft_lp) under autograd on the CPU.  At an exact-zero residual with coef < 1 autograd forms
    inf * 0 = NaN where the limit (and the kernel) is 0: callers leave those elements out of the yardstick."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
    L = O.mse_soft_lp(xt, torch.from_numpy(np.ascontiguousarray(y)).to(dtype), coef)
    L.backward()
    return float(L.detach()), xt.grad.numpy().astype(np.float64)


def softmask_aten(x, y, t, dtype):
    """V:50, literally, under autograd on the CPU -> (L, dL/dx, dL/dt)."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(dtype)
    tt = torch.tensor([t], dtype=dtype, requires_grad=True)
    L = torch.sum((torch.exp((xt - yt) ** 2 / tt)) * (xt - yt) ** 2) / torch.sum(torch.exp((xt - yt).detach() ** 2 / tt))
    L.backward()
    return float(L.detach()), xt.grad.numpy().astype(np.float64), float(tt.grad)


def softlp_floor(x, y, coef):
    """What 4 A is added to (A = 0 at n = 1): first-order rounding of the kernel's own lines, HIP's documented 1 ulp (= 2 u) for powf.
    p = powf(|d|, coef): d is off by u, which the power multiplies by coef, + 2 u [coef + 2]; w = fl(p + 1) [coef + 3, p <= w];
    fl(w fl(d d)) [coef + 3 + 3 + 1].  Numerator and denominator are sums of positive terms with those relative errors, the quotient
    adds them, the cast one more: (2 coef + 11) u on L.  Seed d (coef p + 2 (p + 1)) inv: coef p [coef + 3], 2 (p + 1) [coef + 3],
    their sum [coef + 4], times d [coef + 6], inv = fl(1 / Dn) [coef + 3 + 1], the product [1]: (2 coef + 11) u of each element
    -> (floor of |dL| relative to |L|, floor of the seed relative to max|seed|)."""
    k = gamma(2 * coef + 11)
    return k, k


def softmask_floor(x, y, t):
    """The same for w = expf(z), z = fl(fl(d d) / t): z is off by 4 u z, which exp turns into a relative 4 u z of w, + 2 u for expf's
    1 ulp: rel(w_i) = (4 z_i + 2) u.  Terms: w d^2 [4 z + 6], w d^4 [4 z + 10], each weighted by its size in its sum:
      rN = sum((4 z + 6) w d^2) / N u, rD = sum((4 z + 2) w) / Dn u, r4 = sum((4 z + 10) w d^4) / s4 u
    L: rN + rD + u.  dL/dt = -(s4 / Dn - L^2) / t^2 in fp64 from those sums: (s4 / Dn (r4 + rD) + 2 L^2 (rN + rD)) / t^2 + u |dL/dt|.
    Seed w (2 d + 2 d^3 / t) inv: d^3 [5], / t [6], the sum of two terms of one sign [7], times w [4 z + 10], inv [rD + u], the
    product [1]: (4 z_i + 12) u + rD of element i
    -> (floor of |dL| relative to |L|, floor of the seed relative to max|seed|, floor of |d dL/dt|, absolute)."""
    L, seed, dt = softmask64(x, y, t)
    d = f64(x) - f64(y)
    z = d * d / t
    w = np.exp(z)
    Dn, N, s4 = w.sum(), (w * d * d).sum(), (w * d ** 4).sum()
    rN = ((4 * z + 6) * w * d * d).sum() / N * U if N > 0 else 0.0
    rD = ((4 * z + 2) * w).sum() / Dn * U
    r4 = ((4 * z + 10) * w * d ** 4).sum() / s4 * U if s4 > 0 else 0.0
    fl_L = rN + rD + U
    gmax = np.abs(seed).max()
    fl_seed = float((np.abs(seed) * ((4 * z + 12) * U + rD)).max() / gmax) if gmax > 0 else 0.0
    fl_dt = (s4 / Dn * (r4 + rD) + 2 * L * L * (rN + rD)) / (t * t) + U * abs(dt)
    return fl_L, fl_seed, fl_dt


# ================================================================================================ patch term
PATCH_SIZES = ((1, 1), (1, 2), (1, 37), (3, 64), (4, 65), (4, 256), (8, 100), (16, 256), (16, 1000))
PATCH_FAMILIES = ("mild", "invalid", "quantised", "special")
PATCH_FLOOR = gamma(16)     # gtn [3 roundings], prq / r [3], alpha [1], e [2], the fp64 mean's cast [1], / P / 2 [1]; the gradient's
#                             weight w [2], ebar - e [1], gi [1], / r [1]: 16 u of |L|, and of max|g| per patch, added to 4 A


def patch_inputs(P, n, family, seed=0):
    """depth, mono [P n] float32.  mild: depth in [1.2, 6], mono in [0.05, 1].  invalid: a fifth of the priors invalid (0, negative or
    NaN) and a twentieth of the depths non-positive.  quantised: depths on a 0.25 grid, priors on a 0.125 grid (ties at both min and
    max).  special: mild, but patch 1 has no valid prior and patch 2 one depth for all its rays (each is minimum AND maximum)."""
    rs = np.random.RandomState(9500 + 23 * seed + 1000 * P + n + 7 * PATCH_FAMILIES.index(family))
    depth = rs.uniform(NEAR, FAR, size=(P, n))
    mono = rs.uniform(0.05, 1.0, size=(P, n))
    if family == "invalid":
        bad = rs.uniform(size=(P, n))
        mono[bad < 0.2] = 0.0
        mono[bad < 0.13] = -0.5
        mono[bad < 0.06] = np.nan
        dbad = rs.uniform(size=(P, n))
        depth[dbad < 0.05] = 0.0
        depth[dbad < 0.025] = -1.0
    elif family == "quantised":
        depth = np.round(depth * 4) / 4
        mono = np.maximum(np.round(mono * 8) / 8, 0.125)
    elif family == "special":
        if P > 1:
            mono[1] = -np.abs(mono[1])
        if P > 2:
            depth[2] = 2.5
    return depth.reshape(-1).astype(F), mono.reshape(-1).astype(F)


def patch_lines(depth, mono, P, n, dtype):
    """oracle.patch_depth_loss under autograd on the CPU -> (loss, d loss / d depth [P n])."""
    d = torch.from_numpy(np.ascontiguousarray(depth)).to(dtype).requires_grad_(True)
    L = O.patch_depth_loss(d, torch.from_numpy(np.ascontiguousarray(mono)).to(dtype), patch_num=P, n=n)
    L.backward()
    return float(L.detach()), d.grad.numpy().astype(np.float64)


# ================================================================================================ Adam
ADAM_SMALL = (1, 255, 256, 257)
ADAM_SWEEP = 4096 * 256                        # elements one sweep of the grid covers
ADAM_LARGE = (ADAM_SWEEP - 1, ADAM_SWEEP, ADAM_SWEEP + 1, 2 * ADAM_SWEEP + 77)
ADAM_PARAMS = ((0.0, 1.0), (0.1, 1.0), (0.0, 0.125), (0.05, 3.0), (0.1, 0.125))      # (clip, grad_scale)
ADAM_STEPS = (1, 2, 7, 1000, 200000)
ADAM_MUTANTS = ("bc2_unrooted", "eps_in_root", "clip_before_scale", "beta2_float")


def adam_lr(step):
    return O.lr_at(5e-4, step, 250)


def adam_scalars32(step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """(1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2), eps) as cnerf_adam_step rounds them: computed in double, then cast."""
    bc1, bc2 = 1.0 - math.pow(b1, step), 1.0 - math.pow(b2, step)
    return F(1.0 - b1), F(b2), F(1.0 - b2), F(lr / bc1), F(math.sqrt(bc2)), F(eps)


def clamp_keep_nan(g, clip):
    """torch.clamp(g, -clip, clip): NaN stays NaN, +-inf clip."""
    c = g.dtype.type(clip)
    return np.where(g < -c, -c, np.where(g > c, c, g))


def adam32(p, g, m, v, step, lr, clip=0.0, gscale=1.0):
    """adam_k in numpy float32, one correctly rounded IEEE operation per kernel operation, in its order -> (p, m, v)."""
    w1, beta2, w2, step_size, bc2_sqrt, eps = adam_scalars32(step, lr)
    with np.errstate(all="ignore"):
        gi = g * F(gscale)
        if clip > 0:
            gi = clamp_keep_nan(gi, F(clip))
        mi = m + w1 * (gi - m)
        vi = v * beta2 + w2 * (gi * gi)
        denom = np.sqrt(vi) / bc2_sqrt + eps
        pn = p - step_size * (mi / denom)
    assert pn.dtype == mi.dtype == vi.dtype == np.float32
    return pn, mi, vi


def adam64(p, g, m, v, step, lr, clip=0.0, gscale=1.0, b1=0.9, b2=0.999, eps=1e-8, mutant=None):
    """torch.optim.Adam's step after grad * grad_scale and clip_grad_value_, in float64 with the exact (double) scalars
    -> (p, m, v), (bound_p, bound_m, bound_v): the largest distance of adam_k's fp32 results from them, PER ELEMENT.

    With g~ = clamp(g s), E_g = u |g s| (the clamp is 1-Lipschitz; 0 where both sides clamp), D = g~ - m:
      m' = fl(m + fl(w1^ fl(g^ - m))):  E_m = w1 (E_g + 3 u |D|) + u |m'|            (the difference, w1's own rounding, the product; the sum)
      v' = fl(fl(v b2^) + fl(w2^ fl(g^ g^))):  E_v = 2 u v b2 + w2 (2 |g~| E_g + E_g^2 + 3 u g~^2) + u v'
      sqrt: |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), + u sqrt(v');  / fl(sqrt(bc2)): 2 u;  + fl(eps): u eps;  the sum: u denom
      q = m' / denom:  E_q = E_m / (denom - E_den) + |m'| E_den / (denom (denom - E_den)) + u |q|
      p' = fl(p - fl(step^ q)):  E_p = step (E_q + 2 u |q|) + u |p'|
    Every result that may fall under 2^-126 adds TINY; (1 + 16 u) over all for the second-order terms.  A near-cancelling m' or p'
    is covered by its own bound: no floor relative to the tensor.  mutant: one of ADAM_MUTANTS."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    bc1, bc2 = 1.0 - math.pow(b1, step), 1.0 - math.pow(b2, step)
    w1, w2 = 1.0 - b1, 1.0 - (float(F(b2)) if mutant == "beta2_float" else b2)
    cl = (lambda a: clamp_keep_nan(a, clip)) if clip > 0 else (lambda a: a)
    with np.errstate(all="ignore"):
        gs = g * gscale
        gc = cl(g) * gscale if mutant == "clip_before_scale" else cl(gs)
        m2 = m + w1 * (gc - m)
        v2 = v * b2 + w2 * gc * gc
        root = bc2 if mutant == "bc2_unrooted" else math.sqrt(bc2)
        den = np.sqrt(v2 + eps) / root if mutant == "eps_in_root" else np.sqrt(v2) / root + eps
        q = m2 / den
        step_size = lr / bc1
        p2 = p - step_size * q
        # bounds
        Eg = U * (np.minimum(np.abs(gs), clip * (1 + 2 * U)) if clip > 0 else np.abs(gs)) + TINY
        Em = w1 * (Eg + 3 * U * np.abs(gc - m)) + U * np.abs(m2) + 2 * TINY
        Ev = 2 * U * v * b2 + w2 * (2 * np.abs(gc) * Eg + Eg * Eg + 3 * U * gc * gc) + U * v2 + 3 * TINY
        sv = np.sqrt(v2)
        Es = np.minimum(np.where(sv > 0, Ev / np.where(sv > 0, sv, 1.0), np.inf), np.sqrt(Ev)) + U * sv
        Eden = (Es + 2 * U * sv) / math.sqrt(bc2) + TINY + U * eps + U * den
        lo = den - Eden
        Eq = Em / lo + np.abs(m2) * Eden / (den * lo) + U * np.abs(q) + TINY
        Ep = step_size * (Eq + 2 * U * np.abs(q)) + TINY + U * np.abs(p2)
    k = 1 + 16 * U
    return (p2, m2, v2), (Ep * k, Em * k, Ev * k)


_ADAM_BASE = {}


def _adam_base():
    """p, three warm-up gradients and the step's gradient at the largest size, drawn once; smaller cases take slices."""
    if not _ADAM_BASE:
        n = max(ADAM_LARGE)
        rs = np.random.RandomState(4242)
        p = rs.standard_normal(n).astype(F)
        m, v = np.zeros(n, F), np.zeros(n, F)
        for s in (1, 2, 3):                                   # the warm state: three earlier steps of the fp32 restatement
            p, m, v = adam32(p, (rs.standard_normal(n) * 0.05).astype(F), m, v, s, 5e-4)
        _ADAM_BASE.update(p=p, m=m, v=v, g=(rs.standard_normal(n) * 0.2).astype(F))
    return _ADAM_BASE


def adam_inputs(n, clip, gscale):
    """p, g, m, v [n] float32: a warm state (three earlier steps), gradients N(0, 0.2) / grad_scale (they straddle the clip), and
    from element 0 on — and again at the end of the buffer where it is long enough — the special elements:
      4 with g = 0 on m = v = 0 (denom = eps); 4 fresh ones (m = v = 0, g ordinary); |g s| = 1e-30 ... 1e+18, 25 of alternating sign
      (g g underflows to 0, to subnormals, and is ordinary); 3e19 and -1e25 (g g overflows); +-clip exactly; +-inf; NaN warm and fresh."""
    b = _adam_base()
    p, m, v = b["p"][:n].copy(), b["m"][:n].copy(), b["v"][:n].copy()
    g = (b["g"][:n] / F(gscale)).astype(F)
    mags = 10.0 ** np.linspace(-30, 18, 25) * np.where(np.arange(25) % 2 == 0, 1, -1)
    spec = [(0.0, True)] * 4 + [(0.3, True), (-0.02, True), (1e-5, True), (-4.0, True)] + [(x, False) for x in mags]
    spec += [(3e19, False), (-1e25, False), (np.inf, False), (-np.inf, False), (np.nan, False), (np.nan, True)]
    if clip > 0:
        spec += [(clip, False), (-clip, False), (clip, True)]
    for base in ([0] if n < 2 * len(spec) else [0, n - len(spec)]):
        for k, (val, fresh) in enumerate(spec[:n]):
            with np.errstate(all="ignore"):
                g[base + k] = F(F(val) / F(gscale))
            if fresh:
                m[base + k] = v[base + k] = 0
    return p, g, m, v


def adam_cases():
    """(n, clip, grad_scale, step): every small size with every parameter pair and step would be 100 cases of a few hundred elements;
    the small sizes take all parameter pairs at rotating steps and all steps at rotating pairs, each large size one pair and step."""
    cases = []
    for i, n in enumerate(ADAM_SMALL):
        for j, (c, s) in enumerate(ADAM_PARAMS):
            cases.append((n, c, s, ADAM_STEPS[(i + j) % 5]))
        for j, st in enumerate(ADAM_STEPS):
            c, s = ADAM_PARAMS[(i + j + 2) % 5]
            if (n, c, s, st) not in cases:
                cases.append((n, c, s, st))
    for i, n in enumerate(ADAM_LARGE):
        c, s = ADAM_PARAMS[(i + 1) % 5]
        cases.append((n, c, s, ADAM_STEPS[(2 * i + 1) % 5]))
    return cases


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements where ref is finite (0 / 0 = 0: an exact 0 meets a bound of 0)."""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)
        r = np.where(d == 0, 0.0, d / bound)
    ok = np.isfinite(ref) & np.isfinite(bound)
    return float(np.max(np.where(ok, r, 0.0))) if r.size else 0.0


# ================================================================================================ the cases both test files run
MASKED_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 32768, 49153)
MASKED_CHUNK = 16384
MSE_SIZES = (1, 1023, 1025, 16384, 16385, 40000, 65536, 65537, 3 * 16384 + 1)


def masked_variants():
    """(depth term on, global counts, g_scale): the four combinations every size and mask runs."""
    return ((True, False, 1.0), (True, True, 0.125), (False, True, 1.0), (False, False, 0.125))


def masked_case(B, mask_kind, with_depth, with_counts, g_scale):
    """-> (kwargs of masked64 / masked_bounds / masked32)."""
    d = masked_inputs(B, mask_kind)
    return dict(rgb=d["rgb"], tgt=d["tgt"], depth=d["depth"] if with_depth else None, prior=d["prior"] if with_depth else None,
                mask=d["mask"], far=FAR, coef=COEF, counts=global_counts(d["mask"], B) if with_counts else None, g_scale=g_scale)


def masked_ratio(got, kw):
    """max over the four outputs of |got - masked64| / masked_bounds (got: a dict with masked64's keys)."""
    ref, bnd = masked64(**kw), masked_bounds(**kw)
    keys = ("img", "d_rgb") + (("dep", "d_depth") if kw["depth"] is not None else ())
    return max(ratio(got[k], ref[k], bnd[k]) for k in keys)


def soft_yardstick(kind, x, y, par):
    """-> (ref, A, bound): the float64 lines, the fp32 ATen lines' distance from them and 4 A + floor, per quantity: (L, seed [relative
    to max|seed|; the elements where ATen's own autograd is NaN left out of A], and for softmask dL/dt)."""
    if kind == "softlp":
        ref = softlp64(x, y, par)
        a32 = softlp_aten(x, y, par, torch.float32)
        floor = softlp_floor(x, y, par)
        floor = (floor[0] * abs(ref[0]), floor[1])
    else:
        ref = softmask64(x, y, par)
        a32 = softmask_aten(x, y, par, torch.float32)
        floor = softmask_floor(x, y, par)
        floor = (floor[0] * abs(ref[0]), floor[1], floor[2])
    gmax = float(np.abs(ref[1]).max())
    fin = np.isfinite(a32[1])
    A = [abs(a32[0] - ref[0]), float(np.abs(a32[1] - ref[1])[fin].max() / gmax) if (gmax > 0 and fin.any()) else 0.0]
    if kind == "softmask":
        A.append(abs(a32[2] - ref[2]))
    return ref, A, [4 * a + f for a, f in zip(A, floor)]


def mutant_ratios(large_adam=True):
    """Every mutant of the float64 statements on the GPU test's own inputs -> [(family, mutant, case, |mutant - reference| / bound)],
    the largest ratio over the case's quantities.  A bound that admitted one of them (ratio < 4) would be too loose to tell a wrong
    kernel from a right one."""
    rows = []
    for B in MASKED_SIZES:
        if B < 63:
            continue                                  # one ray: dropping it leaves 0 / 0
        for wd, wc, gs in masked_variants():
            kw = masked_case(B, "mixed", wd, wc, gs)
            for mu in MASKED_MUTANTS:
                if mu in ("dup_16384", "drop_chunk") and B <= MASKED_CHUNK:
                    continue
                if (mu == "local_counts" and not wc) or (mu == "depth_seed_m0" and not wd):
                    continue
                rows.append(("masked", mu, f"B{B}-depth{int(wd)}-counts{int(wc)}-g{gs}", masked_ratio(masked64(mutant=mu, **kw), kw)))
    for n in MSE_SIZES:
        x, y = mse_inputs(n)
        (v, s), (bv, bs) = mse64(x, y), mse_bounds(x, y)
        for mu in MSE_MUTANTS:
            if n < 2 or (mu != "drop_last" and n <= MASKED_CHUNK):
                continue
            mv, ms = mse64(x, y, mu)
            rows.append(("mse", mu, f"n{n}", max(ratio(mv, v, bv), ratio(ms, s, bs))))
    for n in SOFT_SIZES:
        if n < 2:
            continue
        x, y = soft_inputs(n)
        for t in SOFT_TEMPS:
            ref, _A, bnd = soft_yardstick("softmask", x, y, t)
            gmax = np.abs(ref[1]).max()
            mu = softmask64(x, y, t, "den_not_detached")
            rows.append(("softmask", "den_not_detached", f"n{n}-t{t:.3g}", float(np.abs(mu[1] - ref[1]).max() / gmax / bnd[1])))
            mu = softmask64(x, y, t, "no_L2")
            rows.append(("softmask", "no_L2", f"n{n}-t{t:.3g}", abs(mu[2] - ref[2]) / bnd[2]))
    for n, clip, gs, step in adam_cases():
        if n < 255 or (n > 257 and (not large_adam or n != ADAM_LARGE[0])):
            continue
        p, g, m, v = adam_inputs(n, clip, gs)
        ref, bnd = adam64(p, g, m, v, step, adam_lr(step), clip, gs)
        for mu in ADAM_MUTANTS:
            if (mu == "bc2_unrooted" and step > 1000) or (mu == "clip_before_scale" and (clip == 0 or gs == 1.0)):
                continue                              # 1 - 0.999^200000 is 1.0 in double; clamp and scale commute without either
            got, _ = adam64(p, g, m, v, step, adam_lr(step), clip, gs, mutant=mu)
            rows.append(("adam", mu, f"n{n}-clip{clip}-gs{gs}-step{step}", max(ratio(a, b, c) for a, b, c in zip(got, ref, bnd))))
    return rows
