"""Float64 statements, derived bounds, input families, case lists and mutants for the SSIM / MS-SSIM envelope
(tests/test_gpu_ssim_envelope.py runs the kernels of csrc/ssim.hip against these; tests/test_ssim_env_cpu.py checks the statements, the
bounds and the mutants without a GPU).  numpy / torch on the CPU only; the product never imports it.

The truth.  tests/_ssim_ref.py in float64, filtered with the LIBRARY's window: cn_ssim_window builds its taps in fp32 (restated in
numpy float32 by taps32(): its running fp32 sum differs from ATen's vectorised sum, so these taps sit up to two ulps from
_ssim_ref.window(dtype=float32)), and the truth casts those taps up.  With float64 taps the two windows' difference (1e-8 of
f(XX)) would land in f(XX) - mu^2 on flat images and be charged to the kernel.  C1 and C2 are likewise the fp32 numbers the C entry
points receive, cast up.

Forward bound (per plane, on the means of S and of cs).  ssim_tile_k accumulates the five filtered sums in fp64, forms the
variances there and rounds mu_x, mu_y, s_xx, s_yy, s_xy to fp32 once each; cn_ssim_pixel_var then runs K_S fp32 operations.  To
first order per pixel

    u (|lx| |mu_x| + |ly| |mu_y| + |b| (|s_xx| + |s_yy|) + |c| |s_xy| + K_S |S|),     lx = cs 2 (mu_y - l mu_x) / B1

b = -S / B2 and c = 2 l / B2 are ssim.hpp's coefficients; lx is the FIRST term of ssim.hpp's a_x: the kernel rounds the means after
the variances are formed, so a mean's rounding reaches S through the luminance factor alone (the other two terms of a_x belong to
the f(x^2) parametrisation and are what |b| |s_xx| carries here).  cs does not depend on the means at fixed variances:
u (|cs / B2| (|s_xx| + |s_yy|) + |2 / B2| |s_xy| + K_CS |cs|).  The plane's bound is the mean of these + u |mean| (the last rounding).
An fp32 filter (cn_patch_ssim_wave; the ATen fp32 lines) is the same propagation with the filter's own roundings: `nf` roundings
per filtered sum make d mu <= nf u f(|X|), d f(XX) <= (nf + 1) u f(XX), and the fp32 subtraction f(XX) - mu^2 adds
2 |mu| d mu + u mu^2 + u |s_xx|.
    K_S  = 12: mx mx, my my, mx my (3), B1 (2 additions), B2 (2), 2 s_xy + C2 (1), its division (1), 2 mxy + C1 (1), its division (1),
               l cs (1); inputs >= 0, so no numerator cancels
    K_CS = 4:  B2 (2), 2 s_xy + C2 (1), the division (1)
    NF_PATCH = 22: cn_patch_ssim_wave's 11 taps, a product and an addition each when the compiler does not fuse them

Backward bound (elementwise).  A[i] = the backward's own sum with every term replaced by its absolute value:
    A = f^T|a_x| + 2 |X| f^T|b| + |Y| f^T|c|,  each coefficient map times |seed| / (Ho Wo),
|a_x| the sum of the absolute values of the three terms of ssim.hpp's a_x (of the one term of the cs form), and for MS-SSIM a
quarter of the next level's A pooled back, as the kernel adds the gradient.  The assertion is |g - g64| <= C_GRAD u A + FLOOR max|g64|
(per plane; the floor is for products that underflow).  C_GRAD = 4 x the largest |g32 - g64| / (u A) of the fp32 ATen autograd of
_ssim_ref over every case below, rounded up to a power of two, per section (REF_RATIO_MEASURED; tests/test_ssim_env_cpu.py
re-derives it); it is never measured on the kernel.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import _ssim_ref as R

U = 2.0 ** -24
FLOOR = 1e-12
K_S, K_CS, NF_PATCH = 12, 4, 22
FTH, FTW, BTH, BTW = 8, 64, 8, 32          # csrc/ssim.hip's forward output tile and backward input tile
# per section (its own cases): the largest |g32 - g64| / (u A) of the fp32 ATen autograd on the CPU, and C_GRAD = 4 x that rounded
# up to a power of two.  One figure for all three sections would be the MS-SSIM one (the fp32 lines lose most where the last level is
# a single window of a four times pooled image); each section is held to its own, smaller wherever the reference allows.
# (ATen's fp32 sums depend on the CPU: two machines gave 16.4 / 21.7, 296 / 235, 103.2 / 103.2; the larger is kept)
REF_RATIO_MEASURED = {"ssim": 21.7, "msssim": 296.0, "patch": 103.2}
C_GRAD = {"ssim": 128, "msssim": 2048, "patch": 512}
MS_WEIGHTS6 = R.MS_WEIGHTS + (0.1,)


def c_from(ratio):
    return 2 ** math.ceil(math.log2(4.0 * ratio))


def f32c(x):
    return float(np.float32(x))


def consts(data_range, K=(0.01, 0.03)):
    """(C1, C2) as the C entry points receive them: the doubles of pytorch-msssim rounded to fp32."""
    return f32c((K[0] * data_range) ** 2), f32c((K[1] * data_range) ** 2)


def taps32(win_size, win_sigma):
    """cn_ssim_window's fp32 sequence (expf correctly rounded, the sum running in fp32 in index order)."""
    sigma = np.float32(win_sigma)
    den = np.float32(2.0 * float(sigma) * float(sigma))
    g = np.empty(win_size, np.float32)
    s = np.float32(0)
    for t in range(win_size):
        c = np.float32(t - win_size // 2)
        g[t] = np.float32(math.exp(float(np.float32(-(c * c)) / den)))
        s = np.float32(s + g[t])
    return g / s


# ================================================================================================ inputs
FAMILIES = ("noise", "flat", "near", "masked", "same", "anti", "hdr")


def images(family, shape, seed, data_range=1.0):
    """(X, Y) float32 [N, C, H, W] on the CPU.  hdr: values up to data_range, some pixels above it."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(*shape, generator=g)
    n1, n2 = torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)
    if family == "noise":
        Y = (X + 0.15 * n1).clamp(0, 1)
    elif family == "flat":
        X, Y = 0.6 + 5e-4 * (2 * X - 1), 0.6 + 5e-4 * (2 * n2 - 1)
    elif family == "near":
        Y = (X + 1e-3 * n1).clamp(0, 1)
    elif family == "masked":
        m = (n2 < 0.5).float()
        X, Y = X * m, (X + 0.15 * n1).clamp(0, 1) * m
    elif family == "same":
        Y = X.clone()
    elif family == "anti":
        Y = 1 - X
    elif family == "hdr":
        X, Y = 1.1 * X, (1.1 * X + 0.15 * n1).clamp(0, 1.2)
    else:
        raise ValueError(family)
    return (X * data_range).float().contiguous(), (Y * data_range).float().contiguous()


PLANE_SEEDS = {1: (-1.3,), 6: (1.0, 0.0, -0.7, 1e3, 0.3, -2.5)}


def case(H, W, win=11, sigma=1.5, dr=1.0, fam="noise", planes=(1, 1)):
    dr = 255.0 if fam == "hdr" else dr
    name = f"{H}x{W}-w{win}-dr{dr:g}-{fam}-{planes[0]}x{planes[1]}"
    return SimpleNamespace(name=name, H=H, W=W, win=win, sigma=sigma, dr=dr, fam=fam, planes=planes)


def ssim_cases():
    out = []
    corners = {(1, 1), (8, 64), (9, 65)}
    for Ho in (1, 7, 8, 9, 17):                                          # forward tile edges, window 11
        for Wo in (1, 63, 64, 65, 129):
            out.append(case(Ho + 10, Wo + 10, planes=(2, 3) if (Ho, Wo) in corners else (1, 1)))
    for win in (3, 11):                                                  # backward tile edges (window 11: H unfiltered)
        for H in (8, 9):
            for W in (31, 32, 33):
                out.append(case(H, W, win=win))
    out += [case(5, 80), case(80, 5), case(10, 11), case(11, 10)]        # one side unfiltered
    out += [case(1, 1), case(8, 8), case(1, 40)]                         # neither side filtered
    out += [case(45, 100, win=1), case(45, 100, win=3, planes=(2, 3)), case(45, 100, win=7), case(45, 100, win=31, sigma=5.0)]
    out += [case(64, 80, dr=255.0), case(19, 75, dr=255.0, planes=(2, 3))]
    for fam in FAMILIES:
        out += [case(11, 11, fam=fam), case(19, 75, fam=fam, planes=(2, 3)), case(64, 80, fam=fam)]
    seen, uniq = set(), []
    for c in out:
        if c.name not in seen:
            seen.add(c.name)
            uniq.append(c)
    return uniq


def ms_case(H, W, win=3, levels=5, fam="noise", planes=(1, 1)):
    name = f"{H}x{W}-w{win}-L{levels}-{fam}-{planes[0]}x{planes[1]}"
    return SimpleNamespace(name=name, H=H, W=W, win=win, sigma=1.5, dr=1.0, fam=fam, planes=planes, levels=levels)


def ms_cases():
    out = [ms_case(33, 33), ms_case(48, 48), ms_case(40, 40), ms_case(33, 34), ms_case(34, 33), ms_case(33, 97), ms_case(35, 131)]
    out += [ms_case(33, 50, levels=L) for L in (1, 2, 3, 6)]
    out += [ms_case(161, 161, win=11), ms_case(162, 175, win=11), ms_case(175, 161, win=11)]
    for fam in ("noise", "flat", "masked", "anti"):
        out.append(ms_case(33, 50, fam=fam, planes=(2, 3) if fam == "noise" else (1, 1)))
        if fam != "noise":
            out.append(ms_case(161, 161, win=11, fam=fam))
    return out


PATCH_FAMILIES = ("noise", "near", "same")


def patch_inputs(P, fam):
    """(rgb, target) float32 [P * 256, 3]."""
    X, Y = images(fam, (P * 256, 3), 600 + P)
    return X, Y


def case_inputs(c):
    """-> X, Y float32 [N, C, H, W], seed float32 [N, C] (or g_v [levels, N, C] of mixed sign for an MS-SSIM case)."""
    N, C = c.planes
    sd = sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 100000
    X, Y = images(c.fam, (N, C, c.H, c.W), sd, c.dr)
    if hasattr(c, "levels"):
        g = torch.randn(c.levels, N, C, generator=torch.Generator().manual_seed(sd + 1))
        g = torch.where(g.abs() < 0.1, torch.full_like(g, 0.5), g)
        return X, Y, g.float()
    return X, Y, torch.tensor(PLANE_SEEDS[N * C], dtype=torch.float32).view(N, C)


# ================================================================================================ the explicit float64 statement
def _rep(g, C, dim):
    k = g.numel()
    return (g.view(1, 1, k, 1) if dim == 2 else g.view(1, 1, 1, k)).repeat(C, 1, 1, 1)


def _conv(x, g, dim):
    return F.conv2d(x, _rep(g, x.shape[1], dim), groups=x.shape[1])


def _convT(x, g, dim):
    return F.conv_transpose2d(x, _rep(g, x.shape[1], dim), groups=x.shape[1])


def pixel(X, Y, taps, C1, C2, mutant=None):
    """The five filtered quantities and S, cs per output pixel (ssim.hpp's statement)."""
    g = torch.as_tensor(taps).to(X.dtype)
    k = g.numel()
    fh, fw = X.shape[2] >= k, X.shape[3] >= k
    q = []
    for t in (X, Y, X * X, Y * Y, X * Y, X.abs(), Y.abs(), (X * Y).abs()):
        v = _conv(t, g, 2) if fh else t
        o = _conv(v, g, 3) if fw else v
        if mutant == "fwd_halo_col" and fw and k > 1 and o.shape[3] >= FTW:       # tile 0's halo lacks its last column
            o = o.clone()
            o[..., FTW - 1] -= g[k - 1] * v[..., FTW - 1 + k - 1]
        q.append(o)
    p = SimpleNamespace(mx=q[0], my=q[1], exx=q[2], eyy=q[3], exy=q[4], fax=q[5], fay=q[6], faxy=q[7], g=g)
    p.sxx, p.syy, p.sxy = p.exx - p.mx * p.mx, p.eyy - p.my * p.my, p.exy - p.mx * p.my
    p.B1, p.B2 = p.mx * p.mx + p.my * p.my + C1, p.sxx + p.syy + C2
    p.cs = (2 * p.sxy + C2) / p.B2
    p.l = (2 * p.mx * p.my + C1) / p.B1
    p.S = p.l * p.cs
    return p


def plane_means(p):
    return p.S.flatten(2).mean(-1), p.cs.flatten(2).mean(-1)


def coefs(p, on_cs):
    """(terms of a_x, terms of a_y, b, c) as ssim.hpp writes them."""
    if on_cs:
        return [2 * (p.mx * p.cs - p.my) / p.B2], [2 * (p.my * p.cs - p.mx) / p.B2], -p.cs / p.B2, 2 / p.B2
    ax = [p.cs * 2 * (p.my - p.l * p.mx) / p.B1, 2 * p.mx * p.S / p.B2, -2 * p.l * p.my / p.B2]
    ay = [p.cs * 2 * (p.mx - p.l * p.my) / p.B1, 2 * p.my * p.S / p.B2, -2 * p.l * p.mx / p.B2]
    return ax, ay, -p.S / p.B2, 2 * p.l / p.B2


def fT(m, g, H, W, mutant=None):
    """The zero-padded full correlation back to [H, W]; a side the forward left unfiltered is left alone."""
    k = g.numel()
    gg = g
    if mutant == "tap" and k > 1:
        gg = g.clone()
        gg[k - 1] = 0
    for dim, side in ((2, H), (3, W)):
        if m.shape[dim] != side:
            v = _convT(m, gg, dim)
            if mutant == "bwd_halo_row" and dim == 2 and H > BTH and BTH - (k - 1) >= 0:   # the tile at row 8 lacks its first halo row
                v = v.clone()
                v[:, :, BTH, :] -= gg[k - 1] * m[:, :, BTH - (k - 1), :]
            m = v
        elif mutant == "unfiltered_filtered" and k > 1 and side < k:
            pad = (k // 2, 0) if dim == 2 else (0, k // 2)
            m = F.conv2d(m, _rep(g, m.shape[1], dim), padding=pad, groups=m.shape[1])
    if mutant == "corner" and k > 1 and m.shape[2] > 1 and m.shape[3] > 1:      # the outermost tap dropped at the first pixel alone
        m = m.clone()
        m[:, :, 0, 0] = 0
    return m


def level_grad(p, X, Y, seed, on_cs, mutant=None, absolute=False):
    """dX, dY of sum_planes seed * mean(S or cs) by ssim.hpp's formula; absolute=True gives A (every term by its absolute value)."""
    N, C, H, W = X.shape
    Ho, Wo = p.S.shape[2:]
    cnt = H * W if mutant == "inv_cnt" else Ho * Wo
    sc = (seed.abs() if absolute else seed).to(X.dtype).view(N, C, 1, 1) / cnt
    axt, ayt, b, c = coefs(p, on_cs)
    if absolute:
        ax, ay, b, c, X, Y = sum(t.abs() for t in axt), sum(t.abs() for t in ayt), b.abs(), c.abs(), X.abs(), Y.abs()
    else:
        ax, ay = sum(axt), sum(ayt)
    if mutant == "dy_from_ax":
        ay = ax
    fa, fy, fb, fc = (fT(t * sc, p.g, H, W, mutant) for t in (ax, ay, b, c))
    return fa + 2 * X * fb + Y * fc, fy + 2 * Y * fb + X * fc


def unpool(n, H, W, mutant=None):
    """avg_pool2d(2, padding (H % 2, W % 2))'s backward without the quarter: input pixel (i, j) <- n[(i + H % 2) >> 1, (j + W % 2) >> 1]."""
    sh, sw = (0, 0) if mutant == "pool_parity" else (H % 2, W % 2)
    r = (torch.arange(H) + sh) >> 1
    c = (torch.arange(W) + sw) >> 1
    return n[:, :, r][:, :, :, c]


def pyramid(X, Y, levels):
    out = [(X, Y)]
    for _ in range(levels - 1):
        X, Y = R.pool(X), R.pool(Y)
        out.append((X, Y))
    return out


def ms_explicit(X, Y, taps, C1, C2, g_v, mutant=None, absolute=False):
    """dX, dY of sum(g_v * v) level by level as cnerf_msssim_bwd walks them."""
    levels = g_v.shape[0]
    pyr = pyramid(X, Y, levels)
    nX = nY = None
    for l in range(levels - 1, -1, -1):
        x, y = pyr[l]
        on_cs = l < levels - 1
        if (mutant == "seed_S_for_cs" and l < levels - 1) or (mutant == "seed_cs_for_S" and l == levels - 1):
            on_cs = not on_cs
        dx, dy = level_grad(pixel(x, y, taps, C1, C2), x, y, g_v[l], on_cs, mutant, absolute)
        if nX is not None:
            dx = dx + 0.25 * unpool(nX, x.shape[2], x.shape[3], mutant)
            dy = dy + 0.25 * unpool(nY, x.shape[2], x.shape[3], mutant)
        nX, nY = dx, dy
    return nX, nY


# ================================================================================================ truths by autograd (any dtype)
def ssim_lines(X, Y, taps, C1, C2, seed, dtype=torch.float64):
    """_ssim_ref.maps in `dtype` -> (S [N, C], cs [N, C], dX, dY of sum(seed * S)), all float64."""
    x, y = X.to(dtype).clone().requires_grad_(), Y.to(dtype).clone().requires_grad_()
    s, cs = R.maps(x, y, win_size=len(taps), taps=torch.as_tensor(taps), consts=(C1, C2))
    S, CS = s.flatten(2).mean(-1), cs.flatten(2).mean(-1)
    gx, gy = torch.autograd.grad((S * seed.to(dtype)).sum(), (x, y))
    return S.detach().double(), CS.detach().double(), gx.double(), gy.double()


def ms_lines(X, Y, taps, C1, C2, g_v, dtype=torch.float64):
    """-> (v [levels, N, C], dX, dY of sum(g_v * v), [pooled (X_l, Y_l)]) in `dtype`, returned as float64."""
    x, y = X.to(dtype).clone().requires_grad_(), Y.to(dtype).clone().requires_grad_()
    levels = g_v.shape[0]
    a, b, v, pyr = x, y, [], []
    for l in range(levels):
        pyr.append((a.detach().double(), b.detach().double()))
        s, cs = R.maps(a, b, win_size=len(taps), taps=torch.as_tensor(taps), consts=(C1, C2))
        v.append((s if l == levels - 1 else cs).flatten(2).mean(-1))
        if l < levels - 1:
            a, b = R.pool(a), R.pool(b)
    v = torch.stack(v)
    gx, gy = torch.autograd.grad((v * g_v.to(dtype)).sum(), (x, y))
    return v.detach().double(), gx.double(), gy.double(), pyr


def kernel_order_lines(X, Y, taps, C1, C2):
    """The forward in ssim_tile_k's order of operations, on ATen: the filtered sums and the variances in float64, rounded to fp32 once
    each, cn_ssim_pixel_var's operations in fp32, the mean in float64, rounded -> (S, cs) [N, C] as float64.  Honest arithmetic the
    forward bound has to admit, written without the kernel (tests/test_ssim_env_cpu.py)."""
    p = pixel(X.double(), Y.double(), taps, C1, C2)
    mx, my, sxx, syy, sxy = (t.float() for t in (p.mx, p.my, p.sxx, p.syy, p.sxy))
    c1, c2 = torch.tensor(C1, dtype=torch.float32), torch.tensor(C2, dtype=torch.float32)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    B2, B1 = sxx + syy + c2, mxx + myy + c1
    cs = (2 * sxy + c2) / B2
    S = (2 * mxy + c1) / B1 * cs
    return tuple(t.double().flatten(2).mean(-1).float().double() for t in (S, cs))


def kernel_order_ms_lines(X, Y, taps, C1, C2, levels):
    """v [levels, N, C] the same way, the levels pooled in fp32 as avg_pool2_k does."""
    v = []
    x, y = X.float(), Y.float()
    for l in range(levels):
        S, cs = kernel_order_lines(x, y, taps, C1, C2)
        v.append(S if l == levels - 1 else cs)
        x, y = R.pool(x), R.pool(y)
    return torch.stack(v)


def patch_lines(rgb, tgt, P, dtype=torch.float64):
    """_ssim_ref.patch_level (V's lines, the literal 4) with the library's taps -> (value, d value / d rgb [P * 256, 3])."""
    taps, (C1, C2) = torch.as_tensor(taps32(11, 1.5)), consts(1.0)
    r = rgb.to(dtype).clone().requires_grad_()
    t = tgt.to(dtype)
    tot = 0.0
    for p in range(P):
        a, b = r[p * 256:(p + 1) * 256].reshape(1, 16, 16, 3), t[p * 256:(p + 1) * 256].reshape(1, 16, 16, 3)
        s, _ = R.maps(a, b, win_size=11, taps=taps, consts=(C1, C2))
        tot = tot + s.flatten(2).mean(-1).mean(1)
    v = (tot / 4)[0]
    g, = torch.autograd.grad(v, (r,))
    return float(v.detach()), g.double()


# ================================================================================================ bounds
def fwd_bounds(p, nf=0):
    """(bound on the plane mean of S, of cs) [N, C]; nf = the fp32 roundings of one filtered sum (0: fp64 sums and variances)."""
    a = torch.abs
    if nf == 0:
        dmx, dmy, dsxx, dsyy, dsxy = U * a(p.mx), U * a(p.my), U * a(p.sxx), U * a(p.syy), U * a(p.sxy)
    else:
        dmx, dmy = nf * U * p.fax, nf * U * p.fay
        dsxx = (nf + 1) * U * p.exx + 2 * a(p.mx) * dmx + U * p.mx * p.mx + U * a(p.sxx)
        dsyy = (nf + 1) * U * p.eyy + 2 * a(p.my) * dmy + U * p.my * p.my + U * a(p.syy)
        dsxy = (nf + 1) * U * p.faxy + a(p.mx) * dmy + a(p.my) * dmx + U * a(p.mx * p.my) + U * a(p.sxy)
    lx, ly = a(p.cs * 2 * (p.my - p.l * p.mx) / p.B1), a(p.cs * 2 * (p.mx - p.l * p.my) / p.B1)
    bS = lx * dmx + ly * dmy + a(p.S / p.B2) * (dsxx + dsyy) + a(2 * p.l / p.B2) * dsxy + K_S * U * a(p.S)
    bC = a(p.cs / p.B2) * (dsxx + dsyy) + a(2 / p.B2) * dsxy + K_CS * U * a(p.cs)
    mS, mC = plane_means(p)
    return bS.flatten(2).mean(-1) + U * a(mS), bC.flatten(2).mean(-1) + U * a(mC)


def grad_bound(A, g64, c):
    """c u A + FLOOR max|g64| per plane (c = C_GRAD of the section)."""
    return c * U * A + FLOOR * g64.abs().flatten(2).max(-1).values[:, :, None, None]


def grad_ratio(g, g64, A):
    """max |g - g64| / (u A) over the elements above the floor (what C_GRAD is derived from)."""
    d = (g - g64).abs()
    live = d > FLOOR * g64.abs().flatten(2).max(-1).values[:, :, None, None]
    if not live.any():
        return 0.0
    return float((d[live] / (U * A[live])).max())


POOL_U = 3        # avg_pool2_k: three fp32 additions, the division by 4 exact


def ms_fwd_bounds(X64, Y64, taps, C1, C2, levels, nf=0):
    """[levels, N, C]: the level's forward bound on float64-pooled images + the pooling's roundings carried into the level (level l's
    images are POOL_U * l * u from the float64 pool elementwise; to first order that moves v_l by sum_i |dv_l / dx_i| |dx_i|)."""
    out = []
    one = torch.ones(X64.shape[:2], dtype=torch.float64)
    for l, (x, y) in enumerate(pyramid(X64, Y64, levels)):
        p = pixel(x, y, taps, C1, C2)
        last = l == levels - 1
        b = fwd_bounds(p, nf)[0 if last else 1]
        if l:
            gx, gy = level_grad(p, x, y, one, not last)
            b = b + POOL_U * l * U * ((gx * x).abs() + (gy * y).abs()).flatten(2).sum(-1)
        out.append(b)
    return torch.stack(out)


def pool64(X):
    """(avg_pool2d(2, padding (H % 2, W % 2), count_include_pad) in float64, the bound POOL_U u sum|taps| / 4)."""
    pad = [s % 2 for s in X.shape[2:]]
    Xd = X.double()
    return (F.avg_pool2d(Xd, 2, padding=pad, count_include_pad=True),
            POOL_U * U * F.avg_pool2d(Xd.abs(), 2, padding=pad, count_include_pad=True))


# ================================================================================================ per-case truths, shared and cached
_CACHE = {}


def truth(c):
    """Everything a test needs of one case, computed once: inputs, float64 lines, fp32 ATen lines, A, forward bounds."""
    if c.name in _CACHE:
        return _CACHE[c.name]
    X, Y, seed = case_inputs(c)
    taps, (C1, C2) = taps32(c.win, c.sigma), consts(c.dr)
    X64, Y64 = X.double(), Y.double()
    t = SimpleNamespace(X=X, Y=Y, seed=seed, taps=taps, C1=C1, C2=C2)
    if hasattr(c, "levels"):
        t.v, t.gx, t.gy, t.pyr = ms_lines(X, Y, taps, C1, C2, seed)
        t.v32, t.gx32, t.gy32, _ = ms_lines(X, Y, taps, C1, C2, seed, torch.float32)
        t.Ax, t.Ay = ms_explicit(X64, Y64, taps, C1, C2, seed.double(), absolute=True)
        t.bv = ms_fwd_bounds(X64, Y64, taps, C1, C2, c.levels)
        t.bv32 = ms_fwd_bounds(X64, Y64, taps, C1, C2, c.levels, nf=4 * c.win)
    else:
        t.S, t.cs, t.gx, t.gy = ssim_lines(X, Y, taps, C1, C2, seed)
        t.S32, t.cs32, t.gx32, t.gy32 = ssim_lines(X, Y, taps, C1, C2, seed, torch.float32)
        t.p = pixel(X64, Y64, taps, C1, C2)
        t.Ax, t.Ay = level_grad(t.p, X64, Y64, seed.double(), False, absolute=True)
        t.bS, t.bcs = fwd_bounds(t.p)
        t.bS32, t.bcs32 = fwd_bounds(t.p, nf=4 * c.win)          # the ATen fp32 lines: two passes of `win` products and additions
    _CACHE[c.name] = t
    return t


def patch_truth(P, fam):
    key = f"patch-{P}-{fam}"
    if key in _CACHE:
        return _CACHE[key]
    rgb, tgt = patch_inputs(P, fam)
    t = SimpleNamespace(rgb=rgb, tgt=tgt)
    t.v, t.g = patch_lines(rgb, tgt, P)
    t.v32, t.g32 = patch_lines(rgb, tgt, P, torch.float32)
    # the library reads a [1, 16, 16, 3] NHWC patch as NCHW: planes (1, 16), H = 16 (filtered), W = 3 (not); seed 1 / (4 * 16) per plane
    X = rgb.double().reshape(P, 16, 16, 3)
    Y = tgt.double().reshape(P, 16, 16, 3)
    taps, (C1, C2) = taps32(11, 1.5), consts(1.0)
    p = pixel(X, Y, taps, C1, C2)
    seed = torch.full((P, 16), 1.0 / 64, dtype=torch.float64)
    t.A = level_grad(p, X, Y, seed, False, absolute=True)[0].reshape(P * 256, 3)
    bS = fwd_bounds(p, NF_PATCH)[0]                                        # [P, 16]
    t.bv = float(bS.mean(1).sum() / 4 + (P + 2) * U * abs(t.v))             # + ssim_p's rounding, the P additions and the division
    t.bv32 = float(fwd_bounds(p, 2 * 11)[0].mean(1).sum() / 4 + (P + 18) * U * abs(t.v))
    _CACHE[key] = t
    return t


# ================================================================================================ mutants
MUTANTS = ("tap", "fwd_halo_col", "bwd_halo_row", "inv_cnt", "pool_parity", "seed_S_for_cs", "seed_cs_for_S", "dy_from_ax",
           "unfiltered_filtered", "corner")
MS_ONLY = ("pool_parity", "seed_S_for_cs", "seed_cs_for_S")


def _old_rule_grad(gm, g64, g32):
    """The rule of tests/test_gpu_ssim.py / test_gpu_msssim.py (relative to the tensor's largest element) -> the factor by which the
    mutant misses it (<= 1: it passes, the rule does not see it)."""
    scale = float(g64.abs().max())
    if scale == 0:
        return 0.0 if float((gm - g64).abs().max()) == 0 else float("inf")
    d, d32 = float((gm - g64).abs().max()) / scale, float((g32 - g64).abs().max()) / scale
    return d / min(2 * d32 + 1e-6, 1e-3)


def mutant_rows():
    """[(mutant, case, bound it is judged by, factor by which it misses that bound, factor by which it misses the old rule)] over
    every case it can show on."""
    rows = []
    for mu in MUTANTS:
        for c in (ms_cases() if mu in MS_ONLY else ssim_cases() + ms_cases()):
            t = truth(c)
            X64, Y64 = t.X.double(), t.Y.double()
            ms = hasattr(c, "levels")
            if mu == "fwd_halo_col":
                if ms:
                    continue
                mS, mC = plane_means(pixel(X64, Y64, t.taps, t.C1, t.C2, mu))
                r = max(float(((mS - t.S).abs() / t.bS).max()), float(((mC - t.cs).abs() / t.bcs).max()))
                d, d32 = float((mS - t.S).abs().max()), float((t.S32 - t.S).abs().max())
                rows.append((mu, c.name, "forward", r, d / min(1e-5, 2 * d32 + 1e-7)))
                continue
            if ms:
                gx, gy = ms_explicit(X64, Y64, t.taps, t.C1, t.C2, t.seed.double(), mu)
            else:
                gx, gy = level_grad(t.p, X64, Y64, t.seed.double(), False, mu)
            cg = C_GRAD["msssim" if ms else "ssim"]
            r = max(float(((gx - t.gx).abs() / grad_bound(t.Ax, t.gx, cg)).nan_to_num(0).max()),
                    float(((gy - t.gy).abs() / grad_bound(t.Ay, t.gy, cg)).nan_to_num(0).max()))
            rows.append((mu, c.name, "backward", r, max(_old_rule_grad(gx, t.gx, t.gx32), _old_rule_grad(gy, t.gy, t.gy32))))
    return rows


def mutant_summary(rows):
    """{mutant: worst factors under both rules, cases run / outside the bound, and of those how many the old rule passes or sees}"""
    out = {}
    for mu, _case, _kind, r, old in rows:
        o = out.setdefault(mu, {"worst factor": 0.0, "worst factor, old rule": 0.0, "cases outside": 0, "cases": 0,
                                "outside, passing the old rule": 0, "outside, seen by the old rule": 0})
        o["cases"] += 1
        o["worst factor"] = max(o["worst factor"], r)
        o["worst factor, old rule"] = max(o["worst factor, old rule"], old)
        if r > 1:
            o["cases outside"] += 1
            o["outside, passing the old rule" if old <= 1 else "outside, seen by the old rule"] += 1
    return out
