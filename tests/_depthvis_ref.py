"""The project's own numpy restatement of the depth visualiser (alky/vis_utils.py:59-150: lky_visualize_depth -> save_img_u8), the
statement csrc/depthvis.hip implements.  `dtype` switches the running sum of the weighted percentile: float32 reproduces the
reference (it sums the float32 weights as they are), float64 is what the kernel computes.  Ties in value are ordered by pixel index
(a stable sort), the order the kernel's (value, index) select realises.
"""
import numpy as np

EPS32 = np.finfo(np.float32).eps


def interp(t, xp, fp):
    """np.interp for one abscissa, written out: clamped at both ends; j = the LAST index with xp[j] <= t (so a run of equal running
    sums resolves to its end), the node itself where t hits it, else the segment through (xp[j], fp[j]) and (xp[j+1], fp[j+1])."""
    n = len(xp)
    if np.isnan(t):
        return t
    if t > xp[n - 1]:
        return fp[n - 1]
    if t < xp[0]:
        return fp[0]
    j = int(np.searchsorted(xp, t, side="right")) - 1
    if j == n - 1 or xp[j] == t:
        return fp[j]
    slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
    r = slope * (t - xp[j]) + fp[j]
    if np.isnan(r):
        r = slope * (t - xp[j + 1]) + fp[j + 1]
        if np.isnan(r) and fp[j] == fp[j + 1]:
            r = fp[j]
    return r


def weighted_bounds(x, w, dtype=np.float32, ps=(0.5, 99.5)):
    """(lo_auto, hi_auto) as float64: the weighted percentiles 0.5 / 99.5 of x [H, W] float32 under w [H, W] float32."""
    x, w = np.asarray(x, np.float32).reshape(-1), np.asarray(w, np.float32).reshape(-1)
    order = np.argsort(x, kind="stable")                       # ascending, NaN last
    xs, cum = x[order].astype(np.float64), np.cumsum(w[order].astype(dtype))
    total = cum[-1] / 100                                        # in `dtype`, as the reference's acc_w[-1] / 100
    cum = cum.astype(np.float64)
    with np.errstate(all="ignore"):
        return tuple(interp(np.float64(p) * np.float64(total), cum, xs) for p in ps)


def turbo_index(t):
    return np.minimum((t * 256).astype(np.int64), 255)


def visualize(x, acc, lut, lo=None, hi=None, dtype=np.float32, parts=False):
    """x = 1 / disp, acc [H, W] float32, lut [256, 3] float64 -> the float64 image [H, W, 3] (with parts: also the LUT index map and
    the two automatic bounds)."""
    x, acc = np.asarray(x, np.float32), np.asarray(acc, np.float32)
    with np.errstate(all="ignore"):
        lo_auto, hi_auto = weighted_bounds(x, acc, dtype)
        lo = lo or (lo_auto - EPS32)
        hi = hi or (hi_auto + EPS32)
        curve = lambda v: -np.log(v + EPS32)  # noqa: E731
        c, c_lo, c_hi = curve(x), curve(np.float64(lo)), curve(np.float64(hi))      # c stays float32, the bounds float64
        t = np.nan_to_num(np.clip((c - np.minimum(c_lo, c_hi)) / np.abs(c_hi - c_lo), 0, 1))
        idx = turbo_index(t)
        img = lut[idx] * acc[:, :, None] + (1 - acc)[:, :, None]
    return (img, idx, (lo_auto, hi_auto)) if parts else img


def to_u8(img):
    with np.errstate(all="ignore"):
        return (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)
