"""float64 restatement of the standard-normal stream of consistentnerf_amd/csrc/rng.hpp (CnRngDev::normal).  TEST HELPER ONLY.

Element (row0 + r, c) of the [*, cols] stream `offset` of `seed`: ONE Philox4x32-10 block on counter (e, offset) with e = (row0 + r) *
cols + c, key seed ^ "cnerf_rn" — exactly the block of oracle.philox.uniform — and Box-Muller on its words 0 and 1:
u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (x1 >> 8) * 2^-24 in [0, 1), n = sqrt(-2 ln u1) * cos(2 pi u2).  Here in float64;
the kernel evaluates the same formula with the fp32 OCML logf / sqrtf / cospif (a numpy fp32 evaluation deviates from this by 1.6e-6).
"""
import numpy as np

from oracle.philox import KEY_XOR, MASK, philox4x32_10

BOUND = float(np.sqrt(48.0 * np.log(2.0)))       # u1 >= 2^-24: |n| <= sqrt(48 ln 2) = 5.7681

# five standard errors at N = 2^20 (moments()): mean 5 / sqrt(N); variance 5 sqrt(2 / N); kurtosis 5 sqrt(24 / N);
# P(|x| < 1) 5 sqrt(p (1 - p) / N); a mean of products of independent unit-variance values, and a correlation: 5 / sqrt(N)
LIMITS = {"mean": 4.9e-3, "var": 6.9e-3, "kurtosis": 2.4e-2, "p_inside_1": 2.3e-3, "lag1_cols": 4.9e-3, "lag1_rows": 4.9e-3,
          "corr_uniform": 4.9e-3}


def words(seed, offset, rows, cols, row0=0):
    """(x0, x1) uint32 [rows, cols] of the elements' Philox blocks."""
    e = (np.uint64(row0) + np.arange(rows, dtype=np.uint64))[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]
    key = (int(seed) ^ KEY_XOR) & 0xFFFFFFFFFFFFFFFF
    off = int(offset) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10([e & MASK, e >> np.uint64(32), off & 0xFFFFFFFF, off >> 32], [key & 0xFFFFFFFF, key >> 32])
    return x[0], x[1]


def normal(seed, offset, rows, cols, row0=0, dtype=np.float64):
    """[rows, cols] of the normal stream, evaluated in `dtype` (float64: the reference; float32: what fp32 arithmetic costs)."""
    x0, x1 = words(seed, offset, rows, cols, row0)
    u1 = ((x0 >> np.uint32(8)).astype(np.int64) + 1).astype(dtype) * dtype(2.0 ** -24)
    u2 = (x1 >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
    return np.sqrt(dtype(-2.0) * np.log(u1)) * np.cos(dtype(2.0 * np.pi) * u2)


def moments(x, u):
    """The statistics the limits above bound, of a [rows, cols] draw `x` and a uniform draw `u` of the same shape."""
    x = np.asarray(x, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64) - 0.5
    m, v = x.mean(), x.var()
    return {"mean": m, "var": v - 1.0, "kurtosis": ((x - m) ** 4).mean() / v ** 2 - 3.0,
            "p_inside_1": (np.abs(x) < 1.0).mean() - 0.682689, "lag1_cols": (x[:, :-1] * x[:, 1:]).mean(),
            "lag1_rows": (x[:-1] * x[1:]).mean(), "corr_uniform": np.corrcoef(x.ravel(), u.ravel())[0, 1]}
