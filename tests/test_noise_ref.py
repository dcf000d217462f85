"""The float64 restatement of the normal stream (tests/_noise_ref.py) on its own, without a GPU: the statistical limits the GPU
test asserts on the kernel's stream hold for the restatement, so a failure there is the kernel's and not the formula's."""
import numpy as np

import _noise_ref as N
from oracle import philox as P


def test_restated_normal_stream_is_standard_normal():
    x = N.normal(1234, 6, 4096, 256)
    assert x.dtype == np.float64 and np.isfinite(x).all() and np.abs(x).max() <= N.BOUND
    got = N.moments(x, P.uniform(1234, 4, 4096, 256))
    print({k: f"{v:.2e}" for k, v in got.items()})
    for k, lim in N.LIMITS.items():
        assert abs(got[k]) <= lim, (k, got[k], lim)
    # what fp32 arithmetic costs on the same formula (the GPU test allows 1e-5 absolute)
    d = np.abs(N.normal(1234, 6, 4096, 256, dtype=np.float32).astype(np.float64) - x).max()
    print(f"fp32 evaluation vs float64: max|d| {d:.2e}")
    assert d <= 1e-5


def test_restated_normal_stream_shares_the_uniform_streams_block():
    """Word 0 of the element's block is the uniform stream's word; a shard's rows are the rows of the global stream; the bound is
    reached only at u1 = 2^-24."""
    x0, _ = N.words(99, 12, 33, 7, row0=5)
    assert np.array_equal((x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), P.uniform(99, 12, 33, 7, row0=5))
    assert np.array_equal(N.normal(99, 12, 40, 7)[5:38], N.normal(99, 12, 33, 7, row0=5))
    assert abs(np.sqrt(-2.0 * np.log(2.0 ** -24)) - N.BOUND) < 1e-12 and abs(N.BOUND - 5.7681) < 1e-4
