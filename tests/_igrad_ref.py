"""float64 numpy restatement of csrc/mlp_igrad.hip's arithmetic (cnerf_mlp_input_grad): the dZ blocks of the gradient workspace,
the three weight matrices and the stashed encodings in, d_pts and the per-point d_dirs out.

    d gamma(x) = dZ_0 . W_0 + dZ_{skip+1} . W_{skip+1}[:, :in_ch]          (the second term only with a skip layer)
    d gamma(d) = dZ_v . W_v[:, W:W + dir_ch]                               (view-direction networks)
    d_x[j]     = d gamma[j] + sum_k 2^k (cos_kj d gamma[3 + 6k + j] - sin_kj d gamma[3 + 6k + 3 + j])

with sin_kj / cos_kj READ from the stashed encoding (columns 3 + 6k + j / 3 + 6k + 3 + j, Embedder's order), as the kernel does:
no sin or cos is evaluated here.  n_freqs < 0 is the identity encoding (Jacobian I).  tests/test_igrad_ref_cpu.py checks this
against torch autograd of the oracle."""
import numpy as np


def enc_jacobian(d_gamma, gamma, n_freqs):
    """d_gamma, gamma [M, >= 3 (+ 6 n_freqs)] -> [M, 3]: the contraction of d loss / d gamma(v) with d gamma(v) / d v."""
    d_gamma, gamma = np.asarray(d_gamma, np.float64), np.asarray(gamma, np.float64)
    d = d_gamma[:, 0:3].copy()
    for k in range(max(n_freqs, 0)):
        s, c = 3 + 6 * k, 3 + 6 * k + 3
        d += 2.0 ** k * (gamma[:, c:c + 3] * d_gamma[:, s:s + 3] - gamma[:, s:s + 3] * d_gamma[:, c:c + 3])
    return d


def input_grads(dZ0, W0, enc, n_freqs, dZ_skip=None, W_skip_x=None, dZ_v=None, W_v_d=None, denc=None, n_freqs_views=None):
    """dZ0 [M, W] and W0 [W, in_ch] (layer 0), enc [M, >= in_ch] = the stashed gamma(x); with a skip layer dZ_skip [M, W] and
    W_skip_x [W, in_ch] = the gamma(x) columns of layer skip+1; with view directions dZ_v [M, W/2], W_v_d [W/2, dir_ch] = the
    gamma(d) columns of views_linears.0 and denc [M, >= dir_ch] = the stashed gamma(d).  -> (d_pts [M, 3], d_dirs_pt [M, 3] | None)."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    d_gx = f(dZ0) @ f(W0)
    if dZ_skip is not None:
        d_gx = d_gx + f(dZ_skip) @ f(W_skip_x)
    d_pts = enc_jacobian(d_gx, f(enc)[:, :d_gx.shape[1]], n_freqs)
    d_dirs = None
    if dZ_v is not None:
        d_gd = f(dZ_v) @ f(W_v_d)
        d_dirs = enc_jacobian(d_gd, f(denc)[:, :d_gd.shape[1]], n_freqs_views)
    return d_pts, d_dirs
