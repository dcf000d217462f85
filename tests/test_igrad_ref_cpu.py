"""tests/_igrad_ref.py (the float64 numpy restatement of cnerf_mlp_input_grad's arithmetic) against torch autograd of the oracle's
run_network (O.query) on the CPU, in float64.  The dZ blocks the kernel reads from the gradient workspace are taken from the same
autograd pass (the gradients of the oracle's pre-activations), the encodings it reads from the stash are the oracle's own.  No GPU."""
import numpy as np
import pytest
import torch

import _igrad_ref as R
import _inputs as I
from oracle import nerf_oracle as O

# (D, W, multires, multires_views, use_viewdirs, output_ch): with and without view directions, with (D > 5) and without a skip
# layer, the 10 / 4-frequency and the identity encodings
CASES = [(8, 64, 10, 4, True, 4), (4, 32, 10, 4, True, 4), (4, 32, 10, 4, False, 5), (6, 32, -1, -1, True, 4), (2, 32, 3, 1, True, 4)]


def _state_dict(D, W, L, Ld, vd, och, seed):
    rs = np.random.RandomState(seed)
    sd = {}
    for name, shape in I.nerf_param_shapes(D, W, O.embed_dim(L), O.embed_dim(Ld) if vd else 0, och, vd)[3:]:
        b = np.sqrt(6.0 / shape[-1]) if name.endswith(".weight") else 0.1
        sd[name] = torch.from_numpy(rs.uniform(-b, b, size=shape))
    return sd


@pytest.mark.parametrize("D,W,L,Ld,vd,och", CASES)
def test_igrad_ref_equals_autograd_of_the_oracle(monkeypatch, D, W, L, Ld, vd, och):
    rs = np.random.RandomState(5)
    B, S = 7, 5
    pts = torch.from_numpy(rs.uniform(-3, 3, size=(B, S, 3))).requires_grad_(True)
    dirs = rs.normal(size=(B, 3))
    dirs = torch.from_numpy(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).requires_grad_(True)
    sd = _state_dict(D, W, L, Ld, vd, och, 11)
    cfg = O.NetCfg(D, W, L, Ld, vd, och)
    z = {}                                   # the pre-activation of every layer, by name, with its gradient kept
    lin = O._lin

    def recording_lin(sd_, name, x):
        z[name] = lin(sd_, name, x)
        z[name].retain_grad()
        return z[name]

    monkeypatch.setattr(O, "_lin", recording_lin)
    raw = O.query(sd, pts, dirs if vd else None, cfg)
    G = torch.from_numpy(rs.normal(size=tuple(raw.shape)))
    (raw * G).sum().backward()
    in_ch, dir_ch = O.embed_dim(L), O.embed_dim(Ld)
    skip = 4 if D > 5 else None
    kw = {}
    if skip is not None:
        kw.update(dZ_skip=z[f"pts_linears.{skip + 1}"].grad.numpy(), W_skip_x=sd[f"pts_linears.{skip + 1}.weight"][:, :in_ch].numpy())
    if vd:
        xd = O.embed(dirs.detach()[:, None, :].expand(B, S, 3).reshape(-1, 3), Ld)
        kw.update(dZ_v=z["views_linears.0"].grad.numpy(), W_v_d=sd["views_linears.0.weight"][:, W:W + dir_ch].numpy(), denc=xd.numpy(),
                  n_freqs_views=Ld)
    d_pts, d_dirs = R.input_grads(z["pts_linears.0"].grad.numpy(), sd["pts_linears.0.weight"].numpy(),
                                  O.embed(pts.detach().reshape(-1, 3), L).numpy(), L, **kw)
    ref = pts.grad.reshape(-1, 3).numpy()
    assert np.abs(d_pts - ref).max() <= 1e-12 * np.abs(ref).max()
    if vd:
        ref_d = dirs.grad.numpy()
        assert np.abs(d_dirs.reshape(B, S, 3).sum(1) - ref_d).max() <= 1e-12 * np.abs(ref_d).max()
    else:
        assert d_dirs is None
