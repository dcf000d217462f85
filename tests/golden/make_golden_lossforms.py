#!/usr/bin/env python3
"""Golden-vector generator for the loss forms other than `--hardmask`. Runs ONLY in the build container (needs the reference
checkout), in the manner of make_golden.py: the reference's own modules are imported with the IO-only third-party modules stubbed,
its lambdas are called and its inline statements are read from its source at generation time and exec'd on seeded inputs; the
*outputs* (arrays only) go to lossforms.npz next to this file. No reference source, bytecode or pickled object is written.

  soft.*   img2mse_softmask / img2mse_depth_softmask (run_nerf_view.py:47-58) on seeded colours [173, 3] and depths [173] at two
           temperatures, softplus(-0.7) and 0.1: loss, d / dx, d / dtemp
  norm.* plain.* coef.*
           the `--with_depth_norm` and plain depth lines (run_nerf_view.py:1730-1773) and the hard-mask depth lines that keep the
           hardmask_coef term (run_nerf_view_cal_correspondance.py:1543-1551) on a 512-ray batch, with a mixed mask and with an
           all-ones mask (the `!= N_rand` guard): depth_loss, d / d depth_pred, and the prior as the lines leave it

usage:  python tests/golden/make_golden_lossforms.py
"""
import os
import sys
import textwrap
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = "/root/reference/nerf-pytorch-master"

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

torch.set_num_threads(8)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference():
    for n in ("imageio", "cv2", "ipdb"):
        _stub(n)
    _stub("tensorboardX", SummaryWriter=object)
    _stub("pytorch_msssim", ssim=None, ms_ssim=None)

    class _LPIPS:  # instantiated at import time
        def __init__(self, *a, **k):
            pass

        def to(self, *a, **k):
            return self

    _stub("lpips", LPIPS=_LPIPS)
    torch.cuda.current_device = lambda: 0
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.LongTensor = torch.LongTensor
    sys.path.insert(0, REF)
    import run_nerf_view as V
    return V


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def ref_lines(path, first, last, must_contain):
    """Lines [first, last] (1-based) of a reference source file, dedented: read now, exec'd, never stored."""
    lines = open(path).read().split("\n")[first - 1:last]
    assert must_contain in lines[0], (lines[0], must_contain)
    return textwrap.dedent("\n".join(lines))


FAR = 6.0
N_RAND = 512
TEMPS = (("sp", float(F.softplus(torch.tensor(-0.7)))), ("p1", 0.1))


def inputs():
    rs = np.random.RandomState(173)
    x3, y3 = rs.uniform(size=(173, 3)).astype(np.float32), rs.uniform(size=(173, 3)).astype(np.float32)
    x1, y1 = rs.uniform(0.2, 1.0, size=(173,)).astype(np.float32), rs.uniform(0.2, 1.0, size=(173,)).astype(np.float32)
    depth = rs.uniform(1.2, FAR, size=(N_RAND,)).astype(np.float32)
    prior = rs.uniform(1.2, FAR, size=(N_RAND,)).astype(np.float32)
    mask = (rs.uniform(size=(N_RAND,)) < 0.55).astype(np.float32)
    return dict(x3=x3, y3=y3, x1=x1, y1=y1, depth=depth, prior=prior, mask=mask)


def main():
    V = import_reference()
    out = inputs()
    for tname, tval in TEMPS:
        out[f"temp.{tname}"] = np.float32(tval)
        for tag, fn, (x, y) in (("rgb", V.img2mse_softmask, (out["x3"], out["y3"])),
                                ("depth", V.img2mse_depth_softmask, (out["x1"], out["y1"]))):
            xt = T(x).requires_grad_(True)
            tt = torch.tensor(np.float32(tval)).requires_grad_(True)
            loss = fn(xt, T(y), tt)
            loss.backward()
            out[f"soft.{tag}.{tname}.loss"], out[f"soft.{tag}.{tname}.d_x"], out[f"soft.{tag}.{tname}.d_temp"] = loss.detach(), xt.grad, tt.grad
    v_block = ref_lines(os.path.join(REF, "run_nerf_view.py"), 1730, 1773, "if args.with_depth_loss:")
    vc_block = ref_lines(os.path.join(REF, "run_nerf_view_cal_correspondance.py"), 1543, 1551, "if args.with_depth_loss:")
    flags = dict(with_depth_loss=True, hardmask=False, softmask=False, softLpmask=False, with_depth_norm=False, hardmask_coef=0.2)
    for mtag, mask in (("mixed", out["mask"]), ("ones", np.ones(N_RAND, np.float32))):
        for form, block, over in (("norm", v_block, dict(with_depth_norm=True)), ("plain", v_block, {}),
                                  ("coef", vc_block, dict(hardmask=True))):
            dp = T(out["depth"]).requires_grad_(True)
            ns = dict(torch=torch, args=types.SimpleNamespace(**dict(flags, **over)), depth_pred=dp, depth_cas_s=T(out["prior"]).clone(),
                      mask_cas_s=T(mask)[:, None], N_rand=N_RAND, far=FAR, img2mse=V.img2mse, img2mse_softLpmask=V.img2mse_softLpmask,
                      img2mse_depth_softmask=V.img2mse_depth_softmask, F=F, render_kwargs_train={})
            exec(block, ns)
            ns["depth_loss"].backward()
            tag = f"{form}.{mtag}."
            out[tag + "loss"], out[tag + "d_depth"], out[tag + "prior_after"] = ns["depth_loss"].detach(), dp.grad, ns["depth_cas_s"]
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "lossforms.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote lossforms.npz ({os.path.getsize(path) / 1024:.1f} KiB), {len(arrays)} arrays")


if __name__ == "__main__":
    main()
