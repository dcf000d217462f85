"""Records tests/golden/depthvis.npz from the reference's depth visualiser (alky/vis_utils.py: lky_visualize_depth, save_img_u8)
and, with --write-lut, writes consistentnerf_amd/csrc/turbo_lut.hpp from matplotlib's public `turbo` colormap.

    python tests/golden/make_golden_depthvis.py --reference <reference checkout>/nerf-pytorch-master [--write-lut]

Needs numpy, matplotlib and PIL; the reference's two unused imports (pytorch_msssim, ipdb) are stubbed.  The archive holds arrays
only: per frame k  disp_k, acc_k [H, W] float32 (disp NaN where acc == 0), img_k [H, W, 3] float64 (lky_visualize_depth(1 / disp,
acc)), u8_k [H, W, 3] uint8 (the PNG save_img_u8 wrote, read back), and lut [256, 3] float64 (the colormap at 0..255).
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def frame(H, W, seed, kind="scene"):
    """depth smooth plus noise; acc a clipped smooth ramp (plateaus of exact 0 and 1) plus an explicit block of each."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = (2.5 + 1.5 * np.sin(3.1 * xx + 0.4) * np.cos(2.3 * yy) + 0.8 * yy + 0.05 * rs.standard_normal((H, W))).astype(np.float32)
    acc = np.clip(1.5 * (0.5 + 0.5 * np.sin(4.0 * xx - 1.0) * np.cos(3.0 * yy + 0.5)) - 0.2 + 0.02 * rs.standard_normal((H, W)), 0, 1)
    acc = acc.astype(np.float32)
    acc[H // 8:H // 3, W // 10:W // 4] = 0.
    acc[H // 2:H // 2 + H // 5, W // 2:W // 2 + W // 4] = 1.
    if kind == "single":
        w = acc[H // 2, W // 3] if acc[H // 2, W // 3] > 0 else np.float32(0.75)
        acc[:] = 0.
        acc[H // 2, W // 3] = w
    elif kind == "empty":
        acc[:] = 0.
    disp = (1. / depth).astype(np.float32)
    disp[acc == 0] = np.nan
    return disp, acc


FRAMES = [(48, 64, 11, "scene"), (161, 176, 12, "scene"), (48, 64, 13, "single"), (48, 64, 14, "empty")]


def load_reference(path):
    for name in ("pytorch_msssim", "ipdb"):
        m = types.ModuleType(name)
        m.ssim = m.ms_ssim = m.set_trace = None
        sys.modules.setdefault(name, m)
    import matplotlib
    import matplotlib.cm as cm
    if not hasattr(cm, "get_cmap"):          # removed from matplotlib.cm in 3.9; the registry holds the same object
        cm.get_cmap = matplotlib.colormaps.get_cmap
    sys.path.insert(0, os.path.join(path, "alky"))
    import vis_utils
    return vis_utils, cm


def write_lut(lut, path):
    rows = ",\n".join("    {%s}" % ", ".join("%.9gf" % v for v in np.float32(row)) for row in lut)
    with open(path, "w") as f:
        f.write("// matplotlib's `turbo` colormap (matplotlib.colormaps['turbo'] at 0..255, RGB), rounded to fp32.  Written by\n"
                "// tests/golden/make_golden_depthvis.py --write-lut; tests/golden/depthvis.npz pins it (tests/test_depthvis_cpu.py).\n"
                "#pragma once\n\n__device__ const float CN_TURBO_LUT[256][3] = {\n" + rows + "\n};\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--write-lut", action="store_true")
    args = ap.parse_args()
    V, cm = load_reference(args.reference)
    from PIL import Image
    out = {"lut": np.asarray(cm.get_cmap("turbo")(np.arange(256)))[:, :3].astype(np.float64)}
    with tempfile.TemporaryDirectory() as tmp, np.errstate(all="ignore"):
        for k, (H, W, seed, kind) in enumerate(FRAMES):
            disp, acc = frame(H, W, seed, kind)
            img = V.lky_visualize_depth(1 / disp, acc)
            pth = os.path.join(tmp, "f.png")
            V.save_img_u8(img, pth)
            out.update({f"disp_{k}": disp, f"acc_{k}": acc, f"img_{k}": np.asarray(img, dtype=np.float64),
                        f"u8_{k}": np.asarray(Image.open(pth))})
    dst = os.path.join(HERE, "depthvis.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")
    if args.write_lut:
        write_lut(out["lut"], os.path.join(ROOT, "consistentnerf_amd", "csrc", "turbo_lut.hpp"))


if __name__ == "__main__":
    main()
