"""An independent torch restatement of LPIPS(net='vgg') 0.1 for the LPIPS tests: F.conv2d / F.max_pool2d in any dtype
on any device, with seeded weights.  `force=` replaces the restatement's own branches (ReLU masks, pool indices) by given ones — the
device oracle.nerf_oracle's `masks=` uses — so that a gradient can be compared ON the branch another implementation took."""
import math

import torch
import torch.nn.functional as F

CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
PAIRS = tuple(dict.fromkeys(CHANNELS))                    # the distinct (Cin, Cout)
POOL_BEFORE = (2, 4, 7, 10)
TAPS = (1, 3, 6, 9, 12)
VGG_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def make_weights(seed=0):
    """{"w": 13 x [Cout, Cin, 3, 3], "b": 13 x [Cout], "lin": 5 x [C]} float32 on the CPU: conv std sqrt(2 / (9 Cin)), bias std 0.05,
    lin uniform [0, 4 / C)."""
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci)) for ci, co in CHANNELS]
    b = [torch.randn(co, generator=g) * 0.05 for _, co in CHANNELS]
    lin = [torch.rand(CHANNELS[l][1], generator=g) * (4.0 / CHANNELS[l][1]) for l in TAPS]
    return {"w": w, "b": b, "lin": lin}


def package_state_dict(wts, lins_prefix=False, scaling=True):
    """The weights under the lpips package's state-dict names."""
    sd = {}
    for l, (idx, sl) in enumerate(zip(VGG_IDX, SLICE_OF)):
        sd[f"net.slice{sl}.{idx}.weight"] = wts["w"][l].clone()
        sd[f"net.slice{sl}.{idx}.bias"] = wts["b"][l].clone()
    for k, v in enumerate(wts["lin"]):
        sd[(f"lins.{k}" if lins_prefix else f"lin{k}") + ".model.1.weight"] = v.reshape(1, -1, 1, 1).clone()
    if scaling:
        sd["scaling_layer.shift"] = torch.tensor(SHIFT).reshape(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor(SCALE).reshape(1, 3, 1, 1)
    return sd


def torchvision_state_dict(wts):
    """torchvision's vgg16 `features.N.*` names plus the package's lin entries."""
    sd = {}
    for l, idx in enumerate(VGG_IDX):
        sd[f"features.{idx}.weight"] = wts["w"][l].clone()
        sd[f"features.{idx}.bias"] = wts["b"][l].clone()
    for k, v in enumerate(wts["lin"]):
        sd[f"lin{k}.model.1.weight"] = v.reshape(1, -1, 1, 1).clone()
    return sd


def trunk(x, wts, force=None):
    """The 13 post-ReLU activations of the scaled batch x [B, 3, H, W] and the branches taken: ({"relu": 13 bool masks,
    "pool": 4 int64 index maps (ATen's flat index inside a plane)}).  With force, those branches are used instead of x's own."""
    dt, dev = x.dtype, x.device
    acts, taken = [], {"relu": [], "pool": []}
    pool = 0
    for l in range(13):
        if l in POOL_BEFORE:
            if force is None:
                x, idx = F.max_pool2d(x, 2, 2, return_indices=True)
            else:
                idx = force["pool"][pool].to(dev)
                B, C, H, W = x.shape
                x = x.reshape(B, C, H * W).gather(2, idx.reshape(B, C, -1)).reshape(B, C, H // 2, W // 2)
            taken["pool"].append(idx)
            pool += 1
        z = F.conv2d(x, wts["w"][l].to(device=dev, dtype=dt), wts["b"][l].to(device=dev, dtype=dt), padding=1)
        if force is None:
            x = F.relu(z)
            m = x > 0
        else:
            m = force["relu"][l].to(dev)
            x = z * m.to(dt)
        taken["relu"].append(m)
        acts.append(x)
    return acts, taken


def head(f0, f1, lin):
    """One tap: mean_{hw} sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 -> [N]"""
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    return ((n0 - n1) ** 2 * lin.to(device=f0.device, dtype=f0.dtype).reshape(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips(x0, x1, wts, force=None):
    """d(x0, x1) for [N, 3, H, W] inputs in [-1, 1] -> (value [N], per-tap [5, N], branches); x0's images come first in the branch
    tensors ([2 N, ...])."""
    N = x0.shape[0]
    shift = torch.tensor(SHIFT, dtype=x0.dtype, device=x0.device).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x0.dtype, device=x0.device).reshape(1, 3, 1, 1)
    x = (torch.cat([x0, x1], 0) - shift) / scale
    acts, taken = trunk(x, wts, force)
    taps = torch.stack([head(acts[l][:N], acts[l][N:], wts["lin"][k]) for k, l in enumerate(TAPS)])
    return taps.sum(0), taps, taken


def branches_of(acts):
    """The force= of the branches an implementation took, from its 13 stored post-ReLU activations: ReLU passes where the stored output
    is > 0, the pool takes ATen's choice on the stored (pre-pool) activation."""
    pool = [F.max_pool2d(acts[l - 1], 2, 2, return_indices=True)[1] for l in POOL_BEFORE]
    return {"relu": [a > 0 for a in acts], "pool": pool}


def images(N, H, W, seed):
    """A pair of smooth-plus-noise image batches in [-1, 1], float32 CPU."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    other = (base + 0.3 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
    return base, other
