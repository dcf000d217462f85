"""One CPU restatement of the four plane arithmetics of the opt-in reduced-precision inference forward (csrc/mlp_fwd_bf.hip), for any
architecture the kernels take: cfg = (D, W, multires, multires_views, skip), view directions always.

  forward64(sd, pts, dirs, cfg, dtype)      NeRF.forward (H:107-130) in `dtype` on points [M, 3] and per-point directions [M, 3]:
                                            float64 is the reference of every bound, float32 (ATen on the CPU) measures what fp32
                                            accumulation costs the network at hand
  forward_planes(sd, pts, dirs, cfg, mode)  the network as the kernel computes it: every GEMM operand split into planes (each plane
                                            the rounding, to nearest even, of what the previous ones left), the kept cross terms
                                            (weight plane, input plane) exactly the kernel's —
                                                NP = 1  (0, 0)            NP = 2  + (0, 1), (1, 0)            NP = 3  + (0, 2), (1, 1), (2, 0)
                                                fp16x2  the NP = 2 set on fp16 planes, with the power-of-two scale rule read from ops
                                            products exact (float64), the accumulator rounded to fp32 ONCE per layer, encodings,
                                            biases and the sigma / rgb heads in fp32.  `flush` (fp16x2): every plane value below
                                            fp16's smallest normal is zero, as a pipe that ignores subnormal inputs would read it.
                                            `drop` / `pair` build the mutants a bound must be able to reject: one kept term (or
                                            several) left out of every GEMM, one term's input plane swapped for another.

What the emulation leaves out is the kernel's fp32 accumulation order (and its own sin / cos): the distance between the two is what
forward64(..., dtype=float32) measures, to a small factor.  tests/test_planes_ref_cpu.py checks this file against the oracle and
against the D8W256 restatement it generalises; tests/test_gpu_plane_inference.py holds the kernels to it."""
import numpy as np
import torch

import _inputs as I

MODES = ("bf16", "bf16x2", "bf16x3", "fp16x2")
TIERS = {"bf16": 1e-1, "bf16x2": 2e-3, "bf16x3": 2e-5, "fp16x2": 2e-5}       # of max(1, max|raw|): the project's tiers
KEPT = {1: [(0, 0)], 2: [(0, 0), (0, 1), (1, 0)], 3: [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]}      # (weight plane, input plane)

# (D, W, multires, multires_views, skip) -> output_ch (half of them 5, half 4; with view directions raw has 4 channels either way)
ARCHS = {
    (1, 128, 10, 4, 4): 5,        # no trunk GEMM
    (2, 256, 10, 4, 4): 4,
    (3, 128, 10, 4, 4): 5,        # odd D
    (6, 256, 10, 4, 4): 4,        # the skip layer is the last trunk layer
    (8, 256, 10, 4, 4): 5,        # the workload's shape
    (8, 128, 10, 4, 4): 4,
    (16, 128, 10, 4, 4): 5,       # deepest
    (4, 128, 10, 4, 0): 4,        # skip right after layer 0
    (8, 256, 10, 4, 2): 5,        # skip 2
    (5, 128, 7, 2, 3): 4,         # shared-panel kernel; 45 and 15 real channels in padded 64 / 32 tiles (skip 3: see UNBUILDABLE)
    (4, 128, 4, 4, 4): 5,         # per-wave only (in_chp = 32)
    (3, 256, -1, -1, 4): 4,       # per-wave only (identity embedding)
    (2, 128, 0, 0, 4): 5,         # per-wave only
}
# D = skip + 1: the reference's constructor builds no wide layer (4 is not in range(D - 1)) while its forward still concatenates
# after layer 4, so feature_linear is mis-shaped — no such model exists, and cn_make_geom refuses the spec.  The architecture
# above carries its purpose (odd D, 7 / 2 frequencies, a skip layer) with the skip one layer earlier.
UNBUILDABLE = (5, 128, 7, 2, 4)


def embed_dim(L):
    return 3 if L < 0 else 3 + 6 * L


def skip_layer(cfg):
    """Index of the trunk layer that reads cat([gamma(x), h]), or None."""
    D, skip = cfg[0], cfg[4]
    return skip + 1 if 0 <= skip and skip + 1 < D else None


def state_dict(cfg, output_ch=4, seed=11, gain=1.0):
    """He-uniform weights and small uniform biases, the rule of _inputs.nerf_state_dict, for any encoding width and skip."""
    D, W, L, Lv, skip = cfg
    rs = np.random.RandomState(seed)
    sd = {}
    for name, shape in I.nerf_param_shapes(D, W, embed_dim(L), embed_dim(Lv), output_ch, True, skips=(skip,)):
        if name in ("temp_rgb", "temp_depth"):
            sd[name] = np.full(shape, -0.7, np.float32)
        elif name == "depth_scale":
            sd[name] = np.full(shape, 1.0, np.float32)
        elif name.endswith(".weight"):
            bound = gain * np.sqrt(6.0 / shape[1])
            sd[name] = rs.uniform(-bound, bound, size=shape).astype(np.float32)
        else:
            sd[name] = rs.uniform(-0.1, 0.1, size=shape).astype(np.float32)
    return sd


def kernel_tensors(sd, D):
    """The parameters in the C-ABI order of include/cnerf.h (NeRF.kernel_tensors) as float32 tensors."""
    names = [f"pts_linears.{l}" for l in range(D)] + ["views_linears.0", "feature_linear", "alpha_linear", "rgb_linear"]
    return [torch.as_tensor(sd[n + k]).float().contiguous() for n in names for k in (".weight", ".bias")]


def embed(x, L):
    if L < 0:
        return x
    out = [x]
    for i in range(L):
        out += [torch.sin(x * 2.0 ** i), torch.cos(x * 2.0 ** i)]
    return torch.cat(out, -1)


def planes_f16(x, flush, n=2):
    out = []
    for _ in range(n):
        h = x.to(torch.float16).to(torch.float32)
        if flush:
            h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
        out.append(h)
        x = x - h          # exact in fp32 (flushed values stay in the residual, and are lost with the last plane)
    return out


def planes_bf16(x, n=2):
    out = []
    for _ in range(n):
        h = x.to(torch.bfloat16).to(torch.float32)
        out.append(h)
        x = x - h
    return out


def forward64(sd, pts, dirs, cfg, dtype=torch.float64):
    D, W, L, Lv, _ = cfg
    s = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    lin = lambda name, x: torch.addmm(s[name + ".bias"], x, s[name + ".weight"].t())      # noqa: E731
    ex, ed = embed(pts.to(dtype), L), embed(dirs.to(dtype), Lv)
    sk = skip_layer(cfg)
    h = ex
    for l in range(D):
        h = torch.relu(lin(f"pts_linears.{l}", torch.cat([ex, h], -1) if l == sk else h))
    sig = lin("alpha_linear", h)
    v = torch.relu(lin("views_linears.0", torch.cat([lin("feature_linear", h), ed], -1)))
    return torch.cat([lin("rgb_linear", v), sig], -1)


def terms_of(mode, drop=None, pair=None):
    """The (weight plane, input plane) products of one GEMM in the order they are summed.  drop: one kept term or a sequence of
    them; pair = (kept term, what is computed in its place)."""
    from consistentnerf_amd import ops
    NP = 2 if mode == "fp16x2" else ops.PRECISION_PLANES[mode]
    terms = list(KEPT[NP])
    if drop is not None:
        drops = [tuple(drop)] if isinstance(drop[0], int) else [tuple(d) for d in drop]
        assert all(d in terms for d in drops), (mode, drop)
        terms = [t for t in terms if t not in drops]
    if pair is not None:
        assert tuple(pair[0]) in terms and max(pair[1]) < NP, (mode, pair)
        terms = [tuple(pair[1]) if t == tuple(pair[0]) else t for t in terms]
    return NP, terms


def forward_planes(sd, pts, dirs, cfg, mode, flush=False, drop=None, pair=None):
    """-> (raw [M, 4] float32, the largest hidden activation or feature in true units).  fp16x2: accumulators in units of
    2^(SW + SX), biases pre-scaled by that factor, head weights by its inverse, activations re-scaled by 2^-SW at the split.  The
    bf16 modes: the same structure without scaling."""
    from consistentnerf_amd import ops
    D, W, L, Lv, _ = cfg
    NP, terms = terms_of(mode, drop, pair)
    if mode == "fp16x2":
        sw, sx = ops.FP16X2_WEIGHT_SHIFT, ops.FP16X2_ACT_SHIFT
        wplanes = lambda w: planes_f16(w * 2.0 ** sw, flush)                  # noqa: E731  (pack: scale, then split)
        enc = lambda x: planes_f16(x * 2.0 ** sx, flush)                      # noqa: E731
        act = lambda a: planes_f16(a * 2.0 ** -sw, flush)                     # noqa: E731  (accumulator -> 2^sx * activation)
        acc_scale = 2.0 ** (sw + sx)
    else:
        wplanes = enc = act = lambda x: planes_bf16(x, NP)                    # noqa: E731
        acc_scale = 1.0
    g = lambda k: torch.as_tensor(sd[k]).float()                             # noqa: E731

    def gemm(wp, xp):      # the kept cross terms, exact products, wide accumulation
        out = None
        for i, j in terms:
            t = xp[j].double() @ wp[i].double().T
            out = t if out is None else out + t
        return out if out is not None else torch.zeros(xp[0].shape[0], wp[0].shape[0], dtype=torch.float64)

    ex, ed = embed(pts, L), embed(dirs, Lv)
    ic, sk = ex.shape[1], skip_layer(cfg)
    acc = (gemm(wplanes(g("pts_linears.0.weight")), enc(ex)) + (g("pts_linears.0.bias") * acc_scale).double()).float()
    amax = 0.0
    for l in range(1, D):
        w = g(f"pts_linears.{l}.weight")
        h = torch.relu(acc)
        amax = max(amax, float(h.abs().max()) / acc_scale)
        if l == sk:        # the skip layer: its input is cat([gamma(x), h])
            a = gemm(wplanes(w[:, ic:].contiguous()), act(h)) + gemm(wplanes(w[:, :ic].contiguous()), enc(ex))
        else:
            a = gemm(wplanes(w), act(h))
        acc = (a + (g(f"pts_linears.{l}.bias") * acc_scale).double()).float()
    h = torch.relu(acc)
    amax = max(amax, float(h.abs().max()) / acc_scale)
    sig = (h.double() @ (g("alpha_linear.weight") / acc_scale).double().T).float() + g("alpha_linear.bias")
    feat = (gemm(wplanes(g("feature_linear.weight")), act(h)) + (g("feature_linear.bias") * acc_scale).double()).float()
    amax = max(amax, float(feat.abs().max()) / acc_scale)
    wv = g("views_linears.0.weight")
    v = (gemm(wplanes(wv[:, :W].contiguous()), act(feat)) + gemm(wplanes(wv[:, W:].contiguous()), enc(ed))
         + (g("views_linears.0.bias") * acc_scale).double()).float()
    rgb = (torch.relu(v).double() @ (g("rgb_linear.weight") / acc_scale).double().T).float() + g("rgb_linear.bias")
    return torch.cat([rgb, sig], -1), amax


def dist(a, ref64, scale):
    return float((a.double() - ref64).abs().max()) / scale


def rel_dist(a, b, ref64):
    """max |a - b| / |ref64| elementwise: the crafted family's measure (every output there is positive and of order 1)."""
    return float(((a.double() - b.double()).abs() / ref64.abs()).max())


# ------------------------------------------------------------------------------------------------ inputs
SHAPES = {1: (1, 1), 33: (3, 11), 127: (1, 127), 128: (4, 32), 129: (43, 3), 161: (7, 23)}      # M -> (B rays, S points per ray)


def points(M, seed=5):
    """Points uniform in [-3, 3]^3 and one unit direction per ray, as tests/test_gpu_bf16x3_training.py::_points draws them ->
    float32 (pts [M, 3], dirs [B, 3])."""
    B, S = SHAPES[M]
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-3, 3, size=(B, S, 3)).astype(np.float32).reshape(-1, 3)
    dirs = rs.normal(size=(B, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    return torch.from_numpy(pts), torch.from_numpy(dirs)


def rays(M, seed=6):
    """The same kind of cloud reached the other way (…::_rays): ray rows [B, 11] = (o, d, near, far, unit d) and depths [B, S]
    with |o_i| <= 1, 1 <= |d| <= 1.3, z in [0, 1.5]: every o + d z stays inside [-3, 3]^3."""
    B, S = SHAPES[M]
    rs = np.random.RandomState(seed)
    o = rs.uniform(-1, 1, size=(B, 3))
    d = rs.normal(size=(B, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rs.uniform(1.0, 1.3, size=(B, 1))
    vd = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rows = np.concatenate([o, d, np.zeros((B, 1)), np.full((B, 1), 1.5), vd], 1).astype(np.float32)
    return torch.from_numpy(rows), torch.from_numpy(rs.uniform(0.0, 1.5, size=(B, S)).astype(np.float32))


def per_point(dirs, M):
    B, S = SHAPES[M]
    return dirs[:, None, :].expand(B, S, 3).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ the crafted family
# Operands whose planes are ALL maximal and of one sign, so that no kept cross term can hide: a positive float32 whose low mantissa
# bits are TAIL[mode].  0x7FBF = 0 1111111 1 0 111111: plane 0 rounds down, plane 1 is the eight ones that follow (2^-8 of the
# operand), plane 2 the last six (2^-17); 0x7F00 stops after plane 1; 0xFFC = 0 1111111111 00 is the same for fp16's 11-bit planes
# (plane 1 = 2^-11 of the operand).  With these tails the planes sum to the operand exactly.
TAIL = {"bf16x3": (0x7FBF, 16), "bf16x2": (0x7F00, 16), "fp16x2": (0xFFC, 13)}


def crafted(shape, mode, lo_exp, hi_exp, seed):
    """Positive float32 values in [2^lo_exp, 2^(hi_exp + 1)): random exponent, random leading mantissa bits, the mode's tail."""
    tail, bits = TAIL[mode]
    rs = np.random.RandomState(seed)
    e = rs.randint(lo_exp, hi_exp + 1, size=shape).astype(np.int64) + 127
    top = rs.randint(0, 1 << (23 - bits), size=shape).astype(np.int64)
    word = (e << 23) | (top << bits) | tail
    return word.astype(np.uint32).view(np.float32).reshape(shape)


def crafted_net(W, L, Lv, mode, which, shift=0, seed=3):
    """A network of non-negative weights and zero biases in which ONE GEMM meets crafted operands on both sides and every other
    layer hands values on through a single power-of-two weight per row -> (cfg, state dict).
      which = "reg"   D = 2: pts_linears.0 selects a raw coordinate per unit with a power-of-two gain (h0 = 2^g x_c, exactly, crafted
                      like x); pts_linears.1, the register-operand GEMM, is crafted: sums of one sign over ONE K-step of 16 inputs
                      per unit (unit n reads inputs 16 ((n + shift) mod W / 16) + [0, 16): adding exact zeros costs nothing, and
                      a narrow sum keeps fp32 accumulation error, which the bound is made of, well below what one lost term
                      moves); the watched units see four K-steps per network, shift = 0, 4, 8, 12 all sixteen of W = 256
      which = "lds"   D = 1: pts_linears.0, the LDS-operand GEMM, is crafted on the three raw coordinates
    sigma (an fp32 head: no split between the crafted GEMM and raw) and the three colours (through feature_linear and
    views_linears.0, which re-split their input: exact at three bf16 planes only) read four units of the last trunk layer, one per
    32-row tile where W allows."""
    D = 2 if which == "reg" else 1
    cfg = (D, W, L, Lv, 4)
    sd = {k: np.zeros_like(v) for k, v in state_dict(cfg, 4, 0).items()}
    ar = np.arange(W)
    if which == "reg":
        sd["pts_linears.0.weight"][ar, ar % 3] = (2.0 ** -(ar % 3)).astype(np.float32)
        win = (ar[None, :] // 16) == ((ar[:, None] + shift) % (W // 16))
        sd["pts_linears.1.weight"][:] = np.where(win, crafted((W, W), mode, -6, -4, seed), np.float32(0))
    else:
        sd["pts_linears.0.weight"][:, :3] = crafted((W, 3), mode, -3, -1, seed)
    watch = [5, W // 4 + 6, W // 2 + 7, W - 24]              # tiles 0, 1, 2, 3 at W = 128; 0, 2, 4, 7 at W = 256
                                                             # (n mod 16 = 5, 6, 7, 8 and n mod 8 = 5, 6, 7, 0)
    sd["alpha_linear.weight"][0, watch[3]] = 1.0
    for c in range(3):
        sd["feature_linear.weight"][c, watch[c]] = 2.0
        sd["views_linears.0.weight"][c, c] = 0.5
        sd["rgb_linear.weight"][c, c] = 1.0
    return cfg, sd


def crafted_columns(mode):
    """The raw columns whose path from the crafted GEMM re-splits nothing inexactly: all four at three bf16 planes (24 bits: every
    fp32 value splits exactly), sigma alone at two planes (there feature_linear and views_linears.0 round their input to 16 / 22 bits,
    and a last-bit difference in front of a rounding boundary comes out as a whole step)."""
    return slice(0, 4) if mode == "bf16x3" else slice(3, 4)


def crafted_points(M, mode, seed=4):
    """Crafted positive coordinates in [0.5, 4) and unit directions -> float32 (pts [M, 3], dirs [B, 3])."""
    return torch.from_numpy(crafted((M, 3), mode, -1, 1, seed)), points(M)[1]


# (W, multires, multires_views, which, shift): both kernels' shapes and the per-wave-only encoding; every K-step of the register GEMM
CRAFTED = ([(256, 10, 4, "reg", sh) for sh in (0, 4, 8, 12)] + [(128, 10, 4, "reg", sh) for sh in (0, 4)] + [(128, 4, 4, "reg", 0)]
           + [(W, L, Lv, "lds", 0) for W, L, Lv in ((256, 10, 4), (128, 10, 4), (128, 4, 4))])


# ------------------------------------------------------------------------------------------------ fp16x2 across its stated range
RANGE_CFGS = [(4, 128, 10, 4, 4), (8, 256, 10, 4, 4)]
RANGE_FAMILIES = ("cold6", "cold9", "hot", "wide")


def range_net(cfg, family, seed=11):
    """The random-init network of `cfg` moved to one end of what the fp16x2 header states:
      cold6 / cold9  pts_linears.1 (weights and bias) times 2^-6 / 2^-9, pts_linears.2 weights divided by the same: the same
                     function (ReLU is positively homogeneous) through a layer whose activations and weights sit 2^6 / 2^9 lower,
                     where the low fp16 planes are subnormal
      hot            pts_linears.0 (weights and bias) times 64: activations in the hundreds
      wide           weights of magnitude 200 (the limit is 255.8) where the contracted input is bounded — three raw-coordinate
                     columns of pts_linears.0 and two direction columns of views_linears.0 — and one in the register GEMM of
                     pts_linears.1 on a unit of h0 that is scaled down to 2^-6 of the unscaled network's; pts_linears.0 times 256 first, so that hidden
                     activations reach the low thousands (the limit is 4094)"""
    sd = {k: v.copy() for k, v in state_dict(cfg, 4, seed).items()}
    D, W = cfg[0], cfg[1]
    if family.startswith("cold"):
        f = np.float32(2.0 ** -int(family[4:]))
        sd["pts_linears.1.weight"] *= f
        sd["pts_linears.1.bias"] *= f
        sd["pts_linears.2.weight"] /= f
    elif family == "hot":
        sd["pts_linears.0.weight"] *= np.float32(64.0)
        sd["pts_linears.0.bias"] *= np.float32(64.0)
    elif family == "wide":
        sd["pts_linears.0.weight"] *= np.float32(256.0)
        sd["pts_linears.0.bias"] *= np.float32(256.0)
        for n, c, s in ((3, 0, 200.0), (W // 2 + 1, 1, -200.0), (W - 2, 2, 200.0)):
            sd["pts_linears.0.weight"][n, c] = s
        sd["pts_linears.0.weight"][7] *= np.float32(2.0 ** -14)
        sd["pts_linears.0.bias"][7] = np.float32(2.0 ** -6)
        sd["pts_linears.1.weight"][W // 4 + 2, 7] = 200.0
        sd["views_linears.0.weight"][5, W + 1] = 200.0
        sd["views_linears.0.weight"][W // 2 - 3, W + 2] = -200.0
    else:
        raise ValueError(family)
    return sd
