"""The argument-rule cases of the forward's C entry points (mlp_fwd.hip, mlp_fwd_bf.hip, sampling.hip, render.hip): per entry point
one call that passes validation, every pointer nulled in turn (struct fields included), the sizes at their edges, the architectures
inside and outside the envelope, and the double faults that pin which code wins.  tests/test_fwd_host_rules.py replays them through
_closs_rule_cases.run (dummy host buffers, a child process that sees no device) and compares the return codes with
tests/golden/fwd_arg_rules.json, which tests/golden/make_golden_closs_rules.py wrote from the library of the commit BEFORE the
forward's host path was rewritten.

Same case format as tests/_closs_rule_cases.py; the struct arguments here are Net, Ptrs, RenderCfg, RenderOut, RenderGrads, RayGen and Rng
of consistentnerf_amd/_lib.py.  A call that passes validation stops at its first launch (no device: 100), the shared-panel plane
forwards one step earlier at the LDS opt-in (-3); cnerf_render_ws_floats returns a size."""
from _closs_rule_cases import P_, null_variants

NET = ("Net", dict(D=8, W=256, multires=10, multires_views=4, use_viewdirs=1, output_ch=5, skip=4))
CFG = ("RenderCfg", dict(Nc=8, Nf=8, lindisp=0, white_bkgd=0, ray_stride=11, train=0))
OUT = ("RenderOut", {k: P_ for k in ("rgb_map", "disp_map", "acc_map", "depth_map", "rgb0", "disp0", "acc0", "depth0", "z_std", "raw",
                                    "z_vals", "weights")})
GRADS = ("RenderGrads", {k: P_ for k in ("g_rgb_map", "g_disp_map", "g_acc_map", "g_depth_map", "g_rgb0", "g_disp0", "g_acc0", "g_depth0")})
CAM = ("RayGen", dict(H=4, W=4, fx=50.0, fy=50.0, cx=2.0, cy=2.0, near=1.0, far=6.0, use_viewdirs=1, ndc=0, ndc_ax=0.0, ndc_ay=0.0, first=0))
RNG = ("Rng", dict(seed=7, offset=0, state_dev=P_, row0=0))
ROWS = dict(pts=None, rays=P_, ray_stride=11, dirs=None, z=P_)
NETS = dict(coarse=NET, packed_coarse=P_, fine=NET, packed_fine=P_)
SAMPLES = dict(t_vals=P_, t_rand=None, u=P_, u_row_stride=0, noise0=None, noise1=None, out=OUT, workspace=P_, stream=None)

# (the order of the arguments IS the C order of each entry point: run() checks the count against SIGNATURES)
BASE = {
    "cnerf_mlp_fwd": dict(net=NET, packed=P_, **ROWS, B=4, S=8, raw=P_, stash=None, stream=None),
    "cnerf_mlp_fwd_live": dict(net=NET, packed=P_, rays=P_, ray_stride=11, z=P_, B=4, S=32, raw=P_, stash=P_, live_rays=P_, stream=None),
    "cnerf_mlp_fwd_embedded": dict(net=NET, packed=P_, x_embedded=P_, M=32, raw=P_, stash=None, stream=None),
    "cnerf_mlp_fwd_bf": dict(net=NET, packed_bf=P_, planes=3, **ROWS, B=4, S=8, raw=P_, stream=None),
    "cnerf_mlp_fwd_bf_train": dict(net=NET, packed_bf=P_, **ROWS, B=4, S=8, raw=P_, stash=P_, stream=None),
    "cnerf_coarse_z": dict(rays=P_, ray_stride=8, B=4, Nc=8, t_vals=P_, t_rand=None, lindisp=0, z=P_, stream=None),
    "cnerf_coarse_z_rng": dict(rays=P_, ray_stride=8, B=4, Nc=8, t_vals=P_, rng=RNG, lindisp=0, z=P_, stream=None),
    "cnerf_resample": dict(z=P_, weights=P_, u=P_, u_row_stride=8, B=4, Nc=8, Nf=8, z_fine=P_, z_std=P_, samples=None, inds=None, stream=None),
    "cnerf_resample_rng": dict(z=P_, weights=P_, rng=RNG, B=4, Nc=8, Nf=8, z_fine=P_, z_std=P_, samples=None, inds=None, stream=None),
    "cnerf_sample_pdf": dict(bins=P_, weights=P_, u=P_, u_row_stride=8, B=4, Nb=8, Nf=8, samples=P_, inds=None, stream=None),
    "cnerf_render_ws_floats": dict(coarse=NET, fine=NET, cfg=CFG, B=16),
    "cnerf_render_fwd": dict(NETS, rays=P_, B=16, cfg=CFG, **SAMPLES),
    "cnerf_render_fwd_cam": dict(NETS, cam=CAM, B=16, cfg=CFG, **SAMPLES),
    "cnerf_render_bwd": dict(NETS, rays=P_, B=16, cfg=("RenderCfg", dict(CFG[1], train=1)), noise0=None, noise1=None, g=GRADS, workspace=P_,
                             grads_coarse=("Ptrs", {}), grads_fine=("Ptrs", {}), accumulate=0, stream=None),
}
PLANE_ENTRIES = ("cnerf_mlp_fwd_bf", "cnerf_mlp_fwd_bf_train")
# name -> Net fields: the three compiled widths with view directions, one network without them, one width outside the envelope
ARCHS = {"d8w256": {}, "d2w128": dict(D=2, W=128), "d2w64": dict(D=2, W=64), "d8w256.novd": dict(use_viewdirs=0), "w96": dict(W=96)}


def _variants(entry, base):
    v = null_variants(base)
    nets = [k for k in ("net", "coarse", "fine") if k in base]
    arch = lambda a: {f"{n}.{f}": x for n in nets for f, x in ARCHS[a].items()}  # noqa: E731
    for a in ARCHS if nets else ():
        v[f"arch.{a}"] = arch(a)
    bname = "M" if "M" in base else "B"
    v["B.neg"], v["B.zero"] = {bname: -1}, {bname: 0}
    out = next(k for k in ("raw", "z", "z_fine", "samples", "out", "workspace", "cfg") if k in base)     # an output (or needed) pointer
    v[f"B.zero+null.{out}"] = {bname: 0, out: None}
    if nets:
        v[f"arch.w96+null.{out}"] = dict(arch("w96"), **{out: None})
    for name in ("S", "Nc"):
        if name in base:
            for n in (0, 2, 3):
                v[f"{name}.{n}"] = {name: n}
    if "ray_stride" in base:
        for n in (5, 7, 8, 10, 11):
            v[f"ray_stride.{n}"] = {"ray_stride": n}
    if "dirs" in base:      # the points form, and each ray-row stride with explicit directions / without a view branch
        v["points"] = {"pts": P_, "dirs": P_, "rays": None, "z": None}
        v["points.null.dirs"] = {"pts": P_, "rays": None, "z": None}
        v["points.null.dirs.ray_stride.11"] = {"pts": P_, "z": None}
        v["points.null.dirs.ray_stride.8"] = {"pts": P_, "z": None, "ray_stride": 8}
        for n in (7, 8, 10):
            v[f"ray_stride.{n}.dirs"] = {"ray_stride": n, "dirs": P_}
            v[f"ray_stride.{n}.novd"] = dict(arch("d8w256.novd"), ray_stride=n)
    if entry in ("cnerf_mlp_fwd", "cnerf_mlp_fwd_embedded"):
        v["stash"] = {"stash": P_}
    if entry == "cnerf_mlp_fwd_live":
        v["S.33"], v["S.64"], v["B.zero+S.33"] = {"S": 33}, {"S": 64}, {"B": 0, "S": 33}
        v["ray_stride.8.novd"] = dict(arch("d8w256.novd"), ray_stride=8)
    if "planes" in base:
        for n in (0, 1, 2, 3, 4, 18):
            v[f"planes.{n}"] = {"planes": n}
        v["planes.0+arch.w96"] = dict(arch("w96"), planes=0)
        v["planes.0+null.raw"] = {"planes": 0, "raw": None}
        v["planes.18.d2w128"] = dict(arch("d2w128"), planes=18)
    if "t_rand" in base:
        v["t_rand"] = {"t_rand": P_}
    if "Nf" in base:
        v["Nf.neg"], v["Nf.zero"] = {"Nf": -1}, {"Nf": 0}
    if entry in ("cnerf_resample", "cnerf_resample_rng"):      # Nc - 1 <= 256 CDF entries, Nc + Nf <= 1024 depths
        v["Nc.257"], v["Nc.258"] = {"Nc": 257}, {"Nc": 258}
        v["all.1024"], v["all.1025"] = {"Nc": 200, "Nf": 824}, {"Nc": 200, "Nf": 825}
        v["Nc.258+null.z"], v["Nc.258+Nf.zero"] = {"Nc": 258, "z": None}, {"Nc": 258, "Nf": 0}
        v["Nc.258+null.source"] = {"Nc": 258, ("u" if "u" in base else "rng"): None}
        v["samples"] = {"samples": P_, "inds": P_}
    if entry == "cnerf_sample_pdf":
        v["Nb.1"], v["Nb.2"], v["Nb.256"], v["Nb.257"] = {"Nb": 1}, {"Nb": 2}, {"Nb": 256}, {"Nb": 257}
        v["Nb.257+null.u"], v["inds"] = {"Nb": 257, "u": None}, {"inds": P_}
    if "cfg" in base:
        for n in (0, 2, 3):
            v[f"Nc.{n}"] = {"cfg.Nc": n}
        v["Nf.neg"], v["Nf.zero"], v["Nf.zero.null.u"] = {"cfg.Nf": -1}, {"cfg.Nf": 0}, {"cfg.Nf": 0, "u": None}
        v["Nc.258"], v["all.1025"] = {"cfg.Nc": 258}, {"cfg.Nc": 200, "cfg.Nf": 825}
        for n in (8, 9, 11):
            v[f"cfg.ray_stride.{n}"] = {"cfg.ray_stride": n}
            v[f"cfg.ray_stride.{n}.novd"] = dict(arch("d8w256.novd"), **{"cfg.ray_stride": n})
        v["cfg.ray_stride.8.fine_only_vd"] = {"cfg.ray_stride": 8, "coarse.use_viewdirs": 0}
        v["train.set"], v["train.cleared"] = {"cfg.train": 1}, {"cfg.train": 0}
        v["no_fine"] = {"fine": None, "packed_fine": None, "grads_fine": None}
        v["no_fine.packed_fine"] = {"fine": None}
    if "cam" in base:
        v["cam.last_pixel"], v["cam.past_last_pixel"], v["cam.B.17"] = {"cam.first": 0, "B": 16}, {"cam.first": 1}, {"B": 17}
        v["cam.fx.zero"], v["cam.fy.zero"], v["cam.first.neg"], v["cam.H.zero"] = {"cam.fx": 0.0}, {"cam.fy": 0.0}, {"cam.first": -1}, {"cam.H": 0}
        v["cam.no_viewdirs"] = {"cam.use_viewdirs": 0}
        v["train.set+null.cam"] = {"cfg.train": 1, "cam": None}
        v["cam.B.17+null.packed_coarse"] = {"B": 17, "packed_coarse": None}
        v["cam.B.17+Nc.0"], v["cam.fx.zero+B.17"] = {"B": 17, "cfg.Nc": 0}, {"cam.fx": 0.0, "B": 17}
    return {k: {a: x for a, x in ch.items() if a.split(".")[0] in base} for k, ch in v.items()}


def cases():
    out = []
    for entry, base in BASE.items():
        for suffix, change in _variants(entry, base).items():
            out.append((f"{entry}:{suffix}", entry, base, change))
            if entry in PLANE_ENTRIES:      # both kernels of the switch
                out.append((f"{entry}:{suffix}:perwave", entry, base, dict(change, **{"$CNERF_BF_PERWAVE": "1"})))
    return out
