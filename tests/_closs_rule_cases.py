"""The argument-rule cases of the folded step loss: the sixteen C entry points of composite.hip and the six loss tails of loss.hip,
each with one call that passes validation and one call per rule broken (tests/test_closs_host_rules.py replays them against the
library and compares the return codes with tests/golden/closs_arg_rules.json, which tests/golden/make_golden_closs_rules.py wrote
from the library of the commit BEFORE the host path was rewritten).

Dummy host buffers stand in for the device pointers: validation dereferences none of them, and run() refuses to issue a single
call where a device is visible — a call that passes validation would hand host pointers to a kernel.  run() is therefore only ever
called in a child process whose environment hides the devices (HIP_VISIBLE_DEVICES=-1): there such a call ends in
hipErrorNoDevice (100) at the launch.

A case is (name, entry point, base call, {argument or struct.field: value}); the base call is an ordered {argument: value} whose
struct arguments are ("Closs" | "ClossTail" | "LossForm", {field: value}) and whose coins are ("coins", 4 ints)."""
import copy
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 520, 32            # two 16 x 16 patches + 8 rays
P_, Q_ = "P", "Q"         # the dummy buffer, and the same 4 bytes on (misaligned for the fp64 partials)

NINE = dict(raw=P_, raw_ch=4, z=P_, rays=P_, ray_stride=8, noise=None, B=B, S=S, white=0)
OUTS = dict(rgb=P_, disp=P_, acc=P_, depth=P_, weights=P_)
CLOSS = ("Closs", dict(target=P_, mask=P_, prior=P_, far=6.0, seg_row=0))
FORM = ("LossForm", dict(rgb_form=2, depth_form=5, lp_coef=1.0, temp_rgb=P_, temp_depth=P_))
TAIL = ("ClossTail", dict(ws_last=P_, ws_coarse=P_, B=B, counts=None, coef=0.2, far=6.0, rgb_w=1.0, depth_w=1.0, patch_w=0.001, has_depth=1,
                          depth_last=P_, depth_coarse=P_, mono=P_, P=2, n=256))
SEEDS = dict(rgb=P_, depth=P_, stats=P_, g_loss=P_, rgb_w=1.0, depth_w=1.0, patch_w=0.001)
PATCH = dict(patch_d=P_, n_patch=512)
SSIM_SEEDS = dict(ssim_w=0.5, ssim_d=P_, n_ssim=512)
SSIM_TAIL = dict(ssim_P=2, ssim_w=0.5, rgb_last=P_, rgb_coarse=P_, target=P_)


def _tail(**kw):
    return ("ClossTail", dict(TAIL[1], **kw))


BASE = {
    "cnerf_composite_fwd": dict(NINE, **OUTS, stream=None),
    "cnerf_composite_bwd": dict(NINE, g_rgb=P_, g_disp=P_, g_acc=P_, g_depth=P_, d_raw=P_, stream=None),
    "cnerf_composite_fwd_mse": dict(NINE, target=P_, loss_add=P_, **OUTS, loss=P_, workspace=P_, counter=P_, stream=None),
    "cnerf_composite_bwd_mse": dict(NINE, rgb=P_, target=P_, g_loss=P_, d_raw=P_, stream=None),
    "cnerf_composite_fwd_closs": dict(NINE, L=CLOSS, **OUTS, workspace=P_, stream=None),
    "cnerf_composite_fwd_lossform": dict(NINE, L=CLOSS, F=FORM, **OUTS, workspace=P_, stream=None),
    "cnerf_composite_bwd_closs": dict(NINE, L=CLOSS, **SEEDS, **PATCH, d_raw=P_, stream=None),
    "cnerf_composite_bwd_closs_ssim": dict(NINE, L=CLOSS, **SEEDS, **PATCH, **SSIM_SEEDS, d_raw=P_, stream=None),
    "cnerf_composite_bwd_closs_lpips": dict(NINE, L=CLOSS, **SEEDS, **PATCH, **SSIM_SEEDS, lpips_dx=P_, n_lpips=512, d_raw=P_, stream=None),
    "cnerf_composite_bwd_lossform": dict(NINE, L=CLOSS, F=FORM, **SEEDS, coef=0.2, **PATCH, **SSIM_SEEDS, d_temp2=P_, g_temp2=P_, d_raw=P_,
                                         stream=None),
    "cnerf_closs_finish": dict(t=TAIL, terms=P_, stats=P_, patch_d=P_, stream=None),
    "cnerf_closs_finish_ss": dict(t=_tail(P=0), coins4=("coins", (1, 0, 1, 0)), terms=P_, stats=P_, stream=None),
    "cnerf_closs_finish_ss2": dict(t=_tail(P=0), coins4=("coins", (1, 0, 1, 0)), seg_row=256, counts3=P_, terms=P_, stats=P_, stream=None),
    "cnerf_closs_finish_ssim": dict(t=TAIL, **SSIM_TAIL, terms=P_, stats=P_, patch_d=P_, ssim_d=P_, stream=None),
    "cnerf_closs_finish_lpips": dict(t=TAIL, **SSIM_TAIL, lpips_P=2, lpips_w=0.25, lpips_v=P_, terms=P_, stats=P_, patch_d=P_, ssim_d=P_,
                                     stream=None),
    "cnerf_lossform_finish": dict(t=TAIL, F_last=FORM, F_coarse=FORM, **SSIM_TAIL, terms=P_, stats=P_, patch_d=P_, ssim_d=P_, d_temp4=P_,
                                  stream=None),
}
# the order in which dict(NINE, ...) etc. list the arguments IS the C order of each entry point (checked against SIGNATURES' lengths
# in run()); cnerf_composite_bwd_lossform takes coef right after the three weights, which is where dict() puts it above.


def null_variants(base):
    """{"valid": {}} and one variant per pointer of the call, struct fields included, with that pointer null."""
    v = {"valid": {}}
    for k, x in base.items():
        if x == P_ or (isinstance(x, tuple)):
            v[f"null.{k}"] = {k: None}
        if isinstance(x, tuple) and x[0] != "coins":
            for fk, fx in x[1].items():
                if fx == P_:
                    v[f"null.{k}.{fk}"] = {f"{k}.{fk}": None}
    return v


def _variants(entry, base):
    """{case suffix: {path: value}} for one entry point: every pointer (struct fields included) nulled in turn, then the edges."""
    v = null_variants(base)
    fin = "t" in base
    bname = "t.B" if fin else "B"
    v["B.neg"], v["B.zero"] = {bname: -1}, {bname: 0}
    if not fin:
        v["S.zero"], v["S.1025"], v["raw_ch.3"], v["ray_stride.5"] = {"S": 0}, {"S": 1025}, {"raw_ch": 3}, {"ray_stride": 5}
        v["B.zero+S.1025"] = {"B": 0, "S": 1025}
        v["null.raw+S.1025"] = {"raw": None, "S": 1025}
    if "workspace" in base:
        v["workspace.misaligned"] = {"workspace": Q_}
        v["workspace.misaligned+S.1025"] = {"workspace": Q_, "S": 1025}
    if entry == "cnerf_composite_fwd_mse":
        v["B.over_mse_limit"] = {"B": "MAX+1"}
        v["B.at_mse_limit"] = {"B": "MAX"}
        v["null.target+B.over_mse_limit"] = {"target": None, "B": "MAX+1"}
        v["B.over_mse_limit+S.1025"] = {"B": "MAX+1", "S": 1025}
    if entry == "cnerf_composite_bwd_mse":
        v["B.over_mse_limit"] = {"B": "MAX+1"}
    if "L" in base:
        v["far.zero"], v["far.zero.no_prior"] = {"L.far": 0.0}, {"L.far": 0.0, "L.prior": None}
        v["null.L+S.1025"] = {"L": None, "S": 1025}
        v["seg_row.8"], v["seg_row.4"], v["seg_row.B"] = {"L.seg_row": 8}, {"L.seg_row": 4}, {"L.seg_row": B}
        v["B.over_mse_limit"] = {"B": "MAX+1"}
    if "F" in base:
        for i, (rf, df) in enumerate(((3, 0), (-1, 0), (0, 6), (0, -1))):
            v[f"form.range{i}"] = {"F.rgb_form": rf, "F.depth_form": df}
        v["form.depth_range.no_prior"] = {"F.depth_form": 6, "L.prior": None}
        v["softmask.no_temp_rgb"] = {"F.temp_rgb": None}
        v["softmask.no_temp_depth"] = {"F.temp_depth": None}
        v["softmask.no_temp_depth.no_prior"] = {"F.temp_depth": None, "L.prior": None}
        v["softlp.no_coef"] = {"F.rgb_form": 1, "F.depth_form": 4, "F.lp_coef": 0.0}
        v["softlp.depth_only.no_coef"] = {"F.rgb_form": 0, "F.depth_form": 4, "F.lp_coef": 0.0}
        v["softlp.depth_only.no_coef.no_prior"] = {"F.rgb_form": 0, "F.depth_form": 4, "F.lp_coef": 0.0, "L.prior": None}
        v["form.range0+S.1025"] = {"F.rgb_form": 3, "S": 1025}
    if "n_patch" in base:
        v["n_patch.neg"], v["n_patch.over_B"], v["n_patch.zero"] = {"n_patch": -1}, {"n_patch": B + 1}, {"n_patch": 0}
        v["n_patch.over_B+S.1025"] = {"n_patch": B + 1, "S": 1025}
    if "n_ssim" in base:
        v["n_ssim.neg"], v["n_ssim.over_B"], v["n_ssim.zero"] = {"n_ssim": -1}, {"n_ssim": B + 1}, {"n_ssim": 0}
        v["n_ssim.zero.null"] = {"n_ssim": 0, "ssim_d": None}
    if "n_lpips" in base:
        v["n_lpips.neg"], v["n_lpips.over_B"], v["n_lpips.zero"] = {"n_lpips": -1}, {"n_lpips": 768}, {"n_lpips": 0}
        v["n_lpips.not_256"], v["n_lpips.one_patch"] = {"n_lpips": 264}, {"n_lpips": 256}
    if "d_temp2" in base:
        v["temps.neither"] = {"d_temp2": None, "g_temp2": None}
    if fin:
        v["ws_last.misaligned"], v["ws_coarse.misaligned"] = {"t.ws_last": Q_}, {"t.ws_coarse": Q_}
        v["far.zero"], v["far.zero.no_depth"] = {"t.far": 0.0}, {"t.far": 0.0, "t.has_depth": 0}
        v["P.9"], v["P.neg"], v["P.zero"] = {"t.P": 9}, {"t.P": -1}, {"t.P": 0, "t.mono": None, "t.depth_last": None, "t.depth_coarse": None}
        v["P.1"], v["P.3.over_B"], v["n.zero"] = {"t.P": 1}, {"t.P": 3}, {"t.n": 0}
        v["one_level"] = {"t.ws_coarse": None, "t.depth_coarse": None, "rgb_coarse": None, "F_coarse": None}
        v["counts"] = {"t.counts": P_}
        if "ssim_P" in base:
            v["ssim_P.zero"], v["ssim_P.9"], v["ssim_P.neg"], v["ssim_P.3.over_B"] = {"ssim_P": 0}, {"ssim_P": 9}, {"ssim_P": -1}, {"ssim_P": 3}
            v["ssim_P.zero.null"] = {"ssim_P": 0, "rgb_last": None, "rgb_coarse": None, "target": None, "ssim_d": None}
        if "lpips_P" in base:
            v["lpips_P.zero"], v["lpips_P.9"], v["lpips_P.neg"], v["lpips_P.3.over_B"] = ({"lpips_P": 0}, {"lpips_P": 9}, {"lpips_P": -1},
                                                                                          {"lpips_P": 3})
        if "seg_row" in base:
            v["seg_row.zero"], v["seg_row.neg"], v["seg_row.4"], v["seg_row.B"] = {"seg_row": 0}, {"seg_row": -8}, {"seg_row": 260}, {"seg_row": B}
            v["seg_row.last"] = {"seg_row": B - 8}
        if "F_last" in base:
            for i, (rf, df) in enumerate(((3, 0), (-1, 0), (0, 6), (0, -1))):
                v[f"form.range{i}"] = {"F_last.rgb_form": rf, "F_last.depth_form": df}
                v[f"form.coarse.range{i}"] = {"F_coarse.rgb_form": rf, "F_coarse.depth_form": df}
            v["form.depth_range.no_depth"] = {"F_last.depth_form": 6, "t.has_depth": 0}
            v["softmask.no_temp_rgb"], v["softmask.no_temp_depth"] = {"F_last.temp_rgb": None}, {"F_coarse.temp_depth": None}
            v["softlp.no_coef"] = {"F_last.rgb_form": 1, "F_last.depth_form": 4, "F_last.lp_coef": 0.0}
            v["soft.counts"] = {"t.counts": P_}
            v["hard.counts"] = {"t.counts": P_, "F_last.rgb_form": 0, "F_last.depth_form": 2, "F_coarse.rgb_form": 0, "F_coarse.depth_form": 1}
            v["soft_depth.counts.no_depth"] = {"t.counts": P_, "t.has_depth": 0, "F_last.rgb_form": 0, "F_coarse.rgb_form": 0}
    return v


def cases():
    out = []
    for entry, base in BASE.items():
        for suffix, change in _variants(entry, base).items():
            if any(k.split(".")[0] not in base for k in change):      # (one_level names arguments only some tails have)
                change = {k: x for k, x in change.items() if k.split(".")[0] in base}
            out.append((f"{entry}:{suffix}", entry, base, change))
    return out


def _materialise(L, base, change, ptr, max_rays, keep):
    call = copy.deepcopy(base)
    for path, x in change.items():
        k, _, fk = path.partition(".")
        if fk:
            call[k][1][fk] = x
        else:
            call[k] = x
    sym = {P_: ptr, Q_: ptr + 4, "MAX": max_rays, "MAX+1": max_rays + 1}
    val = lambda x: sym.get(x, x) if isinstance(x, str) else x  # noqa: E731
    args = []
    for x in call.values():
        if isinstance(x, tuple) and x[0] == "coins":
            x = (C.c_int32 * 4)(*x[1])
        elif isinstance(x, tuple):
            x = getattr(L, x[0])(**{fk: val(fx) for fk, fx in x[1].items()})
            keep.append(x)
            x = C.byref(x)
        args.append(val(x))
    return args


def run(lib_path=None, M=None):
    """{case name: return code} of every case of the cases module M (None: this one; tests/_fwd_rule_cases.py is the other) against the
    library at lib_path (None: the package's own).  Raises where a device is visible.  A change named "$VARIABLE" is no argument: that
    environment variable holds the value during the call."""
    M = M or sys.modules[__name__]
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from consistentnerf_amd import _lib as L
    lib = C.CDLL(lib_path or L.LIB_PATH)
    for n in list(M.BASE) + ["cnerf_device_info", "cnerf_composite_mse_max_rays"]:
        f = getattr(lib, n)
        f.restype, f.argtypes = L.SIGNATURES[n]
    name, cus, mem = C.create_string_buffer(256), C.c_int(0), C.c_int(0)
    if lib.cnerf_device_info(0, name, C.byref(cus), C.byref(mem)) == 0 or name.value:      # (a name: a device of another kind answered)
        raise RuntimeError(f"a device is visible ({name.value.decode(errors='replace')}): the cases pass host pointers and must not run here")
    buf = (C.c_double * 4096)()
    ptr = C.cast(buf, C.c_void_p).value
    assert ptr % 8 == 0
    max_rays = lib.cnerf_composite_mse_max_rays()
    out, keep = {}, []
    for cname, entry, base, change in M.cases():
        env = {k[1:]: x for k, x in change.items() if k.startswith("$")}
        args = _materialise(L, base, {k: x for k, x in change.items() if not k.startswith("$")}, ptr, max_rays, keep)
        assert len(args) == len(L.SIGNATURES[entry][1]), (entry, len(args))
        assert cname not in out, cname
        os.environ.update(env)
        try:
            out[cname] = int(getattr(lib, entry)(*args))
        finally:
            for k in env:
                del os.environ[k]
    return out
