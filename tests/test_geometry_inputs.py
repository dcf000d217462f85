"""The inputs of tests/test_gpu_geometry_envelope.py are decidable by the reference alone (CPU only).

The hard-mask scenes are conditioned (_inputs.condition_hard_mask_inputs) so that no pixel sits on a rounding tie, on the image
border or on a rung of a threshold ladder; on every case the GPU tests run, oracle.hard_masks (fp32, pinned on the reference's own
fixture by test_oracle_golden.test_hard_masks) and the float64 restatement (_inputs.hard_masks_f64) must then give identical
masks, identical per-chunk thresholds as fp32 values and identical NaN entries.  The same for the warp: on the rows the float64
restatement calls decided, oracle.warp_points rounds like it, and at most 2 % of the rows are dropped.  The encoding yardstick: the
reference's fp32 encoding stays within one fp32 unit round-off of float64 at every scale the GPU test uses."""
import numpy as np
import pytest
import torch

import _inputs as I
from oracle import nerf_oracle as O

torch.set_num_threads(4)

NUDGE_CAP, ITER_CAP, DROP_CAP = 0.02, 8, 0.02


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _w2c(pose):
    c2w = torch.eye(4)
    c2w[:3, :4] = T(pose[:3, :4])
    return torch.inverse(c2w).numpy()          # the 4x4 fp32 host inverse, as V:1008-1010


@pytest.mark.parametrize("scene", range(len(I.GEOMETRY_SCENES)))
def test_conditioning_within_caps(scene):
    c = I.geometry_case(scene)
    print(f"  {c['H']}x{c['W']}: {c['info']}")
    assert c["info"]["iterations"] <= ITER_CAP and max(c["info"]["nudged_share"]) <= NUDGE_CAP
    assert c["info"]["nudged_share"][3] == 0.0, "the held-out view is no target"
    moved = c["depths"] != c["raw_depths"]
    assert 0 < moved.mean() <= NUDGE_CAP and np.all(c["depths"][moved] > c["raw_depths"][moved])
    K = c["K"]
    assert K[0, 0] != K[1, 1] and (K[0, 2] - 0.5 * c["W"]) % 1 != 0 and (K[1, 2] - 0.5 * c["H"]) % 1 != 0
    # conditioned means: nothing left to nudge, for any pair and ladder
    again, info = I.condition_hard_mask_inputs(c["H"], c["W"], K, c["poses"], c["depths"])
    assert info["iterations"] == 0 and np.array_equal(again, c["depths"])


def test_conditioning_fails_loudly():
    H, W, focal = I.GEOMETRY_SCENES[0]
    K, poses, depths = I.geometry_scene(H, W, focal)
    with pytest.raises(AssertionError, match="fixed point"):
        I.condition_hard_mask_inputs(H, W, K, poses, depths, max_iter=0)
    with pytest.raises(AssertionError, match="cap"):
        I.condition_hard_mask_inputs(H, W, K, poses, depths, max_share=1e-4)


@pytest.mark.parametrize("scene,i_train,chunk,thr0", I.hard_mask_cases())
def test_oracle_equals_float64_restatement(scene, i_train, chunk, thr0):
    c = I.geometry_case(scene)
    H, W = c["H"], c["W"]
    masks, log = O.hard_masks(H, W, c["K"], c["poses"], c["depths"], list(i_train), float(np.float32(thr0)), chunk)
    m64, thr64, deepest = I.hard_masks_f64(H, W, c["K"], c["poses"], c["depths"], i_train, thr0, chunk)
    assert np.array_equal(masks, m64), f"{int((masks != m64).sum())} mask bits differ"
    assert not masks[3].any() and masks[list(i_train)].any()
    nchunks = (H * W + chunk - 1) // chunk
    assert log.shape[0] == len(i_train) * (len(i_train) - 1) * nchunks
    n_nan = 0
    for t, r, ch, th in log:
        want = thr64[(int(t), int(r))][int(ch)]
        n_nan += int(np.isnan(th))
        assert (np.isnan(th) and np.isnan(want)) or np.float32(th) == want, (t, r, ch, th, want)
    print(f"  {H}x{W} chunk={chunk} thr0={thr0:g}: deepest level {deepest}, {n_nan} of {log.shape[0]} chunks without an in-bounds pixel")
    # the cases do what they are meant to
    if thr0 == I.GEOMETRY_THR0[2]:
        assert deepest == 0
    if thr0 == I.GEOMETRY_THR0[3]:
        assert 64 < deepest < I.KMAX
    if thr0 == 0.1 and chunk <= 257:
        assert deepest >= 2, "the biased prior must force more than one doubling"
    if chunk <= 7:
        assert n_nan > 0.1 * log.shape[0], "small chunks must leave many chunks without an in-bounds pixel"


def test_ladder_is_the_fp32_doubling():
    """The kernel doubles in fp32, the oracle doubles a Python float that ATen casts to fp32 for the comparison: the same values,
    +inf included (from k = 128 - log2(thr0) on)."""
    for thr0 in I.GEOMETRY_THR0:
        r = I.ladder(thr0)
        with np.errstate(over="ignore"):
            want = [float(np.float32(float(np.float32(thr0)) * 2.0 ** k)) for k in range(I.KMAX + 1)]
        assert r.tolist() == want and np.isinf(r[-1]) and np.isfinite(r[64])
    r = I.ladder(0.1)
    lv = I.ladder_level(np.array([0.0, 0.05, r[0], 0.15, r[1], 0.3, r[I.KMAX - 200], np.inf, np.nan]), 0.1)
    assert lv.tolist() == [0, 0, 1, 1, 2, 2, I.KMAX - 199, I.NO_LEVEL, I.NO_LEVEL]


@pytest.mark.parametrize("flip", [True, False])
def test_warp_points_decided_rows(flip):
    """oracle.warp_points == the float64 restatement on the decided rows of the GPU test's points; <= 2 % are dropped."""
    c = I.geometry_case(2)
    H, W, K = c["H"], c["W"], c["K"]
    P, pose = I.warp_envelope_points(c)
    w2c = _w2c(pose)
    assert P.shape == (I.WARP_N[-1], 3)
    p, keep = I.warp_decided_rows(P, w2c, K, H, W, flip)
    dropped = 1.0 - keep.mean()
    print(f"  flip={flip}: dropped {dropped:.3%} of {P.shape[0]} rows; in bounds {p['inb'].mean():.1%}; behind the camera and in bounds "
          f"{int((p['inb'] & (p['Xc'][:, 2] < 0)).sum())}")
    assert dropped <= DROP_CAP
    for n in I.WARP_N[1:-1]:
        assert 1.0 - keep[:n].mean() <= max(DROP_CAP, 1.0 / n)
    assert p["inb"][keep].mean() > 0.1 and (~p["inb"][keep]).mean() > 0.1
    Xc, x, y, inb = O.warp_points(T(P), T(w2c), T(K), H, W, flip)
    assert np.array_equal(x.numpy()[keep], p["x"][keep]) and np.array_equal(y.numpy()[keep], p["y"][keep])
    assert np.array_equal(inb.numpy()[keep], p["inb"][keep])
    bound = 4 * I.U32 * p["S"]
    ratio = np.abs(Xc.numpy().astype(np.float64) - p["Xc"]) / bound
    print(f"  oracle Xc: largest error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("L", [10, 4, 1])
def test_reference_encoding_error_is_the_yardstick(L):
    for scale in I.EMBED_SCALES:
        x = I.embed_envelope_inputs(scale, L)
        err = np.abs(O.embed(T(x), L).numpy().astype(np.float64) - I.embed_f64(x, L)).max()
        print(f"  L={L} scale={scale:g}: fp32 oracle max error {err:.2e}")
        assert err <= I.U32, "the reference's fp32 encoding is within one unit round-off of float64 at every scale"
