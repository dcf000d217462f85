#!/usr/bin/env python3
"""Golden-vector generator for inverse-CDF resampling across CDF lengths. Runs ONLY in the build container (needs the reference
checkout), in the manner of make_golden.py: the reference's own run_nerf_helpers.sample_pdf (H:206-250) is called on the seeded
inputs of _inputs.py (resample_envelope_inputs: 13 rows per shape, an all-zero row, a row with a flat CDF run) for the 19
(Nc, Nf) pairs of _inputs.RESAMPLE_SHAPES and both of its pytest streams (det: linspace incl. the u = 1 tie; rand), with the
`torch.searchsorted` inside it (H:233) intercepted for the indices.  Only *outputs* are written, arrays only, to
sample_pdf_lengths.npz next to this file: `<Nc>_<Nf>_<stream>_inds` (int16) and `<Nc>_<Nf>_<stream>_samples` (fp32).  The inputs
are regenerated from _inputs.py by the tests.  No reference source, bytecode or pickled object is written.

A fixture rather than the oracle at test time: the index at a CDF tie is decided by one fp32 ulp of torch.sum (the pdf normaliser),
which must not depend on the CPU of the machine that runs the GPU tests.

usage:  python tests/golden/make_golden_sample_lengths.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import _inputs as I  # noqa: E402
from make_golden_lossforms import REF  # noqa: E402  (where the reference checkout lives)

torch.set_num_threads(8)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    sys.path.insert(0, REF)
    import run_nerf_helpers as H   # (imports torch / numpy only)
    real = torch.searchsorted
    cap = {}

    def spy(cdf, u, right=False, **kw):
        inds = real(cdf, u, right=right, **kw)
        cap.update(cdf=cdf.clone(), u=u.clone(), inds=inds.clone(), right=right)
        return inds

    out = {}
    B = 13
    for Nc, Nf in I.RESAMPLE_SHAPES:
        z, w = I.resample_envelope_inputs(Nc, B)
        bins = 0.5 * (T(z)[:, 1:] + T(z)[:, :-1])            # R:394
        for tag in ("det", "rand"):
            torch.searchsorted = spy
            try:
                samples = H.sample_pdf(bins, T(w)[:, 1:-1], Nf, det=(tag == "det"), pytest=True)   # R:395
            finally:
                torch.searchsorted = real
            assert cap["right"] is True and cap["cdf"].shape == (B, Nc - 1) and samples.shape == (B, Nf)
            assert np.array_equal(cap["u"].numpy(), I.resample_envelope_u(tag, B, Nf)), "the tests rebuild u from _inputs.py"
            inds = cap["inds"].numpy()
            assert inds.min() >= 0 and inds.max() <= Nc - 1
            margin = (cap["u"][..., None].double() - cap["cdf"][:, None, :].double()).abs().min(-1).values
            out[f"{Nc}_{Nf}_{tag}_inds"] = inds.astype(np.int16)
            out[f"{Nc}_{Nf}_{tag}_samples"] = samples.numpy().astype(np.float32)
            print(f"  Nc {Nc:3d} Nf {Nf:3d} {tag:4s}: {int((margin <= 1e-5).sum()):5d} of {margin.numel():5d} samples within 1e-5 of a "
                  f"CDF entry, {int((inds == Nc - 1).sum())} past the last entry")
    path = os.path.join(HERE, "sample_pdf_lengths.npz")
    np.savez_compressed(path, **out)
    print(f"wrote sample_pdf_lengths.npz ({os.path.getsize(path) / 1024:.1f} KiB), {len(out)} arrays")


if __name__ == "__main__":
    main()
