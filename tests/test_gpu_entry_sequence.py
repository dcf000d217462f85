"""The C entry points a training step calls, in order, against lists recorded on the commit BEFORE the host path between the
callers and the C ABI was rewritten (tests/golden/entry_sequences.json, written by `scripts/step_fingerprint.py --sequences`, never
by the code under test): a change of run_nerf.py, run_nerf_view.py or ops.py that is meant to keep the routes must keep these."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    spec = importlib.util.spec_from_file_location("step_fingerprint", os.path.join(ROOT, "scripts", "step_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    sc = fp.scene(torch.device("cuda:0"))
    with open(os.path.join(ROOT, "tests", "golden", "entry_sequences.json")) as f:
        return fp, sc, fp.routes(sc), json.load(f)


def test_the_recorded_routes_are_the_ones_replayed(rig):
    fp, _, table, want = rig
    assert set(want) == set(fp.SEQUENCE_ROUTES) <= set(table)


@pytest.mark.parametrize("route", ["render_loss.two_levels", "view.ssim_lpips", "view.softmask", "ss.one_render.1100"])
def test_entry_point_sequence(rig, route):
    """run_nerf.render_loss on two levels; run_nerf_view.render_loss with mask, prior, mono, SSIM and LPIPS; the softmask loss forms;
    the one-render in-loop consistency step with both coarse coins 0 — each with its backward."""
    fp, sc, table, want = rig
    got = fp.run_route(sc, table[route])["entries"]
    print(f"{route}: {len(got)} entry points: {' '.join(got)}")
    assert len(want[route]) > 5
    assert got == want[route]
