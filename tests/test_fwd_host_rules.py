"""The argument rules of the forward's C entry points (the MLP forwards, coarse_z / resample / sample_pdf, render_fwd / render_bwd) are
the ones they had before their host path was rewritten: every case of tests/_fwd_rule_cases.py returns what
tests/golden/fwd_arg_rules.json recorded from the earlier library.  The plane forwards run every case on both kernels of the
CNERF_BF_PERWAVE switch.

As tests/test_closs_host_rules.py: the cases run in a child process that cannot see a device (HIP_VISIBLE_DEVICES=-1), so that a call
which passes validation ends at its first launch instead of handing the dummy host pointers to a kernel; the child checks that first
and stops before the first case if a device answers."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _fwd_rule_cases as cases  # noqa: E402

with open(os.path.join(HERE, "golden", "fwd_arg_rules.json")) as _f:
    WANT = json.load(_f)


def seen():
    """The child's {case: return code}."""
    code = ("import json, sys; sys.path.insert(0, %r); import _closs_rule_cases as R, _fwd_rule_cases as M; "
            "print(json.dumps(R.run(None, M)))" % HERE)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-1200:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_cases_and_fixture_name_the_same_calls():
    names = [c[0] for c in cases.cases()]
    assert sorted(names) == sorted(WANT) and len(set(names)) == len(names)
    # every entry point has a call that got past validation — to the launch (100: no device there), the shared-panel plane forwards to
    # the LDS opt-in in front of it (-3), cnerf_render_ws_floats to its size — and rules that refuse
    for entry in cases.BASE:
        past = WANT[f"{entry}:valid"]
        assert past > 0 if entry == "cnerf_render_ws_floats" else past == (-3 if entry in cases.PLANE_ENTRIES else 100), (entry, past)
        assert any(v == -1 for k, v in WANT.items() if k.startswith(entry + ":")), entry
    for entry in cases.PLANE_ENTRIES:      # the per-wave kernel has no opt-in: its launch is what fails (training has no per-wave form)
        assert WANT[f"{entry}:valid:perwave"] == (100 if entry == "cnerf_mlp_fwd_bf" else -3), entry


def test_return_codes_equal_the_earlier_library():
    got = seen()
    assert sorted(got) == sorted(WANT)
    wrong = {k: (got[k], WANT[k]) for k in WANT if got[k] != WANT[k]}      # case: (now, before)
    assert not wrong, wrong
