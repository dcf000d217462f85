"""The argument rules of the folded step loss's C entry points are the ones they had before their host path was rewritten: every
case of tests/_closs_rule_cases.py (one passing call per entry point, each pointer nulled in turn, each size at its edges, a few
double faults that pin which code wins) returns what tests/golden/closs_arg_rules.json recorded from the earlier library.

The cases run in a child process that cannot see a device (HIP_VISIBLE_DEVICES=-1), so that the calls which pass validation end
at the launch with hipErrorNoDevice instead of handing the dummy host pointers to a kernel; the child checks that first and stops
before the first case if a device answers."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _closs_rule_cases as cases  # noqa: E402

with open(os.path.join(HERE, "golden", "closs_arg_rules.json")) as _f:
    WANT = json.load(_f)


def seen():
    """The child's {case: return code}."""
    code = "import json, sys; sys.path.insert(0, %r); import _closs_rule_cases as M; print(json.dumps(M.run()))" % HERE
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-1200:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_cases_and_fixture_name_the_same_calls():
    names = [c[0] for c in cases.cases()]
    assert sorted(names) == sorted(WANT) and len(set(names)) == len(names)
    # every entry point has a call that got past validation (to the launch: no device there), and rules that refuse
    for entry in cases.BASE:
        assert WANT[f"{entry}:valid"] == 100, entry
        assert any(v == -1 for k, v in WANT.items() if k.startswith(entry + ":")), entry


def test_return_codes_equal_the_earlier_library():
    got = seen()
    assert sorted(got) == sorted(WANT)
    wrong = {k: (got[k], WANT[k]) for k in WANT if got[k] != WANT[k]}      # case: (now, before)
    assert not wrong, wrong
