"""Writes tests/golden/closs_arg_rules.json: {case name: return code} of every case of tests/_closs_rule_cases.py against a GIVEN
build of the library —

    HIP_VISIBLE_DEVICES=-1 python tests/golden/make_golden_closs_rules.py LIB.so OUT.json [CASES_MODULE]

CASES_MODULE names another cases module under tests/ (default _closs_rule_cases).  tests/golden/fwd_arg_rules.json, the forward's
rules (_fwd_rule_cases, tests/test_fwd_host_rules.py), was written this way from a build of the commit before the forward's host
path was rewritten ("Test the bf16x3 training kernels against float64 in the default run", 4a01b5f).

closs_arg_rules.json was written from a build of the commit before the folded loss's host path was rewritten ("Add the test-set pass
on the device", aa77ec3), which is what makes tests/test_closs_host_rules.py a comparison with the old rules and not with
themselves.  Regenerate it only from a library whose rules are the ones to keep; code under test never writes it."""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _closs_rule_cases as cases  # noqa: E402

if __name__ == "__main__":
    lib_path, out_path = sys.argv[1:3]
    M = importlib.import_module(sys.argv[3]) if len(sys.argv) > 3 else cases
    if os.environ.get("HIP_VISIBLE_DEVICES") != "-1":
        sys.exit("run with HIP_VISIBLE_DEVICES=-1: the cases pass host pointers")
    seen = cases.run(os.path.abspath(lib_path), M)
    with open(out_path, "w") as f:
        json.dump(seen, f, indent=0, sort_keys=True)
        f.write("\n")
    codes = sorted(set(seen.values()))
    print(f"{len(seen)} cases -> {out_path}; codes {({c: sum(v == c for v in seen.values()) for c in codes})}")
