"""Writes tests/golden/closs_arg_rules.json: {case name: return code} of every case of tests/_closs_rule_cases.py against a GIVEN
build of the library —

    HIP_VISIBLE_DEVICES=-1 python tests/golden/make_golden_closs_rules.py LIB.so OUT.json

The committed file was written from a build of the commit before the folded loss's host path was rewritten ("Add the test-set pass
on the device", aa77ec3), which is what makes tests/test_closs_host_rules.py a comparison with the old rules and not with
themselves.  Regenerate it only from a library whose rules are the ones to keep; code under test never writes it."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _closs_rule_cases as cases  # noqa: E402

if __name__ == "__main__":
    lib_path, out_path = sys.argv[1:3]
    if os.environ.get("HIP_VISIBLE_DEVICES") != "-1":
        sys.exit("run with HIP_VISIBLE_DEVICES=-1: the cases pass host pointers")
    seen = cases.run(os.path.abspath(lib_path))
    with open(out_path, "w") as f:
        json.dump(seen, f, indent=0, sort_keys=True)
        f.write("\n")
    codes = sorted(set(seen.values()))
    print(f"{len(seen)} cases -> {out_path}; codes {({c: sum(v == c for v in seen.values()) for c in codes})}")
