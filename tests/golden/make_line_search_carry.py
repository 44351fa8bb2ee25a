"""Records tests/golden/line_search_carry.json: what the library computes for the cases of tests/line_search_carry_cases.py.

Run on a GPU against the library of the commit BEFORE the change that took the lumas out of the rounds of the 32-lane
line search (VM_LIB_PATH names that build), never against the code under test: tests/test_gpu_line_search_carry.py
holds later builds to these bits.

    VM_LIB_PATH=<parent build>/libvmorph_hip.so python3 tests/golden/make_line_search_carry.py <out.json> <commit>

Layout: one line per case.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import line_search_carry_cases as CC  # noqa: E402
from videomorphing_amd import capi, morph  # noqa: E402


def main():
    out_path = sys.argv[1]
    ctx = morph.Context(0, capi.MATH_FAST)
    cases = {}
    for key, kind, w, h, name, sweeps in CC.cases():
        r = CC.run_case(ctx, kind, w, h, name, sweeps)
        r["reached"] = CC.reached(name, r)
        print(key, "reached" if r["reached"] else "NOT REACHED", "temp_mask max %g" % r["temp_mask_max"],
              [(p["sha256"]["luma"][:12], p["iters"], p["counters"], p["sched_launches"]) for p in r["pages"]], flush=True)
        cases[key] = r
    head = {"made_by": "tests/golden/make_line_search_carry.py", "library": "parent commit " + (sys.argv[2] if len(sys.argv) > 2 else "?"),
            "arithmetic": "FAST", "fields": list(CC.FIELDS), "counters": list(CC.COUNTERS), "w_temp": CC.W_TEMP}
    dumps = lambda o: json.dumps(o, sort_keys=True, separators=(",", ":"))
    with open(out_path, "w") as f:
        f.write("{\n")
        for k in sorted(head):
            f.write(" %s: %s,\n" % (json.dumps(k), dumps(head[k])))
        f.write(' "cases": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), dumps(cases[k])) for k in sorted(cases)) + "\n }\n}\n")
    json.load(open(out_path))


if __name__ == "__main__":
    main()
