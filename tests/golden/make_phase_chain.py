"""Records tests/golden/phase_chain.json: what the library computes for the sweep cases of tests/phase_chain_cases.py.

Run on a GPU against the library of the commit BEFORE a change of the sweep kernels' phase code (VM_LIB_PATH names that
build), never against the code under test: tests/test_gpu_phase_chain.py holds later builds to these bits.

    VM_LIB_PATH=<parent build>/libvmorph_hip.so python3 tests/golden/make_phase_chain.py <out.json> <commit>

Layout: one line per case; the per-sweep counter tables are stored once each (schedules that agree share one).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import line_search_cases as LC  # noqa: E402
import phase_chain_cases as PC  # noqa: E402
from videomorphing_amd import capi, morph  # noqa: E402


def main():
    out_path = sys.argv[1]
    ctx = morph.Context(0, capi.MATH_FAST)
    cases, tables = {}, []
    for k, kind, name, args in PC.cases():
        r = PC.run(ctx, kind, args)
        if kind == "solve":
            r["reached"] = len(r["iters"]) >= 2 and sum(t[2] for t in r["totals"]) > 0
            print(k, r["v_sha256"][:16], r["iters"], r["sched_launches"], flush=True)
        else:
            r["reached"] = r["sched_launches"][LC.SLOT[name]] > 0
            print(k, r["v_sha256"][:16], r["totals"], r["sched_launches"], "reached" if r["reached"] else "NOT REACHED", flush=True)
            per = r.pop("per_sweep")
            if per not in tables:
                tables.append(per)
            r["per_sweep_table"] = tables.index(per)
        cases[k] = r
    head = {"made_by": "tests/golden/make_phase_chain.py", "library": "parent commit " + (sys.argv[2] if len(sys.argv) > 2 else "?"),
            "sweeps": PC.SWEEPS, "arithmetic": "FAST", "counters": list(LC.COUNTERS)}
    dumps = lambda o: json.dumps(o, sort_keys=True, separators=(",", ":"))
    with open(out_path, "w") as f:
        f.write("{\n")
        for k in sorted(head):
            f.write(" %s: %s,\n" % (json.dumps(k), dumps(head[k])))
        f.write(' "cases": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), dumps(cases[k])) for k in sorted(cases)) + "\n },\n")
        f.write(' "per_sweep_tables": [\n' + ",\n".join("  " + dumps(t) for t in tables) + "\n ]\n}\n")
    json.load(open(out_path))


if __name__ == "__main__":
    main()
