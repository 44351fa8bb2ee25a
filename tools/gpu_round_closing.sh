#!/bin/bash
# closing visit: the whole GPU suite, smoke(), the full bench line (timed).  usage (on the box, repo root):
#   bash tools/gpu_round_closing.sh <output dir>
O=${1:?usage: bash tools/gpu_round_closing.sh <output dir>}
mkdir -p "$O"
export TMPDIR=/tmp
timeout 3000 python -m pytest tests -x -q -m gpu > "$O/pytest.log" 2>&1; echo "pytest rc=$?" | tee -a "$O/pytest.log"
tail -4 "$O/pytest.log"
timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1; echo "smoke rc=$?"; tail -1 "$O/smoke.log"
( time timeout 600 python bench.py --full ) > "$O/bench_full.json" 2> "$O/bench_full.err"; echo "bench rc=$?"; tail -4 "$O/bench_full.err"
python - "$O/bench_full.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k: d.get(k) for k in ("value", "ms_per_step", "steps", "warmup", "evals_per_s", "sclk_mhz_observed", "render_frames_per_s")})
print(d["roofline"]["frac"], d["cpu_baseline"]["value"], d["cpu_baseline"]["parity_same_sample"]["bit_identical"])
PY
