# the default bench command with roofline.valu in the line (library of record: the PMC summaries' hash must match)
cd "$GRAFT_REPO_ROOT"
export RESULTS="${RESULTS:-bench_outputs}"; mkdir -p "$RESULTS"   # where this script writes its results (relative: to the repository root)
mkdir -p $RESULTS/r04
timeout -k 10 600 python bench.py --full > $RESULTS/r04/bench_valu_default.json 2> $RESULTS/r04/bench_valu_default.err; rc=$?
python - <<'PY'
import json, os
d = json.loads(open(os.environ["RESULTS"] + "/r04/bench_valu_default.json").read().strip().splitlines()[-1])
r = d["roofline"]
print(d["value"], d["ms_per_step"], r["frac"], r["traffic"])
print("alone    ", r.get("valu"))
print("in flight", r["device_in_flight"].get("valu"))
PY
exit $rc
