#!/bin/bash
# rehearsal: `python bench.py --gpus 2` BARE over gloo (both ranks on this box's one GPU) with the full-size config 5 block (7680x4320)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export RESULTS="${RESULTS:-bench_outputs}"; mkdir -p "$RESULTS"   # where this script writes its results (relative: to the repository root)
mkdir -p $RESULTS/r04
RPT_BENCH_BACKEND=gloo timeout -k 10 600 python bench.py --gpus 2 --steps 20 --warmup 5 --full --no-cpu-baseline > $RESULTS/r04/bench_gloo2_config5.json 2> $RESULTS/r04/bench_gloo2_config5.err
echo rc=$?
python - <<'PY'
import json, os
d = json.loads([l for l in open(os.environ["RESULTS"] + "/r04/bench_gloo2_config5.json") if l.startswith("{")][-1])
print(d["value"], d["ms_per_step"], d["config"]["sharding"])
print(json.dumps(d["comm"]["config5"], indent=1))
print(d["comm"]["split_timings_ms_per_frame"])
PY
tail -3 $RESULTS/r04/bench_gloo2_config5.err
