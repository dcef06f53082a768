#!/usr/bin/env python3
"""A/B of the tile bitmap's triangle stage (csrc/rpt_tile_bitmap.hpp) against the parent revision.

Sides: `parent` = a built checkout of the parent revision (its own bench.py, package and libraries); `commit` = this tree as built.
Never this tree with RPT_TILE_TRIANGLES=0 in the parent's place: the gate compares revisions.

    python3 tools/tile_triangles_ab.py run --parent-tree DIR [--pairs 3] [--lines headline,bunny1080,bunny8k,shadows4k] [--full]
    python3 tools/tile_triangles_ab.py counters --parent-tree DIR [--sets "SQ_WAVES SQ_INSTS_VALU" "SQ_INSTS_VMEM_RD ..."]

`run` alternates the sides, parent first, `--pairs` times, in ONE job, on every line of --lines (bench.py --gpus 1 --steps 50 --warmup 5
plus the line's own arguments), then with --full alternates `bench.py --full --check` the same way (one frame at a time, the animated
figure, the check against the oracle).  Every bench.py run sits under its own `timeout`, the runs are chained, and the tool stops at
the first non-zero status.  It prints one row per run and, per line and side, the range of `value`; the gate is met on a line when all
of the commit's values lie above all of the parent's.

`counters` runs each side's headline once per counter set under rocprofv3 — `--kernel-trace --pmc <set>` and nothing else, one set per
run, never together with another trace — and prints the per-launch means of the frame kernel."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = {
    "headline": [],
    "bunny1080": ["--width", "1920", "--height", "1080"],
    "bunny8k": ["--width", "7680", "--height", "4320"],
    "shadows4k": ["--workload", "shadows"],
}
BASE = ["--gpus", "1", "--steps", "50", "--warmup", "5"]
SETS = ["SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_SMEM", "TA_FLAT_READ_WAVEFRONTS_sum", "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY"]


def run(cmd, tree, limit):
    """One command under its own `timeout`; the tool ends at the first non-zero status (nothing more is started on the device)."""
    env = dict(os.environ)
    env.pop("RPT_HIP_LIB", None)
    env.pop("RPT_TILE_TRIANGLES", None)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"stopped: {' '.join(cmd)} in {tree} ended with status {p.returncode}\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
    return p.stdout


def bench(tree, bench_args, limit):
    out = run([sys.executable, os.path.join(tree, "bench.py")] + bench_args, tree, limit)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def counters(sides, sets, limit):
    for pmc in sets:
        for name, tree in sides:
            with tempfile.TemporaryDirectory() as d:
                run(["rocprofv3", "--kernel-trace", "--pmc", *pmc.split(), "--output-format", "csv", "-d", d, "-o", "pmc", "--",
                     sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], tree, limit)
                sums, launches = {}, {}
                for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        key = (row["Kernel_Name"].split("(")[0][:60], row["Counter_Name"])
                        sums[key] = sums.get(key, 0.0) + float(row["Counter_Value"])
                        launches[key] = launches.get(key, 0) + 1
                # (one row per dispatch, counter and — for some counters — dimension: the dispatch count comes from the smallest row count)
                per_kernel = {}
                for (k, c), v in sums.items():
                    per_kernel.setdefault(k, {})[c] = (v, launches[(k, c)])
                for k, cs in sorted(per_kernel.items(), key=lambda kv: -max(v for v, _ in kv[1].values()))[:2]:
                    n = min(n for _, n in cs.values())
                    print(f"{name:7s} {k}: {n} launches; per launch " + ", ".join(f"{c} {v / n:.0f}" for c, (v, _) in sorted(cs.items())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["run", "counters"])
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--lines", default=",".join(LINES))
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--sets", nargs="+", default=SETS)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each bench.py run (twice that with --full and under the profiler)")
    args = ap.parse_args()
    sides = [("parent", os.path.abspath(args.parent_tree)), ("commit", ROOT)]
    if args.command == "counters":
        return counters(sides, args.sets, 2 * args.timeout)
    lines = [ln for ln in args.lines.split(",") if ln]
    values = {(ln, s): [] for ln in lines for s, _ in sides}
    for ln in lines:
        for k in range(args.pairs):
            for s, tree in sides:
                d = bench(tree, BASE + LINES[ln], args.timeout)
                values[(ln, s)].append(d["value"])
                print(f"{ln:10s} pair {k} {s:7s} value {d['value']}  ms_per_step {d['ms_per_step']:.5f}  kernel_ms {d.get('kernel_ms')}", flush=True)
        pa, co = values[(ln, "parent")], values[(ln, "commit")]
        print(f"{ln:10s} parent [{min(pa)}, {max(pa)}]  commit [{min(co)}, {max(co)}]  commit / parent (medians) "
              f"{sorted(co)[len(co) // 2] / sorted(pa)[len(pa) // 2]:.4f}  all of the commit's above all of the parent's: {min(co) > max(pa)}\n", flush=True)
    if args.full:
        for k in range(args.pairs):
            for s, tree in sides:
                d = bench(tree, BASE + ["--full", "--check", "--no-cpu-baseline"], 2 * args.timeout)
                one = d.get("one_frame_at_a_time") or {}
                print(f"full pair {k} {s:7s} value {d['value']}  one frame at a time {one.get('ms_per_frame')} ms (kernel {one.get('kernel_ms')})  "
                      f"animated {(d.get('animated') or {}).get('ms_per_step')} ms  check: {d.get('check')}", flush=True)


if __name__ == "__main__":
    main()
