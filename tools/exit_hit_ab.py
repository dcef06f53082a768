#!/usr/bin/env python3
"""A/B of the walk's exit records and hit records (csrc/rpt_kernels.hip.h: DExit, DHit) against the parent revision.

Sides: `parent` = a built checkout of the parent revision (its own bench.py, package and libraries); `both` = this tree as built;
and the single parts, builds of this tree's library with one switch off, loaded through RPT_HIP_LIB by this tree's bench.py:
    exits_only   -DRPT_HIT_RECORDS=0             hits_only   -DRPT_EXIT_RECORDS=0
(A third arm, the latency walk of kernels 43 / 49 through exit records too, lost and is gone: profiles/r16_exit_hit_ab.txt.)

    python3 tools/exit_hit_ab.py build [--out DIR]                       (no device needed: compiles the arms into DIR/<arm>/)
    python3 tools/exit_hit_ab.py run --parent-tree DIR [--arms DIR] [--pairs 3] [--lines headline,shadows4k,...] [--full]

`run` alternates the sides, parent first, `--pairs` times, in ONE job, on every line of --lines (bench.py --gpus 1 --steps 50 --warmup 5
plus the line's own arguments), then with --full once per side (--full-runs: more often) `bench.py --full --check` (one frame at a time, kernel 43,
and the check against the oracle).  It prints one row per run and, per line and side, the median and the range of ms_per_step, the ratio to the
parent's median, and whether the side's range lies wholly below the parent's.  A part is adopted only if it does on `headline` while
the mesh-free line (`cubes4k`: kernels that no part changes) stays inside its own spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {
    "exits_only": "-DRPT_HIT_RECORDS=0",
    "hits_only": "-DRPT_EXIT_RECORDS=0",
}
LINES = {
    "headline": [],
    "shadows4k": ["--workload", "shadows"],
    "bunny1080": ["--width", "1920", "--height", "1080"],
    "bunny8k": ["--width", "7680", "--height", "4320"],
    "cubes4k": ["--workload", "cubes"],
}
BASE = ["--gpus", "1", "--steps", "50", "--warmup", "5"]


def build(out):
    csrc = os.path.join(ROOT, "relativitypathtracer_amd", "csrc")
    for arm, flag in ARMS.items():
        d = os.path.abspath(os.path.join(out, arm))
        os.makedirs(d, exist_ok=True)
        subprocess.run(["make", "-C", csrc, f"OUT={d}", f"BUILD={d}/build", f"EXTRA={flag}", f"{d}/librpt_hip.so"], check=True)
        print(f"{arm}: {d}/librpt_hip.so")


def bench(tree, lib, bench_args, timeout):
    env = dict(os.environ)
    env.pop("RPT_HIP_LIB", None)
    if lib:
        env["RPT_HIP_LIB"] = lib
    tree = os.path.abspath(tree)
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + bench_args, capture_output=True, text=True, env=env, timeout=timeout, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"bench.py failed ({tree}, {lib}, rc {p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["build", "run"])
    ap.add_argument("--out", "--arms", dest="arms", default=os.path.join(ROOT, "bench_outputs", "exit_hit_ab"))
    ap.add_argument("--parent-tree")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--lines", default=",".join(LINES))
    ap.add_argument("--sides", default="parent,exits_only,hits_only,both")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--full-runs", type=int, default=1, help="how often the --full leg alternates through the sides")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    if args.command == "build":
        return build(args.arms)
    if not args.parent_tree:
        ap.error("run needs --parent-tree")
    sides = []
    for s in args.sides.split(","):
        if s == "parent":
            sides.append((s, args.parent_tree, None))
        elif s == "both":
            sides.append((s, ROOT, None))
        else:
            lib = os.path.abspath(os.path.join(args.arms, s, "librpt_hip.so"))
            if not os.path.exists(lib):
                raise SystemExit(f"{lib} is missing: run `{sys.argv[0]} build` first")
            sides.append((s, ROOT, lib))
    lines = [ln for ln in args.lines.split(",") if ln]
    ms = {(ln, s): [] for ln in lines for s, _, _ in sides}
    for k in range(args.pairs):
        for ln in lines:
            for s, tree, lib in sides:
                d = bench(tree, lib, BASE + LINES[ln], args.timeout)
                ms[(ln, s)].append(d["ms_per_step"])
                print(f"pair {k} {ln:10s} {s:11s} ms_per_step {d['ms_per_step']:.5f}  value {d['value']}  kernel_ms {d.get('kernel_ms')}", flush=True)
    print()
    for ln in lines:
        pa = ms[(ln, sides[0][0])]
        for s, _, _ in sides:
            v = ms[(ln, s)]
            print(f"{ln:10s} {s:11s} median {statistics.median(v):.5f} ms  range [{min(v):.5f}, {max(v):.5f}]  / {sides[0][0]} median "
                  f"{statistics.median(v) / statistics.median(pa):.4f}  wholly below {sides[0][0]}: {max(v) < min(pa)}", flush=True)
    if args.full:
        print()
        for k, (s, tree, lib) in ((k, side) for k in range(args.full_runs) for side in sides):
            d = bench(tree, lib, BASE + ["--full", "--check", "--no-cpu-baseline"], 2 * args.timeout)
            one = d.get("one_frame_at_a_time") or {}
            print(f"full {k} {s:11s} ms_per_step {d['ms_per_step']:.5f}  one frame at a time {one.get('ms_per_frame')} ms (kernel {one.get('kernel_ms')})  "
                  f"animated {(d.get('animated') or {}).get('ms_per_step')}  check: {d.get('check')}", flush=True)


if __name__ == "__main__":
    main()
