#!/usr/bin/env python3
"""A/B of two built checkouts on one bench.py line, runs alternating A B A B ... in one job (each side's bench.py with its own
package and libraries).  Used for the triangle test's exact reciprocal: A = a built checkout of the parent revision,
B = this tree.
usage (GPU box): python3 tools/exact_rcp_ab.py --tree-a path/to/parent/checkout [--tree-b .] [--pairs 3] [bench.py args ...]
Prints one line per run and a summary: the median of each side, the ranges, and the median of the pairwise B/A ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(tree, bench_args, timeout):
    env = dict(os.environ)
    env.pop("RPT_HIP_LIB", None)
    tree = os.path.abspath(tree)
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + bench_args, capture_output=True, text=True, env=env, timeout=timeout, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"bench.py failed ({tree}, rc {p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree-a", required=True)
    ap.add_argument("--tree-b", default=ROOT)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600)
    args, bench_args = ap.parse_known_args()
    if not bench_args:
        bench_args = ["--gpus", "1", "--steps", "50", "--warmup", "5"]
    side = {"A": [], "B": []}
    for k in range(args.pairs):
        for name, tree in (("A", args.tree_a), ("B", args.tree_b)):
            d = run(tree, bench_args, args.timeout)
            side[name].append(d["ms_per_step"])
            print(f"pair {k} {name}: ms_per_step {d['ms_per_step']:.5f}  value_blocking {d.get('value_blocking')}  check {d.get('check')}", flush=True)
    ratios = [b / a for a, b in zip(side["A"], side["B"])]
    ma, mb = statistics.median(side["A"]), statistics.median(side["B"])
    print(f"A median {ma:.5f} ms [{min(side['A']):.5f}, {max(side['A']):.5f}]   B median {mb:.5f} ms [{min(side['B']):.5f}, {max(side['B']):.5f}]   "
          f"B/A median of pairs {statistics.median(ratios):.4f}   ranges overlap: {max(side['B']) >= min(side['A']) and max(side['A']) >= min(side['B'])}", flush=True)


if __name__ == "__main__":
    main()
