#!/usr/bin/env python3
"""A/B of kernel 41 at six waves per SIMD with its shading state parked in LDS against the parent revision, in the
form of tools/sky_split_ab.py (whose lines, runner and counter reader this tool uses).

Sides: `parent` = a built checkout of the parent revision (its own bench.py, package and libraries); `commit` = this tree as built.

    python3 tools/six_waves_ab.py run --parent-tree DIR [--pairs 3] [--lines headline,bunny8k,...] [--share0-lines headline] [--arm42-lines headline] [--full 3]
    python3 tools/six_waves_ab.py identity --parent-tree DIR
    python3 tools/six_waves_ab.py counters --parent-tree DIR

`run` alternates the sides `--pairs` times in ONE job on every line (bench.py --gpus 1 --steps 50 --warmup 5 plus the line's own
arguments), the order swapping pair by pair; the gate is met on a line when all of the commit's values lie above all of the parent's.
On --share0-lines both sides run a second time with RPT_SKY_SPLIT_SHARE=0 (no sky split: does the fill still pay beside six walkers?);
on --arm42-lines a third arm, reported only: this tree's diagnostics library with --variant 42, kernel 41 WITHOUT the parking at six
waves (the compiler's spills) — the sixth wave apart from the parking.  --full N: `bench.py --full --check` N times per side.
`identity` runs each side's headline once with --dump-outputs and compares the files byte for byte.
`counters` runs each side's headline once under rocprofv3 with the kernel trace and one set of counters and nothing else."""
import argparse
import filecmp
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sky_split_ab as ab       # noqa: E402

PMC_SETS = {"waves": "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU", "lds": "SQ_INSTS_LDS SQ_INSTS_VALU SQ_WAVES",
            "life": "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES", "bytes": "FETCH_SIZE WRITE_SIZE"}


def spread(name, values):
    return f"{name} [{min(values)}, {max(values)}]"


def median(values):
    return sorted(values)[len(values) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["run", "identity", "counters"])
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--lines", default="headline,bunny8k,shadows4k,bunny1440,bunny1800,cubes4k")
    ap.add_argument("--share0-lines", default="")
    ap.add_argument("--arm42-lines", default="")
    ap.add_argument("--full", type=int, default=0)
    ap.add_argument("--pmc", default="waves", choices=sorted(PMC_SETS), help="counters: which set this run collects (one set per run)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each bench.py run (twice that with --full and under the profiler)")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree)
    sides = [("parent", parent), ("commit", ROOT)]
    if args.command == "counters":
        ab.PMC = PMC_SETS[args.pmc]
        return ab.counters(sides, 2 * args.timeout)
    if args.command == "identity":
        with tempfile.TemporaryDirectory() as tmp:
            for name, tree in sides:
                ab.bench(tree, ab.BASE + ["--dump-outputs", os.path.join(tmp, name)], args.timeout)
            a, b = os.path.join(tmp, "parent"), os.path.join(tmp, "commit")
            files = sorted(os.listdir(a))
            _, differ, errors = filecmp.cmpfiles(a, b, files, shallow=False)
            print(f"identity: {len(files)} files ({', '.join(files)}); differing: {differ + errors or 'none'}", flush=True)
            return 1 if differ or errors or sorted(os.listdir(b)) != files else 0
    share0 = [ln for ln in args.share0_lines.split(",") if ln]
    arm42 = [ln for ln in args.arm42_lines.split(",") if ln]
    diag = {"RPT_HIP_LIB": os.path.join(ROOT, "relativitypathtracer_amd", "librpt_hip_diag.so")}
    for ln in [ln for ln in args.lines.split(",") if ln]:
        arms = [(s, tree, ab.BASE + ab.LINES[ln], None) for s, tree in sides]
        if ln in share0:
            arms += [(s + "-share0", tree, ab.BASE + ab.LINES[ln], {"RPT_SKY_SPLIT_SHARE": "0"}) for s, tree in sides]
        if ln in arm42:
            arms += [("arm42", ROOT, ab.BASE + ab.LINES[ln] + ["--variant", "42"], diag)]
        values = {a[0]: [] for a in arms}
        for k in range(args.pairs):
            for s, tree, cmd, env in (arms if k % 2 == 0 else arms[::-1]):
                d = ab.bench(tree, cmd, args.timeout, env)
                values[s].append(d["value"])
                print(f"{ln:10s} pair {k} {s:14s} value {d['value']}  ms_per_step {d['ms_per_step']:.5f}  batches {d.get('ms_per_step_batches')}  kernel_ms {d.get('kernel_ms')}", flush=True)
        pa, co = values["parent"], values["commit"]
        print(f"{ln:10s} {spread('parent', pa)}  {spread('commit', co)}  commit / parent (medians) {median(co) / median(pa):.4f}  "
              f"all of the commit's above all of the parent's: {min(co) > max(pa)}", flush=True)
        for s in values:
            if s not in ("parent", "commit"):
                print(f"{ln:10s} {spread(s, values[s])}  {s} / parent (medians) {median(values[s]) / median(pa):.4f}", flush=True)
        print(flush=True)
    for k in range(args.full):
        for s, tree in (sides if k % 2 == 0 else sides[::-1]):
            d = ab.bench(tree, ab.BASE + ["--full", "--check", "--no-cpu-baseline"], 2 * args.timeout)
            one = d.get("one_frame_at_a_time") or {}
            print(f"full round {k} {s:7s} value {d['value']}  one frame at a time {one.get('ms_per_frame')} ms (kernel {one.get('kernel_ms')})  "
                  f"animated {(d.get('animated') or {}).get('ms_per_step')} ms  check: {d.get('check')}", flush=True)


if __name__ == "__main__":
    sys.exit(main())
