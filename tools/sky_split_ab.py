#!/usr/bin/env python3
"""A/B of the sky split (csrc/rpt_api.hip: launch, rpt_sky_fill_kernel) against the parent revision.

Sides: `parent` = a built checkout of the parent revision (its own bench.py, package and libraries); `commit` = this tree as built.  Never
this tree with a switch off in the parent's place: the gate compares revisions.

    python3 tools/sky_split_ab.py run --parent-tree DIR [--pairs 5] [--lines headline,bunny1080,...] [--full 3]
    python3 tools/sky_split_ab.py sky --parent-tree DIR
    python3 tools/sky_split_ab.py counters --parent-tree DIR
    python3 tools/sky_split_ab.py boxes

`run` alternates the sides `--pairs` times in ONE job on every line of --lines (bench.py --gpus 1 --steps 50 --warmup 5 plus the line's
own arguments), the order swapping pair by pair, then with --full N alternates `bench.py --full --check` N times per side (one frame at a
time, the animated figure, the check against the oracle).  Every bench.py run sits under its own `timeout`, the runs are chained, and the
tool stops at the first non-zero status.  One row per run and, per line and side, the range of `value`; the gate is met on a line when
all of the commit's values lie above all of the parent's.
--wide-lines adds a third arm on the lines it names, reported only: this tree with RPT_SKY_SPLIT_SHARE=100, i.e. split whatever the box covers.
`sky` times the fill alone over the whole 4K frame (the diagnostics library's arm 786, this tree) against the parent's frame of an empty
Object[] (129 600 one-wave workgroups that store), 200 frames back to back on one stream, three times per side, alternating.
`counters` runs each side's headline once under rocprofv3 with `--kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU`
and nothing else, and prints the per-launch means of every kernel.
`boxes` prints, for every line, the kernel and the box of tiles this tree's rule chose (rpt_last_sky_split)."""
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
    "bunny1440": ["--width", "2560", "--height", "1440"],      # 3.7 Mpx and 5.8 Mpx, kernel 41 in flight: what the rule's pixel floor was taken from
    "bunny1800": ["--width", "3200", "--height", "1800"],      # (RPT_SKY_SPLIT_MIN_PIXELS=3000000 in the environment splits them)
    "bunny8k": ["--width", "7680", "--height", "4320"],
    "shadows4k": ["--workload", "shadows"],
    "cubes4k": ["--workload", "cubes"],
    "arch1080": ["--workload", "arch", "--width", "1920", "--height", "1080"],
    "cube640": ["--workload", "cube", "--width", "640", "--height", "480"],
}
BASE = ["--gpus", "1", "--steps", "50", "--warmup", "5"]
PMC = "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU"

SKY_SNIPPET = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from relativitypathtracer_amd import Scene
from relativitypathtracer_amd.renderer import Renderer
s = Scene.from_file("bunny"); s.set_camera((0, 0, 0), 0.0); s.update_objects()
r = Renderer(0); r.upload_scene(s); r.set_scene_params(s, 3840, 2160); r.set_objects(np.zeros(0, dtype=np.uint8))
r.set_variant(int(sys.argv[2])); r.timed_frames(20)
print("SKY", r.last_variant(), " ".join(f"{r.timed_frames(200):.5f}" for _ in range(3)))
"""

BOX_SNIPPET = r"""
import sys
sys.path.insert(0, sys.argv[1])
import bench
from relativitypathtracer_amd import Scene
from relativitypathtracer_amd.renderer import Renderer
for name, W, H in [("bunny", 3840, 2160), ("bunny", 1920, 1080), ("bunny", 2560, 1440), ("bunny", 3200, 1800), ("bunny", 7680, 4320), ("shadows", 3840, 2160), ("cubes", 3840, 2160), ("arch", 1920, 1080), ("cube", 640, 480)]:
    scene, v, t = bench.WORKLOADS[name]
    s = Scene.from_file(scene); s.set_camera(v, t); s.update_objects()
    r = Renderer(0); r.upload_scene(s); r.set_scene_params(s, W, H); r.set_objects(s)
    r.render_async(); r.sync(); a = (r.last_variant(), r.last_sky_split())
    r.render(); b = (r.last_variant(), r.last_sky_split())
    print(f"BOX {name} {W}x{H}: {(W + 7) // 8} x {(H + 7) // 8} tiles; in flight kernel {a[0]} box {a[1]}; blocking kernel {b[0]} box {b[1]}", flush=True)
    r.close()
"""


def run(cmd, tree, limit, env_extra=None):
    """One command under its own `timeout`; the tool ends at the first non-zero status (nothing more is started on the device)."""
    env = dict(os.environ)
    env.pop("RPT_HIP_LIB", None)
    env.pop("RPT_SKY_SPLIT_SHARE", None)
    env.pop("RPT_SKY_SPLIT_MIN_PIXELS", None)
    env.update(env_extra or {})
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"stopped: {' '.join(cmd)} in {tree} ended with status {p.returncode}\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
    return p.stdout


def bench(tree, bench_args, limit, env=None):
    out = run([sys.executable, os.path.join(tree, "bench.py")] + bench_args, tree, limit, env)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def counters(sides, limit):
    for name, tree in sides:
        with tempfile.TemporaryDirectory() as d:
            run(["rocprofv3", "--kernel-trace", "--pmc", *PMC.split(), "--output-format", "csv", "-d", d, "-o", "pmc", "--",
                 sys.executable, os.path.join(tree, "bench.py")] + BASE, tree, limit)
            sums, launches = {}, {}
            for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                per_dispatch = {}
                for row in csv.DictReader(open(path)):       # (a counter may come as one row per dimension: summed per dispatch first)
                    key = (row["Dispatch_Id"], row["Kernel_Name"].split("(")[0][:60], row["Counter_Name"])
                    per_dispatch[key] = per_dispatch.get(key, 0.0) + float(row["Counter_Value"])
                for (_, k, c), v in per_dispatch.items():
                    sums[(k, c)] = sums.get((k, c), 0.0) + v
                    launches[(k, c)] = launches.get((k, c), 0) + 1
            for k in sorted({k for k, _ in sums}):
                cs = {c: (v, launches[(kk, c)]) for (kk, c), v in sums.items() if kk == k}
                print(f"{name:7s} {k}: {min(n for _, n in cs.values())} launches; per launch " + ", ".join(f"{c} {v / n:.0f}" for c, (v, n) in sorted(cs.items())), flush=True)


def sky(sides, limit):
    (_, parent), (_, commit) = sides
    for k in range(3):
        for name, tree, variant, env in (("parent", parent, 0, None), ("commit", commit, 786, {"RPT_HIP_LIB": os.path.join(commit, "relativitypathtracer_amd", "librpt_hip_diag.so")})):
            out = run([sys.executable, "-c", SKY_SNIPPET, tree, str(variant)], tree, limit, env)
            print(f"sky round {k} {name:7s} " + [ln for ln in out.splitlines() if ln.startswith("SKY")][-1] + "   (kernel, ms per frame x 3)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["run", "sky", "counters", "boxes"])
    ap.add_argument("--parent-tree")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--lines", default=",".join(LINES))
    ap.add_argument("--wide-lines", default="", help="lines that get a third arm, reported only: this tree with RPT_SKY_SPLIT_SHARE=100 (the rule's share is decided from it)")
    ap.add_argument("--full", type=int, default=0, help="after the lines: `bench.py --full --check` this many times per side")
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each bench.py run (twice that with --full and under the profiler)")
    args = ap.parse_args()
    if args.command == "boxes":
        print(run([sys.executable, "-c", BOX_SNIPPET, ROOT], ROOT, 2 * args.timeout), end="")
        return
    if not args.parent_tree:
        ap.error("--parent-tree is needed")
    sides = [("parent", os.path.abspath(args.parent_tree)), ("commit", ROOT)]
    if args.command == "counters":
        return counters(sides, 2 * args.timeout)
    if args.command == "sky":
        return sky(sides, args.timeout)
    lines = [ln for ln in args.lines.split(",") if ln]
    wide = [ln for ln in args.wide_lines.split(",") if ln]
    for ln in lines:
        arms = sides + ([("wide", ROOT)] if ln in wide else [])
        values = {s: [] for s, _ in arms}
        for k in range(args.pairs):
            for s, tree in (arms if k % 2 == 0 else arms[::-1]):
                d = bench(tree, BASE + LINES[ln], args.timeout, {"RPT_SKY_SPLIT_SHARE": "100"} if s == "wide" else None)
                values[s].append(d["value"])
                print(f"{ln:10s} pair {k} {s:7s} value {d['value']}  ms_per_step {d['ms_per_step']:.5f}  batches {d.get('ms_per_step_batches')}  kernel_ms {d.get('kernel_ms')}", flush=True)
        pa, co = values["parent"], values["commit"]
        print(f"{ln:10s} parent [{min(pa)}, {max(pa)}]  commit [{min(co)}, {max(co)}]  commit / parent (medians) "
              f"{sorted(co)[len(co) // 2] / sorted(pa)[len(pa) // 2]:.4f}  all of the commit's above all of the parent's: {min(co) > max(pa)}", flush=True)
        if ln in wide:
            wi = values["wide"]
            print(f"{ln:10s} wide (share 100 %) [{min(wi)}, {max(wi)}]  wide / parent (medians) {sorted(wi)[len(wi) // 2] / sorted(pa)[len(pa) // 2]:.4f}", flush=True)
        print(flush=True)
    for k in range(args.full):
        for s, tree in (sides if k % 2 == 0 else sides[::-1]):
            d = bench(tree, BASE + ["--full", "--check", "--no-cpu-baseline"], 2 * args.timeout)
            one = d.get("one_frame_at_a_time") or {}
            print(f"full round {k} {s:7s} value {d['value']}  one frame at a time {one.get('ms_per_frame')} ms (kernel {one.get('kernel_ms')})  "
                  f"animated {(d.get('animated') or {}).get('ms_per_step')} ms  check: {d.get('check')}", flush=True)


if __name__ == "__main__":
    main()
