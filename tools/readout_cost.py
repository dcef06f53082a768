#!/usr/bin/env python3
"""What the readout pass costs (rpt_render_readouts) next to the colour frame of the same view and next to the overlay pass with outlines
only on the same frame: device time between HIP events on the context's launch stream.  Per scene and round the arms alternate —
  every     a display on every object (4 digits, 2 decimals, the default rectangle);
  none      readouts set, no object has a display: every wave reads its records' first 16 B and leaves;
  outlines  rpt_render_overlay with the outlines alone, the overlay kernel's cheapest form —
each `--frames` times: a colour frame (rpt_render_async) between one pair of events, an event frame between a second pair, the pass
between a third, so every pass blends into a fresh picture.  The median over `--rounds` rounds and the spread (max - min) / median are
reported, and each arm's ratio to the colour frame and to the outlines.  Scenes: rulers and ladder_paradox at 3840 x 2160, light delay on.

Every scene runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/readout_cost.py [--frames 40] [--rounds 3] [--out profiles/r17_readout_cost.txt]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
CONFIGS = [("rulers", 2.5), ("ladder_paradox", 1.0)]       # scene, camera time
ARMS = ("every", "none", "outlines")
STEP_TIMEOUT = 300      # seconds per scene


def child(index, frames, rounds):
    import torch
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    name, t = CONFIGS[index]
    s = Scene.from_file(name)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, 0.0), t)
    s.update_objects()
    n = len(s.objects())
    stream = torch.cuda.Stream()
    r = Renderer(0)
    r.set_stream(stream.cuda_stream)
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.render()
    records = r.render_events()
    every = [dict(rate=1.0, offset=0.0, digits=4, decimals=2)] * n
    hit = records["object"] >= 0
    settings = {"every": every, "none": [None] * n}
    times = {k: [] for k in ("colour", "events", *ARMS)}
    changed = {}
    for rnd in range(rounds):
        for arm in ARMS:
            if arm == "outlines":
                r.set_readouts(None)
                r.set_overlay(outlines=True)
            else:
                r.set_overlay()
                r.set_readouts(settings[arm])
            run = (lambda: r.render_overlay(async_=True)) if arm == "outlines" else (lambda: r.render_readouts(async_=True))
            r.render_async()                        # warm-up of the three passes
            r.render_events(async_=True)
            run()
            r.sync()
            marks = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(frames)]
            for m in marks:
                m[0].record(stream)
                r.render_async()
                m[1].record(stream)
                r.render_events(async_=True)
                m[2].record(stream)
                run()
                m[3].record(stream)
            r.sync()
            colour = sum(m[0].elapsed_time(m[1]) for m in marks) / frames
            events = sum(m[1].elapsed_time(m[2]) for m in marks) / frames
            took = sum(m[2].elapsed_time(m[3]) for m in marks) / frames
            times["colour"].append(colour)
            times["events"].append(events)
            times[arm].append(took)
            changed[arm] = r.last_overlay_pixels() if arm == "outlines" else r.last_readout_pixels()
            print(f"{name:15s} {W}x{H} round {rnd} {arm:9s}: colour {colour:8.4f} ms (kernel {r.last_variant()})  events {events:8.4f} ms (kernel {r.last_events_variant()})  "
                  f"pass {took:8.4f} ms, {changed[arm]} pixels changed", flush=True)
    row = {"scene": name, "size": [W, H], "objects": n, "hit_share": round(float(hit.mean()), 4), "changed": changed}
    for k, v in times.items():
        row[f"ms {k}"] = round(statistics.median(v), 4)
        row[f"spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
    for arm in ARMS:
        row[f"ratio to colour, {arm}"] = round(row[f"ms {arm}"] / row["ms colour"], 4)
        row[f"ratio to outlines, {arm}"] = round(row[f"ms {arm}"] / row["ms outlines"], 4)
    r.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.frames, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    lines = [f"librpt_hip.so sha256 {hashlib.sha256(open(_ffi.hip_lib_path(), 'rb').read()).hexdigest()}",
             f"method: device time between HIP events on the launch stream; per round and arm {args.frames} x (colour frame | event frame | the pass), each between its own pair of events,",
             f"        the arms alternating within each of {args.rounds} rounds, median of the rounds (spread = (max - min) / median)", ""]
    rows = []
    for k in range(len(CONFIGS)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--frames", str(args.frames), "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=STEP_TIMEOUT)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print(f"scene {CONFIGS[k][0]} ended with status {p.returncode}: stopping here", flush=True)
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
            else:
                lines.append(line)
    lines += ["", f"{'scene':15s} {'hit':>6s} | {'colour ms':>9s} {'events ms':>9s} | {'every ms':>9s} {'/ colour':>8s} {'/ outl.':>8s} | {'none ms':>9s} {'/ colour':>8s} {'/ outl.':>8s} | "
                  f"{'outlines ms':>11s} {'/ colour':>8s} | largest spread"]
    for r in rows:
        spread = max(v for k, v in r.items() if k.startswith("spread "))
        lines.append(f"{r['scene']:15s} {100 * r['hit_share']:5.1f}% | {r['ms colour']:9.4f} {r['ms events']:9.4f} | "
                     f"{r['ms every']:9.4f} {r['ratio to colour, every']:8.4f} {r['ratio to outlines, every']:8.4f} | {r['ms none']:9.4f} {r['ratio to colour, none']:8.4f} {r['ratio to outlines, none']:8.4f} | "
                     f"{r['ms outlines']:11.4f} {r['ratio to colour, outlines']:8.4f} | {100 * spread:.1f}%")
    lines += ["", json.dumps(rows)]
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
