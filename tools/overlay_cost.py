#!/usr/bin/env python3
"""What the overlay pass costs (rpt_render_overlay) next to the colour frame and the event frame of the same view: device time between HIP
events on the context's launch stream.  Per scene and round, `--frames` times: a colour frame (rpt_render_async) between one pair of events,
an event frame between a second pair, the overlay between a third — so every overlay pass blends into a fresh picture (a pass repeated on
its own result soon changes, and writes, nothing) — and the arm's time is the sum of its pairs over `--frames`.  The median over `--rounds`
rounds and the spread (max - min) / median are reported, the overlay's ratio to the colour frame, and its achieved bytes per second
against the 40 B per pixel the algorithm needs: the 32-B record read once, 4 B of the framebuffer read and 4 B written.  Two overlay
arms: all five layers with the tint's range found on the device (kernel 1101, then 1100) and with the range passed (1100 alone).
Scenes: rulers, ladder_paradox and shadows at 3840 x 2160, light delay on.

Every scene runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/overlay_cost.py [--frames 40] [--rounds 3] [--out profiles/r12_overlay_cost.txt]"""
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
#          scene             t     contour steps in the scene's units
CONFIGS = [("rulers", 2.5, dict(delay_step=0.5, clock_step=0.5, lattice_step=(1.0, 1.0, 1.0))),
           ("ladder_paradox", 1.0, dict(delay_step=0.5, clock_step=0.5, lattice_step=(1.0, 1.0, 1.0))),
           ("shadows", 16.0, dict(delay_step=2.0, clock_step=2.0, lattice_step=(2.0, 2.0, 2.0)))]
BYTES_PER_PIXEL = 40
STEP_TIMEOUT = 300      # seconds per scene


def child(index, frames, rounds):
    import numpy as np
    import torch
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    name, t, steps = CONFIGS[index]
    s = Scene.from_file(name)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, 0.0), t)
    s.update_objects()
    stream = torch.cuda.Stream()
    r = Renderer(0)
    r.set_stream(stream.cuda_stream)
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.render()
    records = r.render_events()
    hit = records["object"] >= 0
    t_max = float(np.abs(records["dist"][hit]).max()) if hit.any() else 1.0
    layers = dict(outlines=True, tint=True, **steps)
    arms = {"overlay, range on the device": dict(layers, tint_t_max=0.0), "overlay, range passed": dict(layers, tint_t_max=t_max)}
    times = {k: [] for k in ("colour", "events", *arms)}
    changed = {}
    for rnd in range(rounds):
        for arm, kw in arms.items():
            r.set_overlay(**kw)
            r.render_async()                        # warm-up of the three passes
            r.render_events(async_=True)
            r.render_overlay(async_=True)
            r.sync()
            marks = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(frames)]
            for m in marks:
                m[0].record(stream)
                r.render_async()
                m[1].record(stream)
                r.render_events(async_=True)
                m[2].record(stream)
                r.render_overlay(async_=True)
                m[3].record(stream)
            r.sync()
            colour = sum(m[0].elapsed_time(m[1]) for m in marks) / frames
            events = sum(m[1].elapsed_time(m[2]) for m in marks) / frames
            over = sum(m[2].elapsed_time(m[3]) for m in marks) / frames
            times["colour"].append(colour)
            times["events"].append(events)
            times[arm].append(over)
            changed[arm] = r.last_overlay_pixels()
            print(f"{name:15s} {W}x{H} round {rnd} {arm:30s}: colour {colour:8.4f} ms (kernel {r.last_variant()})  events {events:8.4f} ms (kernel {r.last_events_variant()})  "
                  f"overlay {over:8.4f} ms, {changed[arm]} pixels changed", flush=True)
    row = {"scene": name, "size": [W, H], "hit_share": round(float(hit.mean()), 4), "changed": changed}
    for k, v in times.items():
        row[f"ms {k}"] = round(statistics.median(v), 4)
        row[f"spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
    for arm in arms:
        row[f"ratio to colour, {arm}"] = round(row[f"ms {arm}"] / row["ms colour"], 4)
        row[f"GB/s, {arm}"] = round(BYTES_PER_PIXEL * W * H / (row[f"ms {arm}"] * 1e-3) / 1e9, 1)
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
             f"method: device time between HIP events on the launch stream; per round {args.frames} x (colour frame | event frame | overlay), each between its own pair of events,",
             f"        {args.rounds} rounds per overlay arm, median of the rounds (spread = (max - min) / median); bytes/s = {BYTES_PER_PIXEL} B/pixel x {W} x {H} / overlay time", ""]
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
    lines += ["", f"{'scene':15s} {'hit':>6s} | {'colour ms':>9s} {'events ms':>9s} | {'overlay ms':>10s} {'/ colour':>8s} {'GB/s':>7s} | {'range passed':>12s} {'/ colour':>8s} {'GB/s':>7s} | largest spread"]
    for r in rows:
        a, b = "overlay, range on the device", "overlay, range passed"
        spread = max(v for k, v in r.items() if k.startswith("spread "))
        lines.append(f"{r['scene']:15s} {100 * r['hit_share']:5.1f}% | {r['ms colour']:9.4f} {r['ms events']:9.4f} | {r['ms ' + a]:10.4f} {r['ratio to colour, ' + a]:8.4f} {r['GB/s, ' + a]:7.1f} | "
                     f"{r['ms ' + b]:12.4f} {r['ratio to colour, ' + b]:8.4f} {r['GB/s, ' + b]:7.1f} | {100 * spread:.1f}%")
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
