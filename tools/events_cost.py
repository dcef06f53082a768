#!/usr/bin/env python3
"""What an event pass costs (rpt_render_events) next to the colour frame of the same library, on the same contexts, A/B/A/B: ms per frame
one at a time (rpt_set_objects + the blocking call) and with four contexts in flight (the async call on four contexts sharing the scene),
the method of DESIGN.md section 6: wall clock over `--frames` frames per arm after a warm-up frame, `--rounds` alternations, the median
of the arms.  The colour kernels are the parent commit's machine code (profiles/r09_events_kernel_code_diff.txt), so the colour column is
a baseline outside the code under test.  Prints one line per arm, then a table and a JSON summary with the library's SHA-256.

Every configuration runs in a child process of its own under a time limit, one after the other, and the first failure ends the run:
nothing more is started on the device after a fault, an abort or a timeout.

usage: python tools/events_cost.py [--frames 400] [--rounds 3] [--out profiles/r09_events_cost.txt]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("bunny", 0.0, 3840, 2160), ("shadows", 16.0, 3840, 2160), ("cubes", 3.0, 3840, 2160), ("arch", 5.25, 1920, 1080)]
CAMERA_V = {"bunny": (0.0, 0.0, 0.0), "shadows": (0.0, 0.0, 0.0), "cubes": (0.3, 0.0, 0.1), "arch": (0.0, 0.0, 0.95)}      # the benchmark's own states
IN_FLIGHT = 4
STEP_TIMEOUT = 240      # seconds per configuration


def one_at_a_time(r, s, frames, events):
    t0 = time.perf_counter()
    for _ in range(frames):
        r.set_objects(s)
        if events:
            r._check(r._lib.rpt_render_events(r._h), "rpt_render_events")
        else:
            r.render()
    return (time.perf_counter() - t0) / frames * 1e3


def in_flight(slots, s, frames, events):
    t0 = time.perf_counter()
    for f in range(frames * len(slots)):
        r = slots[f % len(slots)]
        r.sync()
        r.set_objects(s)
        if events:
            r.render_events(async_=True)
        else:
            r.render_async()
    for r in slots:
        r.sync()
    return (time.perf_counter() - t0) / (frames * len(slots)) * 1e3


def child(index, frames, rounds):
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    name, t, W, H = CONFIGS[index]
    s = Scene.from_file(name)
    s.set_camera(CAMERA_V[name], t)
    s.update_objects()
    slots = [Renderer(0) for _ in range(IN_FLIGHT)]
    slots[0].upload_scene(s)
    for r in slots[1:]:
        r.share_scene(slots[0])
    for r in slots:
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.set_objects(s)
    res = {arm: {"one": [], "flight": []} for arm in ("colour", "events")}
    kernels = {}
    for rnd in range(rounds):
        for arm in ("colour", "events"):
            ev = arm == "events"
            for r in slots:                      # warm-up frame of this arm
                if ev:
                    r._check(r._lib.rpt_render_events(r._h), "rpt_render_events")      # (Renderer.render_events would also read 265 MB back)
                else:
                    r.render()
            one = one_at_a_time(slots[0], s, frames, ev)
            kb = slots[0].last_events_variant() if ev else slots[0].last_variant()
            fl = in_flight(slots, s, frames, ev)
            kf = slots[0].last_events_variant() if ev else slots[0].last_variant()
            kernels[arm] = [kb, kf]
            res[arm]["one"].append(one)
            res[arm]["flight"].append(fl)
            print(f"{name:8s} {W}x{H} round {rnd} {arm:6s}: one at a time {one:8.4f} ms (kernel {kb})   {IN_FLIGHT} in flight {fl:8.4f} ms/frame (kernel {kf})", flush=True)
    row = {"scene": name, "size": [W, H], "kernels": kernels}
    for mode in ("one", "flight"):
        c, e = statistics.median(res["colour"][mode]), statistics.median(res["events"][mode])
        row[f"ms_{mode}_colour"], row[f"ms_{mode}_events"], row[f"ratio_{mode}"] = round(c, 4), round(e, 4), round(e / c, 3)
    for r in slots:
        r.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3, help="colour / events pairs per configuration")
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.frames, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    lines = [f"librpt_hip.so sha256 {hashlib.sha256(open(_ffi.hip_lib_path(), 'rb').read()).hexdigest()}",
             f"method: wall clock over {args.frames} frames per arm after a warm-up frame, {args.rounds} colour / events alternations, median of the arms;",
             f"        one at a time = rpt_set_objects + the blocking call on one context; in flight = the async call on {IN_FLIGHT} contexts sharing the scene", ""]
    rows = []
    for k in range(len(CONFIGS)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--frames", str(args.frames), "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=STEP_TIMEOUT)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print(f"configuration {CONFIGS[k]} ended with status {p.returncode}: stopping here", flush=True)
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
            else:
                lines.append(line)
    lines += ["", f"{'scene':8s} {'size':>10s} | {'colour one':>10s} {'events one':>10s} {'ratio':>6s} | {'colour x4':>10s} {'events x4':>10s} {'ratio':>6s} | kernels (colour; events)"]
    for r in rows:
        lines.append(f"{r['scene']:8s} {r['size'][0]:>5d}x{r['size'][1]:<4d} | {r['ms_one_colour']:10.4f} {r['ms_one_events']:10.4f} {r['ratio_one']:6.3f} | "
                     f"{r['ms_flight_colour']:10.4f} {r['ms_flight_events']:10.4f} {r['ratio_flight']:6.3f} | {r['kernels']['colour']}; {r['kernels']['events']}")
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
