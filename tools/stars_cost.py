#!/usr/bin/env python3
"""What the star-field pass costs (rpt_render_stars) at 3840 x 2160, and whether the catalogue's spatial order pays:
device time of its two kernels — the splat (1120, the scattered integer atomics) and the resolve (1121) — between HIP events the library
records around them (rpt_set_stars_measurement), next to the overlay's outlines pass on the same frame, which reads and writes the same
framebuffer and records without scattering.  Per camera (at rest; gamma = 5 along the view axis, where half the sky crowds into the
middle of the frame), catalogue size (10^4, 10^5, 10^6 stars of stars.random_catalogue) and catalogue order (as generated, which is
random; sorted here by a spatial key — the cube face of dir, then the Morton code of the two other components, 10 bits each — so that a
wave's taps fall near each other: the library keeps whatever order it is given): `--frames` times a colour frame, an event frame, the outlines and the star-field pass, so every pass adds
to a fresh picture; the arm's time is the mean over the frames, the median over `--rounds` rounds and the spread (max - min) / median
are reported.  Atomic bytes per second = 8 B x the non-zero taps' channels the float64 model counts inside the frame / the splat's time.

Every camera runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/stars_cost.py [--frames 20] [--rounds 3] [--out profiles/stars_cost.txt]"""
import argparse
import hashlib
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
SCENE, SCENE_T = "cubes", 3.0
CAMERAS = [("at rest", 0.0), ("gamma 5", math.sqrt(1.0 - 1.0 / 25.0))]
COUNTS = [10 ** 4, 10 ** 5, 10 ** 6]
STEP_TIMEOUT = 420      # seconds per camera


def spatial_order(cat):
    """The catalogue sorted by cube face and Morton code of its directions (stable)."""
    import numpy as np
    d = cat["dir"].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = np.argmax(np.abs(d), axis=1)
    rows = np.arange(len(d))
    major = d[rows, axis]
    u, v = d[rows, (axis + 1) % 3] / np.abs(major), d[rows, (axis + 2) % 3] / np.abs(major)

    def spread(c):
        c = np.clip(((c * 0.5 + 0.5) * 1024.0).astype(np.int64), 0, 1023)
        c = (c | (c << 8)) & 0x00ff00ff
        c = (c | (c << 4)) & 0x0f0f0f0f
        c = (c | (c << 2)) & 0x33333333
        return (c | (c << 1)) & 0x55555555

    key = ((2 * axis + (major < 0)) << 20) | spread(u) | (spread(v) << 1)
    return cat[np.argsort(key, kind="stable")]


def atomic_words(cat, E, camera):
    """The 8-byte adds the splat makes: per star, its taps inside the frame times its non-zero channels (float64 model, beaming + shift)."""
    import numpy as np
    from relativitypathtracer_amd import stars
    p = stars.project(cat, E, -1, camera, doppler=3)
    ok = p["visible"] & np.isfinite(p["X"]) & np.isfinite(p["Y"])
    x0, y0 = np.floor(p["X"][ok]), np.floor(p["Y"][ok])
    taps = np.zeros(int(ok.sum()))
    for dx in (0, 1):
        for dy in (0, 1):
            taps += ((x0 + dx >= 0) & (x0 + dx < W) & (y0 + dy >= 0) & (y0 + dy < H))
    return int((taps * (p["rgb"][ok] > 0).sum(axis=1)).sum())


def child(index, frames, rounds):
    import torch
    from relativitypathtracer_amd import Scene, stars
    from relativitypathtracer_amd.renderer import Renderer
    label, beta = CAMERAS[index]
    s = Scene.from_file(SCENE)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, beta), SCENE_T if beta == 0.0 else 0.0)
    s.update_objects()
    E = s.camera_lorentz()[1]
    stream = torch.cuda.Stream()
    r = Renderer(0)
    r.set_stream(stream.cuda_stream)
    r.set_doppler(True, True)
    r.set_environment_frame(E)
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.set_overlay(outlines=True)
    camera = dict(mode="pinhole", width=W, height=H)
    for n in COUNTS:
        cat = stars.random_catalogue(n, 1)
        words = atomic_words(cat, E, camera)
        row = {"camera": label, "stars": n, "atomic words": words}
        for order in ("spatial order", "caller's order"):
            r.set_stars_measurement(timed=True)
            r.set_stars(spatial_order(cat) if order == "spatial order" else cat)
            times = {k: [] for k in ("colour", "events", "outlines", "splat", "resolve")}
            for rnd in range(rounds):
                r.render_async()                        # warm-up of the four passes
                r.render_events(async_=True)
                r.render_overlay(async_=True)
                r.render_stars(async_=True)
                r.sync()
                sums = dict.fromkeys(times, 0.0)
                for _ in range(frames):
                    m = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    m[0].record(stream)
                    r.render_async()
                    m[1].record(stream)
                    r.render_events(async_=True)
                    m[2].record(stream)
                    r.render_overlay(async_=True)
                    m[3].record(stream)
                    r.render_stars(async_=True)
                    r.sync()
                    splat, resolve = r.last_stars_ms()
                    for k, v in zip(times, (m[0].elapsed_time(m[1]), m[1].elapsed_time(m[2]), m[2].elapsed_time(m[3]), splat, resolve)):
                        sums[k] += v
                for k in times:
                    times[k].append(sums[k] / frames)
                inside, changed = r.last_stars()
                print(f"{label:8s} {n:8d} stars, {order:14s} round {rnd}: colour {times['colour'][-1]:7.4f} ms  events {times['events'][-1]:7.4f}  outlines {times['outlines'][-1]:7.4f}  "
                      f"splat {times['splat'][-1]:7.4f}  resolve {times['resolve'][-1]:7.4f}  ({inside} stars inside, {changed} pixels changed)", flush=True)
            for k, v in times.items():
                row[f"{order}: ms {k}"] = round(statistics.median(v), 4)
                row[f"{order}: spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
            row[f"{order}: atomic GB/s"] = round(8 * words / (row[f"{order}: ms splat"] * 1e-3) / 1e9, 2)
            row["inside"], row["changed"] = inside, changed
        print("ROW " + json.dumps(row), flush=True)
    r.set_stars_measurement()
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.frames, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    lines = [f"librpt_hip.so sha256 {hashlib.sha256(open(_ffi.hip_lib_path(), 'rb').read()).hexdigest()}",
             f"method: {SCENE} at {W} x {H}, Doppler shift and beaming on; per round {args.frames} x (colour frame | event frame | outlines | stars); colour, events and outlines",
             f"        between HIP events on the launch stream, splat and resolve between the library's own; {args.rounds} rounds, median (spread = (max - min) / median)", ""]
    rows = []
    for k in range(len(CAMERAS)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--frames", str(args.frames), "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=STEP_TIMEOUT)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print(f"camera {CAMERAS[k][0]} ended with status {p.returncode}: stopping here", flush=True)
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
            else:
                lines.append(line)
    a, b = "spatial order", "caller's order"
    lines += ["", f"{'camera':8s} {'stars':>8s} {'inside':>8s} | {'outlines ms':>11s} | {'splat ms':>9s} {'GB/s':>7s} {'resolve ms':>10s} | {'unsorted splat':>14s} {'GB/s':>7s} {'resolve ms':>10s} | largest spread"]
    for r in rows:
        spread = max(v for k, v in r.items() if ": spread " in k)
        lines.append(f"{r['camera']:8s} {r['stars']:8d} {r['inside']:8d} | {r[a + ': ms outlines']:11.4f} | {r[a + ': ms splat']:9.4f} {r[a + ': atomic GB/s']:7.2f} {r[a + ': ms resolve']:10.4f} | "
                     f"{r[b + ': ms splat']:14.4f} {r[b + ': atomic GB/s']:7.2f} {r[b + ': ms resolve']:10.4f} | {100 * spread:.1f}%")
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
