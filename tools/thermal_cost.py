#!/usr/bin/env python3
"""What the thermal colour rule costs (rpt_set_star_temperatures / rpt_set_particle_temperatures) at 3840 x 2160: device
time of the thermal splat (kernels 1122 / 1132) beside the plain splat (1120 / 1130) of the same catalogue and the same set, between the
HIP events the library records around them (rpt_set_stars_measurement, rpt_set_particles_measurement).  The resolves (1121 / 1131) are
shared and reported once per arm.

Per camera (at rest; gamma = 5 along the view axis) and size (10^4, 10^5, 10^6): stars.random_catalogue with its temperatures, and the
lamps of tools/particles_cost.py riding every moving cube of cubes.txt with temperatures of 3000 - 12000 K; shift and beaming on (the
thermal law acts under the shift only).  `--frames` times a colour frame, an event frame and then each pass TWICE on that frame, once
with the temperatures set and once without, the thermal arm first on even frames and the plain arm first on odd ones, so the two arms
alternate inside every round and meet the same machine; an arm's time is the mean over the frames, the median over `--rounds` rounds and
the spread (max - min) / median are reported.  No threshold: the figure to read is the thermal splat's time over the plain splat's.

The arms do not issue the same atomics where sources move: under the shift S_f blacks out every source beyond its outer knots (at gamma =
5 the whole forward patch), and a black source adds nothing, while the thermal law keeps it lit.  At rest (D == 1 for the stars) both
arms return the colour untouched and the difference is the extra load and the branch.  The counts printed beside the times say which.

Every camera runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/thermal_cost.py [--frames 10] [--rounds 3] [--out profiles/r22_thermal_cost.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H = 3840, 2160
SCENE, SCENE_T = "cubes", 3.0
CAMERAS = [("at rest", 0.0), ("gamma 5", math.sqrt(1.0 - 1.0 / 25.0))]
COUNTS = [10 ** 4, 10 ** 5, 10 ** 6]
STEP_TIMEOUT = 420      # seconds per camera
ARMS = ("stars thermal", "stars plain", "particles thermal", "particles plain")


def child(index, frames, rounds):
    import numpy as np
    from particles_cost import riding_lattice
    from relativitypathtracer_amd import Scene, stars
    from relativitypathtracer_amd.renderer import Renderer
    label, beta = CAMERAS[index]
    s = Scene.from_file(SCENE)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, beta), SCENE_T if beta == 0.0 else 0.0)
    s.update_objects()
    r = Renderer(0)
    r.set_doppler(True, True)
    r.set_environment_frame(s.camera_lorentz()[1])
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.set_stars_measurement(timed=True)
    r.set_particles_measurement(timed=True)
    r.set_particle_options(inverse_square=True)
    for n in COUNTS:
        cat, star_T = stars.random_catalogue(n, 1, return_temperatures=True)
        ps, riders = riding_lattice(s, n)
        lamp_T = np.exp(np.random.default_rng(2).uniform(math.log(3000.0), math.log(12000.0), n)).astype(np.float32)
        ps["rgb"] = stars.blackbody_rgb(lamp_T) * 0.8
        r.set_stars(cat)
        r.set_particles(ps)

        def passes(thermal):
            """Both passes on the current frame, with or without temperatures: ((splat, resolve) of the stars, of the particles, counts)."""
            r.set_star_temperatures(star_T if thermal else None)
            r.set_particle_temperatures(lamp_T if thermal else None)
            r.render_stars(async_=True)
            r.render_particles(async_=True)
            r.sync()
            return r.last_stars_ms(), r.last_particles_ms(), r.last_stars() + r.last_particles()

        splat = {k: [] for k in ARMS}
        resolve = {k: [] for k in ARMS}
        counts = {}
        for rnd in range(rounds):
            r.render_async()                            # warm-up of both arms
            r.render_events(async_=True)
            passes(True)
            passes(False)
            sums, sums_resolve = dict.fromkeys(ARMS, 0.0), dict.fromkeys(ARMS, 0.0)
            for f in range(frames):
                r.render_async()
                r.render_events(async_=True)
                for thermal in ((True, False) if f % 2 == 0 else (False, True)):
                    star_ms, lamp_ms, c = passes(thermal)
                    arm = "thermal" if thermal else "plain"
                    counts[arm] = c
                    sums[f"stars {arm}"] += star_ms[0]
                    sums[f"particles {arm}"] += lamp_ms[0]
                    sums_resolve[f"stars {arm}"] += star_ms[1]
                    sums_resolve[f"particles {arm}"] += lamp_ms[1]
            for k in ARMS:
                splat[k].append(sums[k] / frames)
                resolve[k].append(sums_resolve[k] / frames)
            print(f"{label:8s} {n:8d}, round {rnd}: stars splat thermal {splat[ARMS[0]][-1]:7.4f} ms  plain {splat[ARMS[1]][-1]:7.4f}   particles splat thermal "
                  f"{splat[ARMS[2]][-1]:7.4f}  plain {splat[ARMS[3]][-1]:7.4f}   (pixels changed: stars {counts['thermal'][1]} / {counts['plain'][1]}, "
                  f"particles {counts['thermal'][3]} / {counts['plain'][3]}; {riders} objects carry lamps)", flush=True)
        row = {"camera": label, "count": n, "stars inside": counts["thermal"][0], "particles seen": counts["thermal"][2],
               "star pixels changed thermal": counts["thermal"][1], "star pixels changed plain": counts["plain"][1],
               "particle pixels changed thermal": counts["thermal"][3], "particle pixels changed plain": counts["plain"][3]}
        for k in ARMS:
            row[f"ms splat {k}"] = round(statistics.median(splat[k]), 4)
            row[f"spread splat {k}"] = round((max(splat[k]) - min(splat[k])) / statistics.median(splat[k]), 4)
            row[f"ms resolve {k}"] = round(statistics.median(resolve[k]), 4)
        for what in ("stars", "particles"):
            ratios = [p / q for p, q in zip(splat[f"{what} thermal"], splat[f"{what} plain"])]
            row[f"{what} ratio"] = round(statistics.median(ratios), 3)
            row[f"{what} ratio spread"] = round((max(ratios) - min(ratios)) / statistics.median(ratios), 4)
        print("ROW " + json.dumps(row), flush=True)
    r.set_stars_measurement()
    r.set_particles_measurement()
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.frames, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    lines = [f"librpt_hip.so sha256 {hashlib.sha256(open(_ffi.hip_lib_path(), 'rb').read()).hexdigest()}",
             f"method: {SCENE} at {W} x {H}, shift and beaming on, inverse square on; per round {args.frames} x (colour frame | event frame | stars and particles with",
             f"        temperatures | the same without; the two arms' order alternating frame by frame); each kernel between the library's own HIP events;",
             f"        {args.rounds} rounds, median (spread = (max - min) / median).  Under the shift the plain arm's sources beyond S_f's knots are black and add nothing.", ""]
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
    for what, first in (("stars", "stars inside"), ("particles", "particles seen")):
        lines += ["", f"{what}:", f"{'camera':8s} {'count':>8s} {first.split()[1]:>8s} | {'thermal splat':>13s} {'plain splat':>11s} | {'ratio':>6s} {'its spread':>10s} | "
                                  f"{'resolve th.':>11s} {'plain':>7s} | {'pixels changed th.':>18s} {'plain':>8s} | largest spread of a splat"]
        one = what[:-1] if what == "stars" else "particle"
        for r in rows:
            spread = max(r[f"spread splat {what} thermal"], r[f"spread splat {what} plain"])
            lines.append(f"{r['camera']:8s} {r['count']:8d} {r[first]:8d} | {r[f'ms splat {what} thermal']:13.4f} {r[f'ms splat {what} plain']:11.4f} | {r[f'{what} ratio']:6.3f} "
                         f"{100 * r[f'{what} ratio spread']:9.1f}% | {r[f'ms resolve {what} thermal']:11.4f} {r[f'ms resolve {what} plain']:7.4f} | "
                         f"{r[f'{one} pixels changed thermal']:18d} {r[f'{one} pixels changed plain']:8d} | {100 * spread:.1f}%")
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
