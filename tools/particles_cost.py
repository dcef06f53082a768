#!/usr/bin/env python3
"""What the particle pass costs (rpt_render_particles) at 3840 x 2160 beside the star-field pass with as many stars:
device time of each pass's two kernels — the splat (1130 / 1120) and the resolve (1131 / 1121) — between HIP events the library records
around them (rpt_set_particles_measurement, rpt_set_stars_measurement).  The number to read is the particle splat's time over the star
splat's at equal count: per particle the splat adds an 80-byte object fetch and up to four 8-byte record reads to what a star costs.

Per camera (at rest; gamma = 5 along the view axis) and size (10^4, 10^5, 10^6): a particles.lattice of lamps riding every moving
cube of cubes.txt, and stars.random_catalogue of the same size; beaming without the shift, so that no source leaves the visible band
and every one inside the frame issues its atomics.  `--frames` times a colour frame, an event frame and then BOTH passes on
that frame, the stars first on even frames and the particles first on odd ones, so the two arms alternate inside every round and meet
the same machine; an arm's time is the mean over the frames, the median over `--rounds` rounds and the spread (max - min) / median are
reported.

Every camera runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/particles_cost.py [--frames 20] [--rounds 3] [--out profiles/particles_cost.txt]"""
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


def riding_lattice(scene, n):
    """n lamps in all: a cubic lattice of the same size around the rest-frame centre of every moving cube of the scene (every cube,
    if none moves), 3 units across, truncated to n."""
    import numpy as np
    from relativitypathtracer_amd import particles
    objs = scene.objects()
    cubes = [i for i in range(len(objs)) if objs["type"][i] == 1]
    identity = np.eye(4, dtype=np.float32)
    moving = [i for i in cubes if not np.allclose(objs["Lorentz"][i][1:, 1:], identity[1:, 1:], atol=1e-6)] or cubes
    per_axis = max(2, math.ceil((n / len(moving)) ** (1.0 / 3.0)))
    sets = []
    for i in moving:
        centre = objs["M"][i][:3, 3].astype(np.float64)
        sets.append(particles.lattice(i, centre - 1.5, centre + 1.5, per_axis, (0.8, 0.7, 0.5)))
    ps = np.concatenate(sets)
    assert len(ps) >= n
    return np.ascontiguousarray(ps[np.random.default_rng(1).permutation(len(ps))[:n]]), len(moving)


def child(index, frames, rounds):
    from relativitypathtracer_amd import Scene, stars
    from relativitypathtracer_amd.renderer import Renderer
    label, beta = CAMERAS[index]
    s = Scene.from_file(SCENE)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, beta), SCENE_T if beta == 0.0 else 0.0)
    s.update_objects()
    r = Renderer(0)
    r.set_doppler(False, True)      # beaming alone: with the shift most lamps of the fast cubes leave the visible band and add nothing
    r.set_environment_frame(s.camera_lorentz()[1])
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.set_stars_measurement(timed=True)
    r.set_particles_measurement(timed=True)
    r.set_particle_options(inverse_square=True)
    arms = ("stars splat", "stars resolve", "particles splat", "particles resolve")
    for n in COUNTS:
        ps, riders = riding_lattice(s, n)
        r.set_stars(stars.random_catalogue(n, 1))
        r.set_particles(ps)
        times = {k: [] for k in arms}
        for rnd in range(rounds):
            r.render_async()                            # warm-up of the four passes
            r.render_events(async_=True)
            r.render_stars(async_=True)
            r.render_particles(async_=True)
            r.sync()
            sums = dict.fromkeys(arms, 0.0)
            for f in range(frames):
                r.render_async()
                r.render_events(async_=True)
                for which in ((0, 1) if f % 2 == 0 else (1, 0)):
                    (r.render_stars if which == 0 else r.render_particles)(async_=True)
                r.sync()
                for k, v in zip(arms, r.last_stars_ms() + r.last_particles_ms()):
                    sums[k] += v
            for k in arms:
                times[k].append(sums[k] / frames)
            inside, _ = r.last_stars()
            seen, changed = r.last_particles()
            print(f"{label:8s} {n:8d}, round {rnd}: stars splat {times[arms[0]][-1]:7.4f} ms  resolve {times[arms[1]][-1]:7.4f}   particles splat {times[arms[2]][-1]:7.4f}  "
                  f"resolve {times[arms[3]][-1]:7.4f}   ({inside} stars inside; {seen} particles seen on {riders} objects, {changed} pixels changed)", flush=True)
        row = {"camera": label, "count": n, "stars inside": inside, "particles seen": seen, "pixels changed": changed}
        for k, v in times.items():
            row[f"ms {k}"] = round(statistics.median(v), 4)
            row[f"spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
        ratios = [p / q for p, q in zip(times["particles splat"], times["stars splat"])]
        row["splat ratio"] = round(statistics.median(ratios), 3)
        row["splat ratio spread"] = round((max(ratios) - min(ratios)) / statistics.median(ratios), 4)
        print("ROW " + json.dumps(row), flush=True)
    r.set_stars_measurement()
    r.set_particles_measurement()
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
             f"method: {SCENE} at {W} x {H}, beaming on (no shift: every lamp and star adds), inverse square on; per round {args.frames} x (colour frame | event frame | stars and particles,",
             f"        their order alternating frame by frame); each kernel between the library's own HIP events; {args.rounds} rounds, median (spread = (max - min) / median)", ""]
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
    lines += ["", f"{'camera':8s} {'count':>8s} {'seen':>8s} | {'stars splat':>11s} {'resolve':>8s} | {'particles splat':>15s} {'resolve':>8s} | {'splat ratio':>11s} {'its spread':>10s} | largest spread of a time"]
    for r in rows:
        spread = max(v for k, v in r.items() if k.startswith("spread "))
        lines.append(f"{r['camera']:8s} {r['count']:8d} {r['particles seen']:8d} | {r['ms stars splat']:11.4f} {r['ms stars resolve']:8.4f} | {r['ms particles splat']:15.4f} "
                     f"{r['ms particles resolve']:8.4f} | {r['splat ratio']:11.3f} {100 * r['splat ratio spread']:9.1f}% | {100 * spread:.1f}%")
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
