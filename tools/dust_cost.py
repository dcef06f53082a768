#!/usr/bin/env python3
"""What a shaft of light costs: the lit particles (rpt_set_particle_lighting) at 3840 x 2160 beside the plain particle pass
on the same cloud — device time of the splat between the HIP events the library records around it (rpt_set_particles_measurement):
kernel 1130 (plain), 1134 (lit) and 1135 (lit + shadowed).  The numbers to read are lit / plain and shadowed / lit at equal count, and
the shadowed splat against the colour frame of the same view (rpt_last_frame_ms).

Per scene (shadows.txt: one lamp at 0.95c, a mesh among the occluders; cubes.txt with one lamp added: 35 objects, no mesh), camera (at
rest; gamma = 5 along the view axis) and size (10^4, 10^5, 10^6): particles.dust in a box around the scene, riding an object at rest;
beaming without the shift, so that no grain leaves the visible band.  `--frames` times a colour frame, an event frame and then the three
arms on that frame, their order rotating frame by frame, so the arms alternate inside every round and meet the same machine; an arm's
time is the mean over the frames, the median over `--rounds` rounds and the spread (max - min) / median are reported.

Every (scene, camera) runs in a child process of its own under a time limit, one after the other, and the first failure ends the run:
nothing more is started on the device after a fault, an abort or a timeout.

usage: python tools/dust_cost.py [--frames 10] [--rounds 3] [--out profiles/r24_dust_cost.txt]"""
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
LAMP = "Os\n p-2,3,6,0,0,0,0,0.3,0.3,0.3\n l1\n c8,8,8\n v0.5,0,0\n"
SCENES = {"shadows": dict(t=16.0, host=1, box=((-7.0, -3.4, 4.0), (7.0, 4.0, 14.0))),
          "cubes": dict(t=3.0, host=0, box=((-15.0, -2.0, 1.0), (3.0, 4.0, 18.0)))}
CAMERAS = [("at rest", 0.0), ("gamma 5", math.sqrt(1.0 - 1.0 / 25.0))]
COUNTS = [10 ** 4, 10 ** 5, 10 ** 6]
ARMS = (("plain", dict()), ("lit", dict(lit=True)), ("shadowed", dict(lit=True, shadows=True)))
STEP_TIMEOUT = 280      # seconds per (scene, camera)


def load(name, beta):
    from relativitypathtracer_amd import Scene
    if name == "cubes":
        with open(os.path.join(ROOT, "assets", "reference", "Scenes", "cubes.txt")) as f:
            head, tail = f.read().split("TTextures", 1)
        s = Scene()
        s.inputScene(head + LAMP + "TTextures" + tail)
    else:
        s = Scene.from_file(name)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, beta), SCENES[name]["t"] if beta == 0.0 else 0.0)
    s.update_objects()
    return s


def child(name, index, frames, rounds):
    from relativitypathtracer_amd import particles
    from relativitypathtracer_amd.renderer import Renderer
    label, beta = CAMERAS[index]
    s = load(name, beta)
    r = Renderer(0)
    r.set_doppler(False, True)
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.set_particles_measurement(timed=True)
    names = [a for a, _ in ARMS]
    for n in COUNTS:
        r.set_particles(particles.dust(SCENES[name]["host"], *SCENES[name]["box"], n, (0.8, 0.7, 0.6), 1))
        times = {k: [] for k in names + ["colour frame"]}
        tallies = {}
        for rnd in range(rounds):
            sums = dict.fromkeys(times, 0.0)
            for f in range(-1, frames):                 # frame -1: the warm-up of every arm, not counted
                r.render_async()
                r.render_events(async_=True)
                r.sync()
                if f >= 0:
                    sums["colour frame"] += r.last_frame_ms()
                for k in range(len(ARMS)):
                    arm, lighting = ARMS[(k + max(f, 0)) % len(ARMS)]
                    r.set_particle_lighting(**lighting)
                    r.render_particles()
                    if f >= 0:
                        sums[arm] += r.last_particles_ms()[0]
                    tallies[arm] = r.last_particles() + r.last_particle_lighting()
            for k in times:
                times[k].append(sums[k] / frames)
            print(f"{name:8s} {label:8s} {n:8d}, round {rnd}: " + "  ".join(f"{k} {times[k][-1]:8.4f} ms" for k in times), flush=True)
        row = {"scene": name, "camera": label, "count": n, "seen": tallies["lit"][0], "pairs lit": tallies["shadowed"][2], "pairs shadowed": tallies["shadowed"][3]}
        for k, v in times.items():
            row[f"ms {k}"] = round(statistics.median(v), 4)
            row[f"spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
        for what, (p, q) in (("lit / plain", ("lit", "plain")), ("shadowed / lit", ("shadowed", "lit")), ("shadowed / colour frame", ("shadowed", "colour frame"))):
            ratios = [a / b for a, b in zip(times[p], times[q])]
            row[what] = round(statistics.median(ratios), 3)
            row[f"spread {what}"] = round((max(ratios) - min(ratios)) / statistics.median(ratios), 4)
        print("ROW " + json.dumps(row), flush=True)
    r.set_particles_measurement()
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), args.frames, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    lines = [f"librpt_hip.so sha256 {hashlib.sha256(open(_ffi.hip_lib_path(), 'rb').read()).hexdigest()}",
             f"method: {W} x {H}, beaming on (no shift), particles.dust riding an object at rest; per round {args.frames} x (colour frame | event frame | plain, lit, shadowed,",
             f"        their order rotating frame by frame); each splat between the library's own HIP events; {args.rounds} rounds, median (spread = (max - min) / median); MEASURED", ""]
    rows = []
    for name in SCENES:
        for k in range(len(CAMERAS)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(k), "--frames", str(args.frames), "--rounds", str(args.rounds)],
                               capture_output=True, text=True, timeout=STEP_TIMEOUT)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                print(f"{name}, camera {CAMERAS[k][0]} ended with status {p.returncode}: stopping here", flush=True)
                return 1
            for line in p.stdout.splitlines():
                if line.startswith("ROW "):
                    rows.append(json.loads(line[4:]))
                else:
                    lines.append(line)
    lines += ["", f"{'scene':8s} {'camera':8s} {'count':>8s} {'seen':>8s} {'shadowed':>8s} | {'plain 1130':>10s} {'lit 1134':>9s} {'shadowed 1135':>13s} {'colour frame':>12s} | "
                  f"{'lit/plain':>9s} {'shadowed/lit':>12s} {'shadowed/frame':>14s} | largest spread"]
    for r in rows:
        spread = max(v for k, v in r.items() if k.startswith("spread "))
        lines.append(f"{r['scene']:8s} {r['camera']:8s} {r['count']:8d} {r['seen']:8d} {r['pairs shadowed']:8d} | {r['ms plain']:10.4f} {r['ms lit']:9.4f} {r['ms shadowed']:13.4f} "
                     f"{r['ms colour frame']:12.4f} | {r['lit / plain']:9.3f} {r['shadowed / lit']:12.3f} {r['shadowed / colour frame']:14.3f} | {100 * spread:.1f}%")
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
