#!/usr/bin/env python3
"""What the rocket pass costs (rpt_render_rockets) at 3840 x 2160 beside the ballistic pass with as many sources: device
time of each pass's two kernels — the splat (1160 / 1150) and the resolve (1131 for both) — between HIP events the library records around
them (rpt_set_rockets_measurement, rpt_set_ballistics_measurement).  The number to read is the rocket splat's time over the ballistic
splat's at equal count: per source the splat reads 64 bytes for 48 and adds two square roots and some ten divisions.

Per camera (at rest; gamma = 5 along the view axis) and size (10^4, 10^5, 10^6), tools/ballistics_cost.py's lamps that fly apart at up to
0.9 c, two ways on the rocket side: the ballistic records as rockets with acc = 0 (rockets.from_ballistics: the same worldlines, the same
pixels: "coasting"); and the same records under proper accelerations of up to 0.05 in random directions ("thrust").  Beaming without the
shift, so that no source leaves the visible band.  `--frames` times a colour frame, an event frame and then the ballistic pass and one
rocket set on that frame, the ballistic records first on even frames and the rockets first on odd ones, so the two arms alternate inside
every round and meet the same machine; an arm's time is the mean over the frames, the median over `--rounds` rounds and the spread
(max - min) / median are reported.

Every camera runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/rockets_cost.py [--frames 10] [--rounds 3] [--out profiles/rockets_cost.txt]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ballistics_cost import ballistic_sets      # noqa: E402
from particles_cost import CAMERAS, COUNTS, H, SCENE, SCENE_T, STEP_TIMEOUT, W, riding_lattice      # noqa: E402


def rocket_sets(bs):
    """(the ballistic set coasting, the same records under thrust): ROCKET_DTYPE records in the order of bs."""
    import numpy as np
    from relativitypathtracer_amd import rockets
    coasting = rockets.from_ballistics(bs)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(len(bs), 3))
    thrust = coasting.copy()
    thrust["acc"] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.05, (len(bs), 1))
    return coasting, thrust


def child(index, frames, rounds):
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    label, beta = CAMERAS[index]
    s = Scene.from_file(SCENE)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, beta), SCENE_T if beta == 0.0 else 0.0)
    s.update_objects()
    r = Renderer(0)
    r.set_doppler(False, True)      # beaming alone: with the shift most lamps of the fast cubes leave the visible band and add nothing
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.set_ballistics_measurement(timed=True)
    r.set_rockets_measurement(timed=True)
    r.set_ballistic_options(inverse_square=True)
    r.set_rocket_options(inverse_square=True)
    arms = ("ballistics splat", "ballistics resolve", "rockets splat", "rockets resolve")
    for n in COUNTS:
        ps, riders = riding_lattice(s, n)
        _, bs = ballistic_sets(s, ps)
        r.set_ballistics(bs)
        for what, rs in zip(("coasting", "thrust"), rocket_sets(bs)):
            r.set_rockets(rs)
            times = {k: [] for k in arms}
            for rnd in range(rounds):
                r.render_async()                            # warm-up of the four passes
                r.render_events(async_=True)
                r.render_ballistics(async_=True)
                r.render_rockets(async_=True)
                r.sync()
                sums = dict.fromkeys(arms, 0.0)
                for f in range(frames):
                    r.render_async()
                    r.render_events(async_=True)
                    for which in ((0, 1) if f % 2 == 0 else (1, 0)):
                        (r.render_ballistics if which == 0 else r.render_rockets)(async_=True)
                    r.sync()
                    for k, v in zip(arms, r.last_ballistics_ms() + r.last_rockets_ms()):
                        sums[k] += v
                for k in arms:
                    times[k].append(sums[k] / frames)
                seen_b, _ = r.last_ballistics()
                seen, changed = r.last_rockets()
                print(f"{label:8s} {n:8d} {what:8s}, round {rnd}: ballistics splat {times[arms[0]][-1]:7.4f} ms  resolve {times[arms[1]][-1]:7.4f}   rockets splat "
                      f"{times[arms[2]][-1]:7.4f}  resolve {times[arms[3]][-1]:7.4f}   ({seen_b} ballistic records seen, {seen} rockets seen on {riders} objects, {changed} pixels changed)", flush=True)
            row = {"camera": label, "count": n, "set": what, "ballistics seen": seen_b, "rockets seen": seen, "pixels changed": changed}
            for k, v in times.items():
                row[f"ms {k}"] = round(statistics.median(v), 4)
                row[f"spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
            ratios = [p / q for p, q in zip(times["rockets splat"], times["ballistics splat"])]
            row["splat ratio"] = round(statistics.median(ratios), 3)
            row["splat ratio spread"] = round((max(ratios) - min(ratios)) / statistics.median(ratios), 4)
            print("ROW " + json.dumps(row), flush=True)
    r.set_ballistics_measurement()
    r.set_rockets_measurement()
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
             f"method: {SCENE} at {W} x {H}, beaming on (no shift: every source adds), inverse square on; per round {args.frames} x (colour frame | event frame | ballistics and",
             f"        rockets, their order alternating frame by frame); each kernel between the library's own HIP events; {args.rounds} rounds, median (spread = (max - min) / median)",
             "        coasting: the ballistic records with acc = 0 (kernel 1160 against 1150 on the same worldlines); thrust: the same records under |acc| up to 0.05", ""]
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
    lines += ["", f"{'camera':8s} {'count':>8s} {'set':8s} {'seen':>8s} | {'ballistics splat':>16s} {'resolve':>8s} | {'rockets splat':>13s} {'resolve':>8s} | {'splat ratio':>11s} {'its spread':>10s} | largest spread of a time"]
    for r in rows:
        spread = max(v for k, v in r.items() if k.startswith("spread "))
        lines.append(f"{r['camera']:8s} {r['count']:8d} {r['set']:8s} {r['rockets seen']:8d} | {r['ms ballistics splat']:16.4f} {r['ms ballistics resolve']:8.4f} | "
                     f"{r['ms rockets splat']:13.4f} {r['ms rockets resolve']:8.4f} | {r['splat ratio']:11.3f} {100 * r['splat ratio spread']:9.1f}% | {100 * spread:.1f}%")
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
