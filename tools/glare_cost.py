#!/usr/bin/env python3
"""What glare costs (rpt_set_glare) at 3840 x 2160 on the star-field pass: device time of everything after the splat —
kernels 1170 and 1171 with glare on, kernel 1121 with it off — between the HIP events the library records around them
(rpt_set_stars_measurement; the second figure of rpt_last_stars_ms), for one narrow layer and for three layers with the widest there is,
next to the plain resolve of the same pass on the same frame.  Per camera (at rest; gamma = 5 along the view axis, Doppler shift and
beaming on) and catalogue size (10^4 and 10^6 stars of stars.random_catalogue): `--frames` times a colour frame, an event frame and the
star pass for each of the three arms in turn — plain, narrow, three layers, alternating inside one job, so that whatever drifts on the
device drifts under all three — every pass adding to a fresh picture.  An arm's time is the mean over the frames; the median over
`--rounds` rounds and the spread (max - min) / median are reported, and the ratios to the plain resolve.  The splat's time is reported
beside them: glare does not touch it.  RPT_HIP_LIB names another build of the library to measure instead, e.g. one made with
`make -C relativitypathtracer_amd/csrc EXTRA=-DRPT_GLARE_SKIP=0 OUT=... BUILD=...`, in which no wave and no tile skips its arithmetic:
what the zero skip of the two kernels is worth.

Every camera runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/glare_cost.py [--frames 10] [--rounds 3] [--out profiles/glare_cost.txt]"""
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
COUNTS = [10 ** 4, 10 ** 6]
ARMS = [("plain", None), ("narrow", [(0.4, 0.7)]), ("three", [(0.3, 1.0), (0.2, 4.0), (0.1, 32.0 / 3.0)])]
STEP_TIMEOUT = 420      # seconds per camera


def child(index, frames, rounds):
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
    for n in COUNTS:
        r.set_stars(stars.random_catalogue(n, 1))
        row = {"camera": label, "stars": n}
        times = {arm: {"splat": [], "after": []} for arm, _ in ARMS}
        counts = {}
        for rnd in range(rounds):
            for arm, layers in ARMS:                    # warm-up: every arm once (the planes are reserved here)
                r.set_glare(layers)
                r.render_async()
                r.render_events(async_=True)
                r.render_stars(async_=True)
                r.sync()
            sums = {arm: [0.0, 0.0] for arm, _ in ARMS}
            for _ in range(frames):
                for arm, layers in ARMS:
                    r.set_glare(layers)
                    r.render_async()
                    r.render_events(async_=True)
                    r.render_stars(async_=True)
                    r.sync()
                    splat, after = r.last_stars_ms()
                    sums[arm][0] += splat
                    sums[arm][1] += after
                    counts[arm] = r.last_stars()
            for arm, _ in ARMS:
                times[arm]["splat"].append(sums[arm][0] / frames)
                times[arm]["after"].append(sums[arm][1] / frames)
            print(f"{label:8s} {n:8d} stars round {rnd}: " + "  ".join(f"{arm} splat {times[arm]['splat'][-1]:7.4f} after {times[arm]['after'][-1]:7.4f} ms" for arm, _ in ARMS), flush=True)
        for arm, _ in ARMS:
            for k, v in times[arm].items():
                row[f"{arm}: ms {k}"] = round(statistics.median(v), 4)
                row[f"{arm}: spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
            row[f"{arm}: inside"], row[f"{arm}: changed"] = counts[arm]
        print("ROW " + json.dumps(row), flush=True)
    r.set_glare(None)
    r.set_stars_measurement()
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
             f"method: {SCENE} at {W} x {H}, Doppler shift and beaming on; per round {args.frames} x (colour frame | event frame | stars) for each arm in turn:",
             "        " + "; ".join(f"{arm} = {layers if layers else 'glare off'}" for arm, layers in ARMS),
             f"        splat and after (everything behind the splat) between the library's own HIP events; {args.rounds} rounds, median (spread = (max - min) / median)", ""]
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
    lines += ["", f"{'camera':8s} {'stars':>8s} | {'splat ms':>9s} | {'plain ms':>9s} | {'narrow ms':>9s} {'x plain':>8s} {'changed':>9s} | {'three ms':>9s} {'x plain':>8s} {'changed':>9s} | largest spread"]
    for r in rows:
        spread = max(v for k, v in r.items() if ": spread " in k)
        plain = r["plain: ms after"]
        lines.append(f"{r['camera']:8s} {r['stars']:8d} | {r['plain: ms splat']:9.4f} | {plain:9.4f} | {r['narrow: ms after']:9.4f} {r['narrow: ms after'] / plain:8.1f} {r['narrow: changed']:9d} | "
                     f"{r['three: ms after']:9.4f} {r['three: ms after'] / plain:8.1f} {r['three: changed']:9d} | {100 * spread:.1f}%")
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
