#!/usr/bin/env python3
"""What the segment pass costs (rpt_render_segments) at 3840 x 2160, and which of its two splat kernels is the faster:
the pooled one (1140: a wave shares the steps of its 64 pieces) or the plain loop per lane (the diag library's arm, rpt_set_variant
1141).  Both come from ONE library, librpt_hip_diag.so, on ONE context, and alternate pass by pass inside every round, so they meet the
same machine; device time between HIP events the library records around the kernels (rpt_set_segments_measurement).  Beside them, in the
same rounds, what a user had to do before the pass existed: the particle pass (kernel 1130) fed segments.as_particles with as many lamps
as the segment pass takes samples (the float64 model's count; at most 2^22, the particle pass's limit — the table says where that cut).

Per camera (at rest; gamma = 5 along the view axis), load (count x pieces about 10^4, 10^5, 10^6) and pieces (1, 16, 64): a
segments.rod_lattice riding every moving cube of cubes.txt, 3 units across, the set shuffled and cut to count rods; beaming without the
shift, the inverse square on.  Per round one colour frame and one event frame, then `--passes` times the three arms in rotating order
(a pass adds to the frame it finds; the splat's work does not depend on what the bytes hold).  An arm's time is the mean over the
passes; the median over `--rounds` rounds and the spread (max - min) / median are reported.  A cell's verdict: the arm whose median
is lower by more than the larger of the two spreads, else `tie`.

Every camera runs in a child process of its own under a time limit, one after the other, and the first failure ends the run: nothing
more is started on the device after a fault, an abort or a timeout.

usage: python tools/segments_cost.py [--passes 6] [--rounds 3] [--out profiles/segments_cost.txt]"""
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
LOADS = [10 ** 4, 10 ** 5, 10 ** 6]
PIECES = [1, 16, 64]
LOOP_ARM = 1141
MAX_LAMPS = 1 << 22
STEP_TIMEOUT = 500      # seconds per camera


def riding_lattice(scene, count):
    """count rods in all: a rod_lattice of the same size around the rest-frame centre of every moving cube of the scene (every cube, if
    none moves), 3 units across, shuffled and truncated to count."""
    import numpy as np
    from relativitypathtracer_amd import segments
    objs = scene.objects()
    cubes = [i for i in range(len(objs)) if objs["type"][i] == 1]
    identity = np.eye(4, dtype=np.float32)
    moving = [i for i in cubes if not np.allclose(objs["Lorentz"][i][1:, 1:], identity[1:, 1:], atol=1e-6)] or cubes
    cells = 1
    while 3 * cells * (cells + 1) ** 2 * len(moving) < count:
        cells += 1
    sets = []
    for i in moving:
        centre = objs["M"][i][:3, 3].astype(np.float64)
        sets.append(segments.rod_lattice(i, centre - 1.5, centre + 1.5, cells, (0.8, 0.7, 0.5)))
    rods = np.concatenate(sets)
    assert len(rods) >= count
    return np.ascontiguousarray(rods[np.random.default_rng(1).permutation(len(rods))[:count]]), len(moving)


def child(index, passes, rounds):
    import numpy as np
    from relativitypathtracer_amd import Scene, segments
    from relativitypathtracer_amd.renderer import Renderer
    label, beta = CAMERAS[index]
    s = Scene.from_file(SCENE)
    s.set_interval(-1)
    s.set_camera((0.0, 0.0, beta), SCENE_T if beta == 0.0 else 0.0)
    s.update_objects()
    r = Renderer(0, diag=True)
    r.set_doppler(False, True)      # beaming alone: with the shift most of the fast cubes' light leaves the visible band and adds nothing
    r.upload_scene(s)
    r.set_scene_params(s, W, H)
    r.set_output(None)
    r.set_segments_measurement(timed=True)
    r.set_particles_measurement(timed=True)
    r.set_particle_options(inverse_square=True)
    arms = ("pooled splat", "loop splat", "segment resolve", "lamp splat", "lamp resolve")
    for load in LOADS:
        for pieces in PIECES:
            rods, riders = riding_lattice(s, load // pieces)
            model = segments.project(rods, s, dict(mode="pinhole"), W, H, -1, 2, dict(inverse_square=True, pieces=pieces))
            samples = int(model["m"].sum())
            per_rod = np.maximum(1, model["m"].sum(axis=1))
            if per_rod.sum() > MAX_LAMPS:       # the particle pass takes no more: thin every rod's lamps alike, one at least
                per_rod = 1 + ((per_rod - 1) * ((MAX_LAMPS - len(rods)) / (per_rod.sum() - len(rods)))).astype(np.int64)
            lamps = segments.as_particles(rods, per_rod)
            r.set_segments(None)
            r.set_segment_options(inverse_square=True, pieces=pieces)
            r.set_segments(rods)
            r.set_particles(lamps)
            times = {k: [] for k in arms}

            def run(which):
                if which == 2:
                    r.render_particles()
                    return dict(zip(("lamp splat", "lamp resolve"), r.last_particles_ms()))
                r.set_variant(LOOP_ARM if which == 1 else 0)
                try:
                    r.render_segments()
                finally:
                    r.set_variant(0)
                splat, resolve = r.last_segments_ms()
                return {"loop splat" if which == 1 else "pooled splat": splat, "segment resolve": resolve}

            for rnd in range(rounds):
                r.render_async()
                r.render_events(async_=True)
                r.sync()
                for which in (0, 1, 2):                 # warm-up of the three arms
                    run(which)
                sums, shots = dict.fromkeys(arms, 0.0), dict.fromkeys(arms, 0)
                for f in range(passes):
                    for which in ((0, 1, 2), (1, 2, 0), (2, 0, 1))[f % 3]:
                        for k, v in run(which).items():
                            sums[k] += v
                            shots[k] += 1
                for k in arms:
                    times[k].append(sums[k] / shots[k])
                r.set_variant(0)
                r.render_segments()
                drawn, changed = r.last_segments()
                print(f"{label:8s} load {load:8d} pieces {pieces:2d}, round {rnd}: pooled {times[arms[0]][-1]:8.4f} ms  loop {times[arms[1]][-1]:8.4f}  resolve {times[arms[2]][-1]:7.4f}   "
                      f"lamps {times[arms[3]][-1]:8.4f}  resolve {times[arms[4]][-1]:7.4f}   ({len(rods)} rods on {riders} objects, {samples} samples, {drawn} pieces drawn, "
                      f"{len(lamps)} lamps)", flush=True)
            row = {"camera": label, "load": load, "pieces": pieces, "rods": len(rods), "samples": samples, "pieces drawn": drawn, "pixels changed": changed, "lamps": len(lamps)}
            for k, v in times.items():
                row[f"ms {k}"] = round(statistics.median(v), 4)
                row[f"spread {k}"] = round((max(v) - min(v)) / statistics.median(v), 4)
            print("ROW " + json.dumps(row), flush=True)
    r.set_segments_measurement()
    r.set_particles_measurement()
    r.close()


def verdict(row):
    pooled, loop = row["ms pooled splat"], row["ms loop splat"]
    spread = max(row["spread pooled splat"], row["spread loop splat"])
    if pooled < loop * (1.0 - spread):
        return "pooled"
    if loop < pooled * (1.0 - spread):
        return "loop"
    return "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.passes, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    diag = _ffi._path("librpt_hip_diag.so")
    lines = [f"librpt_hip_diag.so sha256 {hashlib.sha256(open(diag, 'rb').read()).hexdigest()}",
             f"method: {SCENE} at {W} x {H}, beaming on (no shift), inverse square on; per round one colour frame and one event frame, then {args.passes} x (pooled splat 1140 |",
             f"        loop splat, variant {LOOP_ARM} | particle pass on as_particles), their order rotating pass by pass; each kernel between the library's own HIP events;",
             f"        {args.rounds} rounds, median (spread = (max - min) / median)", ""]
    rows = []
    for k in range(len(CAMERAS)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--passes", str(args.passes), "--rounds", str(args.rounds)],
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
    lines += ["", f"{'camera':8s} {'load':>8s} {'P':>2s} {'samples':>9s} {'drawn':>8s} | {'pooled':>8s} {'loop':>8s} {'loop/pooled':>11s} {'verdict':>7s} | {'resolve':>7s} | {'lamps':>8s} {'lamp splat':>10s} "
              f"{'lamps/pooled':>12s} | largest spread of a splat"]
    for r in rows:
        spread = max(r[f"spread {k}"] for k in ("pooled splat", "loop splat", "lamp splat"))
        lines.append(f"{r['camera']:8s} {r['load']:8d} {r['pieces']:2d} {r['samples']:9d} {r['pieces drawn']:8d} | {r['ms pooled splat']:8.4f} {r['ms loop splat']:8.4f} "
                     f"{r['ms loop splat'] / r['ms pooled splat']:11.2f} {verdict(r):>7s} | {r['ms segment resolve']:7.4f} | {r['lamps']:8d} {r['ms lamp splat']:10.4f} "
                     f"{r['ms lamp splat'] / r['ms pooled splat']:12.2f} | {100 * spread:.1f}%")
    tally = {v: sum(verdict(r) == v for r in rows) for v in ("pooled", "loop", "tie")}
    lines += ["", f"cells: pooled faster in {tally['pooled']}, loop faster in {tally['loop']}, within the spread in {tally['tie']} of {len(rows)}", "", json.dumps(rows)]
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
