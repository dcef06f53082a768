#!/usr/bin/env python3
"""What adaptive anti-aliasing costs (rpt_set_adaptive_aa) next to the one-sample frame and to rpt_set_msaa(n) of the same library, on the
same contexts, interleaved arm by arm: ms per frame one at a time (rpt_set_objects + the blocking call) and with four contexts in flight
(the async call on four contexts sharing the scene), the method of DESIGN.md section 6: wall clock over `--frames` frames per arm after a
warm-up frame, `--rounds` alternations, the median of the arms and their spread.  The one-sample and MSAA kernels are the parent commit's
machine code, so those columns are baselines outside the code under test.  Configurations: bunny 4K, shadows 4K and arch 1080p with n in
{2, 4} at threshold 8, and one panorama + Doppler + sky view (no MSAA exists there: the one-sample frame and threshold -1).  Prints one
line per arm, then a table with the refined share of pixels and a JSON summary with the library's SHA-256.

Every configuration runs in a child process of its own under a time limit, one after the other, and the first failure ends the run:
nothing more is started on the device after a fault, an abort or a timeout.

usage: python tools/aa_cost.py [--frames 200] [--rounds 3] [--out profiles/r10_adaptive_aa_cost.txt]"""
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

#          scene     t      W     H     n  T   panorama + Doppler + sky
CONFIGS = [("bunny", 0.0, 3840, 2160, 2, 8, False), ("bunny", 0.0, 3840, 2160, 4, 8, False),
           ("shadows", 16.0, 3840, 2160, 2, 8, False), ("shadows", 16.0, 3840, 2160, 4, 8, False),
           ("arch", 5.25, 1920, 1080, 2, 8, False), ("arch", 5.25, 1920, 1080, 4, 8, False),
           ("arch", 5.25, 3840, 1920, 2, -1, True), ("arch", 5.25, 3840, 1920, 2, 8, True)]
CAMERA_V = {"bunny": (0.0, 0.0, 0.0), "shadows": (0.0, 0.0, 0.0), "arch": (0.0, 0.0, 0.95)}      # the benchmark's own states
IN_FLIGHT = 4
STEP_TIMEOUT = 300      # seconds per configuration


def one_at_a_time(r, s, frames):
    t0 = time.perf_counter()
    for _ in range(frames):
        r.set_objects(s)
        r.render()
    return (time.perf_counter() - t0) / frames * 1e3


def in_flight(slots, s, frames):
    t0 = time.perf_counter()
    for f in range(frames * len(slots)):
        r = slots[f % len(slots)]
        r.sync()
        r.set_objects(s)
        r.render_async()
    for r in slots:
        r.sync()
    return (time.perf_counter() - t0) / (frames * len(slots)) * 1e3


def child(index, frames, rounds):
    import numpy as np
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    name, t, W, H, n, T, pano = CONFIGS[index]
    s = Scene.from_file(name)
    s.set_camera(CAMERA_V[name], t)
    s.update_objects()
    slots = [Renderer(0) for _ in range(IN_FLIGHT)]
    slots[0].upload_scene(s)
    for r in slots[1:]:
        r.share_scene(slots[0])
    if pano:
        y, x = np.mgrid[0:512, 0:1024]
        sky = np.ascontiguousarray(np.stack([(x * 255) // 1023, (y * 255) // 511, ((x ^ y) & 255)], -1).astype(np.uint8))
    for r in slots:
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.set_objects(s)
        if pano:
            r.set_projection("equirect")
            r.set_doppler(True, True)
            r.set_environment(sky)
            r.set_environment_frame(s.camera_lorentz()[1])
    arms = ("one-sample", "adaptive") if pano else ("one-sample", "msaa", "adaptive")

    def select(arm):
        for r in slots:
            r.set_msaa(n if arm == "msaa" else 1)
            r.set_adaptive_aa(n if arm == "adaptive" else 1, T)

    res = {arm: {"one": [], "flight": []} for arm in arms}
    kernels, refined = {}, 0
    for rnd in range(rounds):
        for arm in arms:
            select(arm)
            for r in slots:                      # warm-up frame of this arm
                r.render()
            one = one_at_a_time(slots[0], s, frames)
            kb = (slots[0].last_variant(), slots[0].last_aa_variant())
            fl = in_flight(slots, s, frames)
            kf = (slots[0].last_variant(), slots[0].last_aa_variant())
            kernels[arm] = [kb, kf]
            if arm == "adaptive":
                refined = slots[0].last_aa_refined()
            res[arm]["one"].append(one)
            res[arm]["flight"].append(fl)
            print(f"{name:8s} {W}x{H} n {n} T {T:3d} round {rnd} {arm:10s}: one at a time {one:8.4f} ms (kernels {kb})   {IN_FLIGHT} in flight {fl:8.4f} ms/frame (kernels {kf})", flush=True)
    row = {"scene": name + (" panorama+doppler+sky" if pano else ""), "size": [W, H], "n": n, "T": T, "kernels": kernels,
           "refined": refined, "refined_share": round(refined / (W * H), 4)}
    for mode in ("one", "flight"):
        for arm in arms:
            v = res[arm][mode]
            row[f"ms_{mode}_{arm}"] = round(statistics.median(v), 4)
            row[f"spread_{mode}_{arm}"] = round((max(v) - min(v)) / statistics.median(v), 4)
    for r in slots:
        r.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the arms per configuration")
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--only", default="", help="comma-separated configuration indices (default: all)")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.frames, args.rounds)
        return 0
    from relativitypathtracer_amd import _ffi
    lines = [f"librpt_hip.so sha256 {hashlib.sha256(open(_ffi.hip_lib_path(), 'rb').read()).hexdigest()}",
             f"method: wall clock over {args.frames} frames per arm after a warm-up frame, {args.rounds} alternations of the arms, median of the arms (spread = (max - min) / median);",
             f"        one at a time = rpt_set_objects + the blocking call on one context; in flight = the async call on {IN_FLIGHT} contexts sharing the scene", ""]
    rows = []
    todo = [int(k) for k in args.only.split(",")] if args.only else range(len(CONFIGS))
    for k in todo:
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
    lines += ["", f"{'scene':30s} {'size':>10s} {'n':>2s} {'T':>3s} {'refined':>8s} | {'1-sample':>9s} {'msaa(n)':>9s} {'adaptive':>9s} | {'1-smp x4':>9s} {'msaa x4':>9s} {'adapt x4':>9s} | largest spread"]
    for r in rows:
        g = lambda k: f"{r[k]:9.4f}" if k in r else f"{'-':>9s}"
        spread = max(v for k, v in r.items() if k.startswith("spread_"))
        lines.append(f"{r['scene']:30s} {r['size'][0]:>5d}x{r['size'][1]:<4d} {r['n']:2d} {r['T']:3d} {100 * r['refined_share']:7.2f}% | "
                     f"{g('ms_one_one-sample')} {g('ms_one_msaa')} {g('ms_one_adaptive')} | {g('ms_flight_one-sample')} {g('ms_flight_msaa')} {g('ms_flight_adaptive')} | {100 * spread:.1f}%")
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
