#!/usr/bin/env python3
"""A/B/A/B of rpt_set_doppler: Doppler off (the reference's kernels) against on (shift + beaming, the twins) on the same contexts,
ms/frame one frame at a time (rpt_set_objects + rpt_render) and with three frames in flight (rpt_render_async), as tools/configs.py
measures them.  Prints one line per arm and a JSON summary (median of the arms per mode).
usage: python tools/doppler_ab.py [--frames 40] [--rounds 2]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relativitypathtracer_amd import Scene                      # noqa: E402
from relativitypathtracer_amd.renderer import Renderer          # noqa: E402

CONFIGS = [("bunny", 3840, 2160, (0, 0, 0), 0.0), ("shadows", 3840, 2160, (0, 0, 0), 16.0), ("arch", 1920, 1080, (0, 0, 0.95), 5.25),
           ("cubes", 3840, 2160, (0.3, 0, 0.1), 3.0)]


def one_at_a_time(slots, s, frames):
    t0 = time.perf_counter()
    for _ in range(frames):
        slots[0].set_objects(s)
        slots[0].render()
    return (time.perf_counter() - t0) / frames * 1e3


def in_flight(slots, s, frames):
    t0 = time.perf_counter()
    for f in range(frames * 3):
        r = slots[f % len(slots)]
        r.sync()
        r.set_objects(s)
        r.render_async()
    for r in slots:
        r.sync()
    return (time.perf_counter() - t0) / (frames * 3) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2, help="A/B pairs per configuration")
    args = ap.parse_args()
    rows = []
    for name, W, H, vel, t in CONFIGS:
        s = Scene.from_file(name)
        s.set_camera(vel, t)
        s.update_objects()
        slots = [Renderer(0) for _ in range(3)]
        slots[0].upload_scene(s)
        for r in slots[1:]:
            r.share_scene(slots[0])
        for r in slots:
            r.set_scene_params(s, W, H)
            r.set_output(None)
        res = {"off": {"one": [], "flight": []}, "on": {"one": [], "flight": []}}
        kernels = {}
        for rnd in range(args.rounds):
            for arm in ("off", "on"):
                for r in slots:
                    r.set_doppler(arm == "on", arm == "on")
                    r.set_objects(s)
                    r.render()                       # warm-up frame of this arm
                one = one_at_a_time(slots, s, args.frames)
                kb = slots[0].last_variant()
                fl = in_flight(slots, s, args.frames)
                kf = slots[0].last_variant()
                kernels[arm] = (kb, kf)
                res[arm]["one"].append(one)
                res[arm]["flight"].append(fl)
                print(f"{name:8s} {W}x{H} round {rnd} Doppler {arm:3s}: one at a time {one:8.4f} ms (kernel {kb})   3 in flight {fl:8.4f} ms/frame (kernel {kf})", flush=True)
        row = {"scene": name, "W": W, "H": H, "kernels_off": kernels["off"], "kernels_on": kernels["on"]}
        for mode in ("one", "flight"):
            off, on = statistics.median(res["off"][mode]), statistics.median(res["on"][mode])
            row[f"ms_{mode}_off"], row[f"ms_{mode}_on"] = round(off, 4), round(on, 4)
            row[f"cost_{mode}_pct"] = round((on / off - 1) * 100, 1)
        rows.append(row)
        for r in slots:
            r.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
