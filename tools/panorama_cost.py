#!/usr/bin/env python3
"""What the equirectangular camera costs (rpt_set_projection): pinhole 3840x2160 (the reference's camera, kernels 43 / 41 / 44) against
equirect 3840x1920 (the full sphere at square pixels, kernels 341 / 344) on the same contexts, A/B/A/B, ms/frame one frame at a time
(rpt_set_objects + rpt_render) and with four frames in flight (rpt_render_async on four contexts sharing the scene).  Prints one line
per arm and a JSON summary (median of the arms per mode).
usage: python tools/panorama_cost.py [--frames 40] [--rounds 2]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relativitypathtracer_amd import Scene                      # noqa: E402
from relativitypathtracer_amd.renderer import Renderer          # noqa: E402

CONFIGS = [("bunny", (0, 0, 0), 0.0), ("shadows", (0, 0, 0), 16.0), ("arch", (0, 0, 0.95), 5.25), ("cubes", (0.3, 0, 0.1), 3.0)]
ARMS = {"pinhole": (3840, 2160), "equirect": (3840, 1920)}
IN_FLIGHT = 4


def one_at_a_time(slots, s, frames):
    t0 = time.perf_counter()
    for _ in range(frames):
        slots[0].set_objects(s)
        slots[0].render()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2, help="A/B pairs per configuration")
    args = ap.parse_args()
    rows = []
    for name, vel, t in CONFIGS:
        s = Scene.from_file(name)
        s.set_camera(vel, t)
        s.update_objects()
        slots = [Renderer(0) for _ in range(IN_FLIGHT)]
        slots[0].upload_scene(s)
        for r in slots[1:]:
            r.share_scene(slots[0])
        res = {arm: {"one": [], "flight": []} for arm in ARMS}
        kernels = {}
        for rnd in range(args.rounds):
            for arm, (W, H) in ARMS.items():
                for r in slots:
                    r.set_projection(arm)
                    r.set_scene_params(s, W, H)
                    r.set_output(None)
                    r.set_objects(s)
                    r.render()                       # warm-up frame of this arm
                one = one_at_a_time(slots, s, args.frames)
                kb = slots[0].last_variant()
                fl = in_flight(slots, s, args.frames)
                kf = slots[0].last_variant()
                kernels[arm] = (kb, kf)
                res[arm]["one"].append(one)
                res[arm]["flight"].append(fl)
                print(f"{name:8s} round {rnd} {arm:8s} {W}x{H}: one at a time {one:8.4f} ms (kernel {kb})   {IN_FLIGHT} in flight "
                      f"{fl:8.4f} ms/frame (kernel {kf})", flush=True)
        row = {"scene": name, "kernels": kernels}
        for mode in ("one", "flight"):
            a, b = statistics.median(res["pinhole"][mode]), statistics.median(res["equirect"][mode])
            row[f"ms_{mode}_pinhole"], row[f"ms_{mode}_equirect"] = round(a, 4), round(b, 4)
            row[f"cost_{mode}_pct"] = round((b / a - 1) * 100, 1)
            # per pixel: the equirect frame has 8/9 of the pinhole's pixels
            row[f"cost_{mode}_per_pixel_pct"] = round((b / (ARMS["equirect"][0] * ARMS["equirect"][1]) / (a / (ARMS["pinhole"][0] * ARMS["pinhole"][1])) - 1) * 100, 1)
        rows.append(row)
        for r in slots:
            r.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
