#!/usr/bin/env python3
"""What the sky costs (rpt_set_environment): environment off against on (a 4096x2048 image at rest in the scene's frame) and on with a
1x1 image (the same arithmetic, every tap on one texel: what is left of the cost without the scattered texel loads), on the same
contexts, A/B/C/A/B/C, camera at 0.95c so that the lookups scatter; ms/frame one frame at a time (rpt_set_objects +
rpt_set_environment_frame + rpt_render) and with four frames in flight (rpt_render_async on four contexts sharing the scene).
Prints one line per arm and a JSON summary (median of the arms per mode).
usage: python tools/environment_cost.py [--frames 40] [--rounds 2]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relativitypathtracer_amd import Scene                      # noqa: E402
from relativitypathtracer_amd.renderer import Renderer          # noqa: E402

V = (0.0, 0.0, 0.95)
CONFIGS = [("bunny", 0.0, "pinhole", 3840, 2160), ("shadows", 16.0, "pinhole", 3840, 2160), ("arch", 5.25, "pinhole", 1920, 1080),
           ("cubes", 3.0, "pinhole", 3840, 2160), ("bunny", 0.0, "equirect", 3840, 1920)]
ARMS = ("off", "on", "on_1x1")
IN_FLIGHT = 4


def sky(width, height):
    y, x = np.mgrid[0:height, 0:width]
    return np.ascontiguousarray(np.stack([(x * 7 + y) & 255, (x + y * 5) & 255, (x ^ y) & 255], -1).astype(np.uint8))


def one_at_a_time(slots, s, E, frames):
    t0 = time.perf_counter()
    for _ in range(frames):
        slots[0].set_objects(s)
        slots[0].set_environment_frame(E)
        slots[0].render()
    return (time.perf_counter() - t0) / frames * 1e3


def in_flight(slots, s, E, frames):
    t0 = time.perf_counter()
    for f in range(frames * len(slots)):
        r = slots[f % len(slots)]
        r.sync()
        r.set_objects(s)
        r.set_environment_frame(E)
        r.render_async()
    for r in slots:
        r.sync()
    return (time.perf_counter() - t0) / (frames * len(slots)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2, help="off / on / on_1x1 triples per configuration")
    args = ap.parse_args()
    images = {"off": None, "on": sky(4096, 2048), "on_1x1": sky(1, 1)}
    rows = []
    for name, t, proj, W, H in CONFIGS:
        s = Scene.from_file(name)
        s.set_camera(V, t)
        s.update_objects()
        E = s.camera_lorentz()[1]
        slots = [Renderer(0) for _ in range(IN_FLIGHT)]
        slots[0].upload_scene(s)
        for r in slots[1:]:
            r.share_scene(slots[0])
        res = {arm: {"one": [], "flight": []} for arm in ARMS}
        kernels = {}
        for rnd in range(args.rounds):
            for arm in ARMS:
                for r in slots:
                    r.set_projection(proj)
                    r.set_environment(images[arm])
                    r.set_scene_params(s, W, H)
                    r.set_output(None)
                    r.set_objects(s)
                    r.set_environment_frame(E)
                    r.render()                       # warm-up frame of this arm
                one = one_at_a_time(slots, s, E, args.frames)
                kb = slots[0].last_variant()
                fl = in_flight(slots, s, E, args.frames)
                kf = slots[0].last_variant()
                kernels[arm] = (kb, kf)
                res[arm]["one"].append(one)
                res[arm]["flight"].append(fl)
                print(f"{name:8s} {proj:8s} {W}x{H} round {rnd} {arm:7s}: one at a time {one:8.4f} ms (kernel {kb})   {IN_FLIGHT} in flight "
                      f"{fl:8.4f} ms/frame (kernel {kf})", flush=True)
        row = {"scene": name, "projection": proj, "size": [W, H], "kernels": kernels}
        for mode in ("one", "flight"):
            off = statistics.median(res["off"][mode])
            row[f"ms_{mode}_off"] = round(off, 4)
            for arm in ARMS[1:]:
                on = statistics.median(res[arm][mode])
                row[f"ms_{mode}_{arm}"] = round(on, 4)
                row[f"cost_{mode}_{arm}_pct"] = round((on / off - 1) * 100, 1)
        rows.append(row)
        for r in slots:
            r.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
