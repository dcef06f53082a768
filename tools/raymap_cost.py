#!/usr/bin/env python3
"""What the ray-map camera costs (rpt_set_raymap): at 3840x2160 and 4096x4096 on the shipped scenes, on the same contexts, A/B/C per round,
  equirect   the panorama frame of that size — the nearest existing kernel: the same culls, no map read (341 / 344);
  pano_map   a ray map filled with the panorama's own directions — the same rays, so the difference to `equirect` is the map read (1241 / 1244);
  fisheye    a 180-degree equidistant fisheye inscribed in the frame: the pixels outside the image circle have no ray;
ms/frame one frame at a time (rpt_set_objects + rpt_render) and with four frames in flight (rpt_render_async on four contexts sharing
the scene, each with its own copy of the map).  Prints one line per arm and a JSON summary (median of the arms per mode).
usage: python tools/raymap_cost.py [--frames 20] [--rounds 2] [--scenes bunny,shadows,arch,cubes] [--sizes 3840x2160,4096x4096]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relativitypathtracer_amd import Scene                                          # noqa: E402
from relativitypathtracer_amd.renderer import Renderer, projection_tables, raymap   # noqa: E402

CONFIGS = {"bunny": ((0, 0, 0), 0.0), "shadows": ((0, 0, 0), 16.0), "arch": ((0, 0, 0.95), 5.25), "cubes": ((0.3, 0, 0.1), 3.0)}
ARMS = ("equirect", "pano_map", "fisheye")
IN_FLIGHT = 4


def pano_dirs(W, H):
    """the panorama's p (include/rpt.h) as the kernels form it: float products of the library's own tables"""
    cols, rows = projection_tables(W, H)
    sl, cl = cols[None, :, 0], cols[None, :, 1]
    sp, cp = rows[:, None, 0], rows[:, None, 1]
    return np.ascontiguousarray(np.stack([cp * sl, np.broadcast_to(sp, (H, W)), cp * cl], -1).astype(np.float32))


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
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="A/B/C triples per configuration")
    ap.add_argument("--scenes", default="bunny,shadows,arch,cubes")
    ap.add_argument("--sizes", default="3840x2160,4096x4096")
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in size.split("x")) for size in args.sizes.split(",")]
    rows = []
    for W, H in sizes:
        maps = {"pano_map": pano_dirs(W, H), "fisheye": raymap("fisheye", W, H, fov=math.pi, fit=0)}
        share = {arm: float(np.any(m != 0, axis=-1).mean()) for arm, m in maps.items()}
        for name in args.scenes.split(","):
            vel, t = CONFIGS[name]
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
                for arm in ARMS:
                    for r in slots:
                        if arm == "equirect":
                            r.set_projection("equirect")
                        else:
                            r.set_raymap(maps[arm])
                            r.set_projection("raymap")
                        r.set_scene_params(s, W, H)
                        r.set_output(None)
                        r.set_objects(s)
                        r.render()                       # warm-up frame of this arm
                    one = one_at_a_time(slots, s, args.frames)
                    kb = slots[0].last_variant()
                    fl = in_flight(slots, s, args.frames)
                    kernels[arm] = (kb, slots[0].last_variant())
                    res[arm]["one"].append(one)
                    res[arm]["flight"].append(fl)
                    print(f"{name:8s} {W}x{H} round {rnd} {arm:8s}: one at a time {one:8.4f} ms (kernel {kb})   {IN_FLIGHT} in flight "
                          f"{fl:8.4f} ms/frame (kernel {kernels[arm][1]})", flush=True)
            row = {"scene": name, "size": f"{W}x{H}", "kernels": kernels, "fisheye_ray_share": round(share["fisheye"], 4)}
            for mode in ("one", "flight"):
                base = statistics.median(res["equirect"][mode])
                row[f"ms_{mode}_equirect"] = round(base, 4)
                for arm in ("pano_map", "fisheye"):
                    v = statistics.median(res[arm][mode])
                    row[f"ms_{mode}_{arm}"] = round(v, 4)
                    row[f"cost_{mode}_{arm}_pct"] = round((v / base - 1) * 100, 1)
            rows.append(row)
            for r in slots:
                r.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
