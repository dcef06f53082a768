#!/usr/bin/env python3
"""What per-object time windows cost (rpt_set_object_windows) when they reject nothing: at 3840x2160 on the shipped scenes, on the same
contexts, A/B per round,
  plain      the frame without windows — the parent's machine code (profiles/r15_windows_kernel_code_diff.txt);
  windowed   the same frame with every window at its default (-inf, +inf): the windowed kernel of the same camera, the same pixels —
             three more compares per candidate hit, occluder and light, the Doppler twin's code with the flag 0 in the plain colour,
             and the walk instead of the band-first form in the blocking call;
ms/frame one frame at a time (rpt_set_objects + rpt_render) and with four frames in flight (rpt_render_async on four contexts sharing
the scene).  Prints one line per arm and a JSON summary (median of the arms per mode).  Windows that DO reject make frames cheaper or
dearer by what they hide or uncover; that is the scene's cost, not the mechanism's, and is not measured here.
usage: python tools/windows_cost.py [--frames 2000] [--rounds 5] [--scenes bunny,arch,shadows] [--sizes 3840x2160]"""
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

CONFIGS = {"bunny": ((0, 0, 0), 0.0), "shadows": ((0, 0, 0), 16.0), "arch": ((0, 0, 0.95), 5.25), "cubes": ((0.3, 0, 0.1), 3.0)}
ARMS = ("plain", "windowed")
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
    ap.add_argument("--frames", type=int, default=2000, help="per timed window: 2000 frames of 0.1-0.3 ms are 0.2-0.6 s of wall clock (x 4 in flight)")
    ap.add_argument("--rounds", type=int, default=5, help="A/B pairs per configuration")
    ap.add_argument("--scenes", default="bunny,arch,shadows")
    ap.add_argument("--sizes", default="3840x2160")
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in size.split("x")) for size in args.sizes.split(",")]
    rows = []
    for W, H in sizes:
        for name in args.scenes.split(","):
            vel, t = CONFIGS[name]
            s = Scene.from_file(name)
            s.set_camera(vel, t)
            s.update_objects()
            n = len(s.objects())
            default = np.empty((n, 2), dtype=np.float32)
            default[:, 0], default[:, 1] = -np.inf, np.inf
            slots = [Renderer(0) for _ in range(IN_FLIGHT)]
            slots[0].upload_scene(s)
            for r in slots[1:]:
                r.share_scene(slots[0])
            res = {arm: {"one": [], "flight": []} for arm in ARMS}
            kernels = {}
            for rnd in range(args.rounds):
                for arm in ARMS:
                    for r in slots:
                        r.set_object_windows(default if arm == "windowed" else None)
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
            row = {"scene": name, "size": f"{W}x{H}", "kernels": kernels}
            for mode in ("one", "flight"):
                base = statistics.median(res["plain"][mode])
                v = statistics.median(res["windowed"][mode])
                row[f"ms_{mode}_plain"] = round(base, 4)
                row[f"ms_{mode}_windowed"] = round(v, 4)
                for arm in ARMS:
                    row[f"spread_{mode}_{arm}_pct"] = round((max(res[arm][mode]) / min(res[arm][mode]) - 1) * 100, 1)
                row[f"cost_{mode}_pct"] = round((v / base - 1) * 100, 1)
            rows.append(row)
            for r in slots:
                r.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
