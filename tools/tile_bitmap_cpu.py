#!/usr/bin/env python3
"""How many of a mesh's masked tiles are empty, and how many of those the tile bitmap (csrc/rpt_tile_bitmap.hpp) clears.  CPU only.

    python tools/tile_bitmap_cpu.py [--workload bunny] [--width 3840 --height 2160] [--boxes 8 64 512]

Renders the mesh alone on the oracle, counts per 8x8 tile: kept by today's object mask (the proven rectangle / octagon around the
root box, wave_object_mask's skirt), of those without a hit pixel, of those cleared by the bitmap for each number of sub-tree boxes
(the sub-tree stage alone: RPT_TILE_TRIANGLES=0 for those rows), by the triangle stage alone and by the product a context puts on
the device (the sub-tree stage at 64 boxes ANDed with the triangle stage).  Every figure is a CPU count; none is a device time.
"""
import argparse
import ctypes as C
import os
import sys

import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_ffi  # noqa: E402
from relativitypathtracer_amd import Scene, _ffi  # noqa: E402
from tile_bitmap_helpers import bitmap, hit_tiles, mask_tiles  # noqa: E402


def main():
    import test_screen_bounds as tsb
    from bench import WORKLOADS
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bunny")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--boxes", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--max-triangles", type=int, default=8192, help="the triangle stage's cap (rptb::tiles::MAX_TRIANGLES)")
    args = ap.parse_args()
    name, vel, t = WORKLOADS[args.workload]
    scene = Scene.from_file(name)
    scene.set_camera(vel, t)
    scene.update_objects()
    W, H = args.width, args.height
    objs = scene.objects()
    for i in range(len(objs)):
        if int(objs["type"][i]) != 2:
            continue
        n = scene.octrees()[int(objs["meshIndex"][i])]
        root = (C.c_float * 6)(*n["min"][:3], *n["max"][:3])
        b = (C.c_float * 8)()
        assert _ffi.hip().rpt_object_screen_bounds(objs[i:i + 1].copy().ctypes.data, scene.params["interval"], root, b) == 0
        kept = mask_tiles(tuple(b), W, H)
        only = objs[i:i + 1].copy()
        _, _, stats = oracle_ffi.render(scene, W, H, objects=only, want_stats=True, want_rgb=False)
        hit = hit_tiles(tsb.hit_mask(scene, i, W, H), W, H)
        empty = kept & ~hit
        print(f"{name} {W}x{H} object {i}: tiles {kept.size}, kept by the mask {int(kept.sum())}, of those without a hit pixel {int(empty.sum())} "
              f"({100.0 * empty.sum() / max(kept.sum(), 1):.1f} %)")
        print(f"  oracle, this mesh alone, whole frame: octree walks {stats['root_aabb_hits']}, leaf visits {stats['leaf_visits']}, "
              f"descent steps {stats['descent_steps']}, triangle tests {stats['tri_tests']}, pixels hit {stats['pixels_hit']}")
        def row(label, bm, dt):
            assert not (hit & ~bm).any(), "a hit tile was cleared"
            cleared = kept & ~bm
            print(f"  {label}: cleared {int(cleared.sum())} of the kept tiles ({100.0 * cleared.sum() / max(kept.sum(), 1):.1f} % of the kept, "
                  f"{100.0 * cleared.sum() / max(empty.sum(), 1):.1f} % of the empty ones), tiles left walking {int((kept & bm).sum())}, host build {dt * 1e3:.2f} ms")

        words = ((W + 7) // 8 * ((H + 7) // 8) + 31) // 32
        bits = np.zeros(words, dtype=np.uint32)
        st4 = (C.c_int * 4)()
        t0 = time.perf_counter()
        rc = _ffi.hip().rpt_tile_bitmap_stage_host(C.byref(scene.desc()), i, scene.params["interval"], W, H, 1.0, 1, args.max_triangles, bits.ctypes.data, words, st4)
        dt = time.perf_counter() - t0
        if rc == 1:
            tri = np.unpackbits(bits.view(np.uint8), bitorder="little")[:kept.size].reshape(kept.shape).astype(bool)
            row(f"triangle stage alone, {st4[0]} boxes ({st4[1]} proven)", tri, dt)
        else:
            print(f"  triangle stage: none (return {rc}, stats {tuple(st4)})")
        os.environ.pop("RPT_TILE_TRIANGLES", None)
        bm, st, dt = bitmap(scene, i, W, H, 64)
        if bm is None:
            print(f"  product: no bitmap (stats {st})")
        else:
            row(f"product (sub-tree stage, {st[0]} boxes, AND triangle stage)", bm, dt)
        os.environ["RPT_TILE_TRIANGLES"] = "0"          # the rows below: the sub-tree stage alone
        for mb in args.boxes:
            bm, st, dt = bitmap(scene, i, W, H, mb)
            if bm is None:
                print(f"  max_boxes {mb}: no bitmap (stats {st})")
                continue
            assert not (hit & ~bm).any(), "a hit tile was cleared"
            cleared = kept & ~bm
            print(f"  max_boxes {mb}: cut at depth {st[4]}, {st[0]} boxes ({st[1]} proven), cleared {int(cleared.sum())} of the kept tiles "
                  f"({100.0 * cleared.sum() / max(kept.sum(), 1):.1f} % of the kept, {100.0 * cleared.sum() / max(empty.sum(), 1):.1f} % of the empty ones), "
                  f"host build {dt * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
