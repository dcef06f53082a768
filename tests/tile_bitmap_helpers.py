"""Helpers of the tile-bitmap tests (csrc/rpt_tile_bitmap.hpp) and of tools/tile_bitmap_cpu.py: the object mask restated on the host,
the library's bitmap as a boolean array, hit pixels gathered into tiles.  TEST INFRASTRUCTURE, host code only."""
import ctypes as C
import time

import numpy as np

from relativitypathtracer_amd import _ffi


def mask_tiles(bounds, W, H, diagonals=True):
    """wave_object_mask on the host: the tiles whose square, grown by a pixel and a half, touches the region."""
    tx, ty = np.arange((W + 7) // 8), np.arange((H + 7) // 8)
    aspect = np.float32(W) / np.float32(H)
    u0 = ((8.0 * tx - 1.5) / W - 0.5) * aspect
    u1 = ((8.0 * tx + 8.5) / W - 0.5) * aspect
    v0 = ((8.0 * ty - 1.5) / H - 0.5)[:, None]
    v1 = ((8.0 * ty + 8.5) / H - 0.5)[:, None]
    b = bounds
    out = (b[2] < u0) | (b[0] > u1) | (b[3] < v0) | (b[1] > v1)
    if diagonals:
        out = out | (b[5] < u0 + v0) | (b[4] > u1 + v1) | (b[7] < u0 - v1) | (b[6] > u1 - v0)
    return ~out


def bitmap(scene, i, W, H, max_boxes=64, lens=1.0, boxes=None):
    """(tiles_y, tiles_x) bool array of the bitmap's set bits, the stats, the host seconds; None if the object gets no bitmap."""
    words = ((W + 7) // 8 * ((H + 7) // 8) + 31) // 32
    bits = np.zeros(words, dtype=np.uint32)
    st = (C.c_int * 5)()
    bx = None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float32)
    t0 = time.perf_counter()
    rc = _ffi.hip().rpt_tile_bitmap_host(C.byref(scene.desc()), i, scene.params["interval"], W, H, lens, max_boxes,
                                         None if bx is None else bx.ctypes.data, 0 if bx is None else bx.size // 6, bits.ctypes.data, words, st)
    dt = time.perf_counter() - t0
    if rc < 0:
        raise RuntimeError(f"rpt_tile_bitmap_host: {rc}")
    if rc == 0:
        return None, tuple(st), dt
    flat = np.unpackbits(bits.view(np.uint8), bitorder="little")[:(W + 7) // 8 * ((H + 7) // 8)]
    return flat.reshape((H + 7) // 8, (W + 7) // 8).astype(bool), tuple(st), dt


def hit_tiles(hit, W, H):
    ty, tx = (H + 7) // 8, (W + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), dtype=bool)
    pad[:H, :W] = hit
    return pad.reshape(ty, 8, tx, 8).any(axis=(1, 3))
