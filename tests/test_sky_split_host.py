"""The sky split's box on the host (csrc/rpt_sky_split.hpp), without a device: for 10 000 random sets of rectangles at odd
frame sizes no tile outside rpts::object_box's box passes the device's test — wave_object_mask of csrc/rpt_kernels.hip.h without its diagonal
slabs (which only ever drop an object), restated here operation for operation in numpy float32 — and the box is not loose: for a single
object it lies within two tiles of the tiles the device keeps.  The C++ is built with g++ from tests/native/sky_split_main.cpp."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sky_split_main.cpp")
SIZES = [(67, 45), (33, 257), (200, 120), (63, 65), (641, 479), (1001, 251), (9, 7), (257, 33), (1023, 257)]
LARGE_SIZES = [(1921, 1081), (3841, 2161)]      # every 40th set: the restatement costs a comparison per object and tile
SETS = 10000
F = np.float32
BIG = F(3.0e38)


def device_keeps(rects, W, H):
    """[tiles_y, tiles_x] bool: some object i < 64 is kept for the tile — wave_object_mask's four compares, float32 throughout"""
    tx, ty = (W + 7) // 8, (H + 7) // 8
    iw, ih, aspect = F(1.0) / F(W), F(1.0) / F(H), F(W) / F(H)
    x0, y0 = (np.arange(tx) * 8).astype(F), (np.arange(ty) * 8).astype(F)
    tu0, tu1 = ((x0 - F(1.5)) * iw - F(0.5)) * aspect, ((x0 + F(8.5)) * iw - F(0.5)) * aspect
    tv0, tv1 = (y0 - F(1.5)) * ih - F(0.5), (y0 + F(8.5)) * ih - F(0.5)
    assert tu0.dtype == F and tv1.dtype == F
    r = rects[:64]
    with np.errstate(invalid="ignore"):
        out_u = (r[:, 2, None] < tu0[None, :]) | (r[:, 0, None] > tu1[None, :])       # [objects, tiles_x]; a NaN compares false: kept
        out_v = (r[:, 3, None] < tv0[None, :]) | (r[:, 1, None] > tv1[None, :])       # [objects, tiles_y]
    return (~out_v[:, :, None] & ~out_u[:, None, :]).any(axis=0)


def random_rect(rng, aspect):
    kind = rng.integers(0, 12)
    if kind == 0:
        return np.array([-BIG, -BIG, BIG, BIG], dtype=F)                       # rptb::full_rect: an unproven bound
    if kind == 1:
        return np.array([BIG, BIG, -BIG, -BIG], dtype=F)                       # rptb::empty_rect: behind the camera
    if kind == 2:
        r = rng.uniform(-0.4, 0.4, 4).astype(F)
        r[rng.integers(0, 4)] = [np.nan, np.inf, -np.inf][rng.integers(0, 3)]
        return r
    cu, cv = rng.uniform(-0.75, 0.75) * aspect, rng.uniform(-0.75, 0.75)       # centres up to half a frame outside
    if kind == 3:                                                              # far outside, either side
        cu, cv = rng.choice([-1, 1]) * rng.uniform(1, 50) * aspect, rng.choice([-1, 1]) * rng.uniform(0, 50)
    hu, hv = (10.0 ** rng.uniform(-4, -0.3)) * aspect, 10.0 ** rng.uniform(-4, -0.3)
    if kind == 4:
        hu = hv = 0.0                                                          # a point
    return np.array([cu - hu, cv - hv, cu + hu, cv + hv], dtype=F)


def make_sets(rng):
    sets = []
    for k in range(SETS):
        W, H = LARGE_SIZES[k // 40 % 2] if k % 40 == 0 else SIZES[rng.integers(0, len(SIZES))]
        n = int(rng.choice([0, 1, 1, 1, 2, 3, 5, 8, 34, 64, 70]))
        rects = np.zeros((n, 8), dtype=F)
        for i in range(n):
            rects[i, :4] = random_rect(rng, W / H)
            rects[i, 4:] = [-BIG, BIG, -BIG, BIG]
        if n == 70:
            rects[64:, :4] = [-BIG, -BIG, BIG, BIG]      # beyond the mask's 64 bits: tested everywhere by trace(), no business of the box
            if k % 2:
                rects[:64, :4] = rects[:64, :4] * F(0.2)
        sets.append((W, H, rects))
    return sets


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ builds librpt_scene.so (csrc/Makefile): a machine without it cannot build the project either"
    path = str(tmp_path_factory.mktemp("sky_split") / "sky_split_main")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-o", path, SRC], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return path


def test_no_tile_outside_the_box_passes_the_devices_test(exe, tmp_path):
    rng = np.random.default_rng(20250611)
    sets = make_sets(rng)
    src, dst = tmp_path / "sets.bin", tmp_path / "boxes.bin"
    with open(src, "wb") as f:
        for W, H, rects in sets:
            f.write(np.array([W, H, len(rects)], dtype=np.int32).tobytes())
            f.write(rects.tobytes())
    p = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.split()[0] == str(SETS), (p.returncode, p.stdout, p.stderr)
    boxes = np.fromfile(dst, dtype=np.int32).reshape(SETS, 5)
    with_box = full = nothing = single = 0
    for (W, H, rects), (any_, x0, y0, x1, y1) in zip(sets, boxes):
        tx, ty = (W + 7) // 8, (H + 7) // 8
        keeps = device_keeps(rects, W, H) if len(rects) else np.zeros((ty, tx), dtype=bool)
        assert 0 <= x0 <= x1 <= tx and 0 <= y0 <= y1 <= ty
        assert bool(any_) == (x0 < x1 and y0 < y1)
        outside = keeps.copy()
        outside[y0:y1, x0:x1] = False
        assert not outside.any(), f"{W}x{H}, {len(rects)} rectangles: the device keeps an object in tile (x, y) = {np.argwhere(outside)[0][::-1]} outside the box {(x0, y0, x1, y1)}"
        with_box += int(any_)
        full += int(any_ and (x1 - x0) * (y1 - y0) == tx * ty)
        nothing += int(not any_)
        if len(rects) == 1 and keeps.any():       # not loose: within two tiles of what the device keeps
            ys, xs = np.nonzero(keeps)
            assert x0 >= xs.min() - 2 and x1 <= xs.max() + 3 and y0 >= ys.min() - 2 and y1 <= ys.max() + 3, (W, H, rects[0, :4], (x0, y0, x1, y1))
            assert x0 <= max(xs.min() - 1, 0) and x1 >= min(xs.max() + 2, tx) and y0 <= max(ys.min() - 1, 0) and y1 >= min(ys.max() + 2, ty), "the whole-tile margin"
            single += 1
    print(f"{SETS} sets: {with_box} with a box ({full} of them the whole frame), {nothing} with none; {single} single objects held to two tiles")
    assert with_box > SETS // 2 and nothing > SETS // 50 and full > SETS // 50 and single > SETS // 20      # every kind of answer occurred
