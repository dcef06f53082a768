"""csrc/rpt_tile_bitmap.hpp, the triangle stage: one proven region per distinct triangle of the mesh, ANDed with the sub-tree stage.  The
product is what rpt_tile_bitmap_host returns and a context puts on the device; each stage alone (rpt_tile_bitmap_stage_host) and the
product are SOUND — no tile with an oracle hit pixel is cleared — and the product is not the sub-tree stage under another name.
Host code only (no GPU).

* Scenes/bunny.txt at rest at 640x360, 253x141 (neither side a multiple of 8) and 128x72;
* posed bunnies before moving cameras (test_tile_bitmap's scenes, on seeds beyond its twelve), the triangle stage alone;
* the fallbacks: over the cap, the pear, a NaN vertex;
* the rasterisation over the column range a rectangle spans against the loop over every column, restated here in numpy;
* the same bits with no helper threads and with four."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi  # noqa: F401  (builds the oracle)
import test_screen_bounds as tsb
from conftest import load_config
from relativitypathtracer_amd import _ffi
from test_tile_bitmap import _posed_bunny, check, meshes, scene_of
from tile_bitmap_helpers import bitmap, hit_tiles, mask_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(640, 360), (253, 141), (128, 72)]
MAX_TRIANGLES = 8192          # rptb::tiles::MAX_TRIANGLES


def unpack(bits, W, H):
    tx, ty = (W + 7) // 8, (H + 7) // 8
    return np.unpackbits(bits.view(np.uint8), bitorder="little")[:tx * ty].reshape(ty, tx).astype(bool)


def stage(desc, interval, i, W, H, which, max_triangles=MAX_TRIANGLES, lens=1.0):
    """One stage alone: ((tiles_y, tiles_x) bool array or None, stats, return code)."""
    words = ((W + 7) // 8 * ((H + 7) // 8) + 31) // 32
    bits = np.zeros(words, dtype=np.uint32)
    st = (C.c_int * 4)()
    rc = _ffi.hip().rpt_tile_bitmap_stage_host(C.byref(desc), i, interval, W, H, lens, which, max_triangles, bits.ctypes.data, words, st)
    return (unpack(bits, W, H) if rc == 1 else None), tuple(st), rc


@pytest.fixture(scope="module")
def bunny():
    scene = scene_of("bunny", 0.0)
    return scene, meshes(scene)[0]


_hit = {}


def bunny_hits(scene, i, W, H):
    if (W, H) not in _hit:
        _hit[(W, H)] = hit_tiles(tsb.hit_mask(scene, i, W, H), W, H)
    return _hit[(W, H)]


@pytest.mark.parametrize("W,H", SIZES)
def test_the_product_is_the_and_of_the_stages_and_clears_no_hit_tile(bunny, W, H):
    scene, i = bunny
    itv = scene.params["interval"]
    product, st, _ = bitmap(scene, i, W, H)
    s0, st0, rc0 = stage(scene.desc(), itv, i, W, H, 0)
    s1, st1, rc1 = stage(scene.desc(), itv, i, W, H, 1)
    assert product is not None and rc0 == 1 and rc1 == 1, (st, st0, st1)
    assert st[:4] == st0 and st0[0] <= 64 and st0[1] == st0[0]          # the host call's statistics stay the sub-tree stage's
    assert st1[0] == st1[1] and 64 < st1[0] <= MAX_TRIANGLES, st1       # one proof per distinct triangle
    assert (product == (s0 & s1)).all()
    hit = bunny_hits(scene, i, W, H)
    for name, bm in (("product", product), ("sub-tree stage", s0), ("triangle stage", s1)):
        bad = hit & ~bm
        assert not bad.any(), f"{W}x{H}: the {name} clears {int(bad.sum())} tiles with hit pixels"
    print(f"{W}x{H}: {int(hit.sum())} hit tiles; set: sub-tree stage {int(s0.sum())}, triangle stage {int(s1.sum())} ({st1[0]} triangles), product {int(product.sum())}")


def test_the_product_clears_over_a_third_of_the_masked_tiles(bunny):
    """Scenes/bunny.txt at rest, 640x360: 159 of the 400 tiles the object mask keeps (39.8 %) against the sub-tree stage's 109 (27.2 %).
    35 % cannot be met with the triangle stage silently off."""
    scene, i = bunny
    W, H = 640, 360
    objs = scene.objects()
    n = scene.octrees()[int(objs["meshIndex"][i])]
    b = (C.c_float * 8)()
    assert _ffi.hip().rpt_object_screen_bounds(objs[i:i + 1].copy().ctypes.data, scene.params["interval"], (C.c_float * 6)(*n["min"][:3], *n["max"][:3]), b) == 0
    kept = mask_tiles(tuple(b), W, H)
    product, _, _ = bitmap(scene, i, W, H)
    s0, _, _ = stage(scene.desc(), scene.params["interval"], i, W, H, 0)
    cleared, cleared0 = int((kept & ~product).sum()), int((kept & ~s0).sum())
    print(f"640x360: kept {int(kept.sum())}, cleared by the product {cleared}, by the sub-tree stage alone {cleared0}")
    assert cleared >= 0.35 * kept.sum(), (cleared, int(kept.sum()))
    assert cleared > cleared0


POSED_SEEDS = list(range(12, 24))


@pytest.mark.parametrize("seed", POSED_SEEDS)
def test_the_triangle_stage_clears_no_hit_tile_of_a_posed_bunny(seed):
    """test_tile_bitmap's posed bunnies (moving meshes, moving cameras) on further seeds: its own check on the product, and the triangle
    stage ALONE against the oracle's hit tiles."""
    scene = _posed_bunny(seed)
    W, H = [(160, 90), (128, 96), (200, 80)][seed % 3]
    check(scene, W, H, f"posed bunny {seed}")
    for i in meshes(scene):
        s1, st1, rc = stage(scene.desc(), scene.params["interval"], i, W, H, 1)
        assert rc >= 0
        if s1 is None:
            continue
        hit = hit_tiles(tsb.hit_mask(scene, i, W, H), W, H)
        bad = hit & ~s1
        assert not bad.any(), f"posed bunny {seed}: the triangle stage clears {int(bad.sum())} tiles with hit pixels (stats {st1})"


def test_at_least_half_of_the_posed_bunnies_get_a_triangle_stage():
    """The sweep above is not vacuous, counted here on its own (whatever subset or order of its cases ran)."""
    built = 0
    for seed in POSED_SEEDS:
        scene = _posed_bunny(seed)
        W, H = [(160, 90), (128, 96), (200, 80)][seed % 3]
        built += any(stage(scene.desc(), scene.params["interval"], i, W, H, 1)[2] == 1 for i in meshes(scene))
    assert built >= len(POSED_SEEDS) // 2, built


def test_over_the_cap_the_product_is_the_subtree_stage(bunny):
    scene, i = bunny
    W, H = 253, 141
    s1, st1, rc = stage(scene.desc(), scene.params["interval"], i, W, H, 1, max_triangles=100)
    assert rc == 0 and s1 is None
    s0, _, rc0 = stage(scene.desc(), scene.params["interval"], i, W, H, 0, max_triangles=100)
    assert rc0 == 1
    capped, _, rc2 = stage(scene.desc(), scene.params["interval"], i, W, H, 2, max_triangles=100)      # the product under that cap
    assert rc2 == 1 and (capped == s0).all()
    product, _, _ = bitmap(scene, i, W, H)
    assert not (product & ~s0).any() and (product != s0).any()            # under the library's own cap the triangle stage is in


def test_the_pear_gets_neither_stage():
    scene = load_config("shadows")
    ms = meshes(scene)
    assert ms
    for i in ms:
        for which in (0, 1):
            bm, _, rc = stage(scene.desc(), scene.params["interval"], i, 128, 72, which)
            assert rc == 0 and bm is None


def test_a_nan_vertex_in_a_listed_triangle_leaves_no_triangle_stage(bunny):
    scene, i = bunny
    d = scene.desc()
    buf = scene.buffers()
    t = int(buf["octreeTris"][0])                                       # a triangle a leaf list names
    vertices = buf["vertices"].copy()
    vertices[int(buf["triangles"][9 * t + 3]), 1] = np.nan
    broken = _ffi.SceneDesc()
    C.memmove(C.byref(broken), C.byref(d), C.sizeof(d))
    broken.vertices = vertices.ctypes.data
    bm, _, rc = stage(broken, scene.params["interval"], i, 128, 72, 1)
    assert rc <= 0 and bm is None
    bm, _, rc = stage(d, scene.params["interval"], i, 128, 72, 1)       # (the scene itself still gets one)
    assert rc == 1 and bm is not None


def full_row_loop(bounds, W, H, lens, diagonals):
    """build()'s rasterisation as it was: every tile column of every overlapping row, each tile tested on its own.  In double, in the
    order of operations of the header's tables."""
    tx, ty = np.arange((W + 7) // 8, dtype=np.float64), np.arange((H + 7) // 8, dtype=np.float64)
    aspect = np.float64(np.float32(W) / np.float32(H))
    s = np.float64(np.float32(lens))
    u0 = s * (((8.0 * tx - 1.5) / W - 0.5) * aspect)
    u1 = s * (((8.0 * tx + 8.5) / W - 0.5) * aspect)
    v0 = (s * ((8.0 * ty - 1.5) / H - 0.5))[:, None]
    v1 = (s * ((8.0 * ty + 8.5) / H - 0.5))[:, None]
    b = [np.float64(x) for x in bounds]
    out = (b[2] < u0) | (b[0] > u1) | (b[3] < v0) | (b[1] > v1)
    if diagonals:
        out = out | (b[5] < u0 + v0) | (b[4] > u1 + v1) | (b[7] < u0 - v1) | (b[6] > u1 - v0)
    return ~out


def test_the_column_range_rasterisation_sets_the_bits_of_the_full_row_loop():
    rng = np.random.default_rng(20)
    big = np.float32(3.0e38)
    frames = [(640, 360), (253, 141), (128, 72), (200, 80), (8, 8), (1000, 250)]
    for trial in range(200):
        W, H = frames[trial % len(frames)]
        lens = [1.0, 1.0, 0.5, 0.37][trial % 4]
        kind = trial % 10
        cu, cv = rng.uniform(-1.0, 1.0), rng.uniform(-0.6, 0.6)
        hu, hv = rng.uniform(0.0, 0.5) ** 2, rng.uniform(0.0, 0.5) ** 2
        if kind == 0:
            hu = hv = 0.0                                               # a point
        elif kind == 1:
            cu = 5.0 * (1 if rng.random() < 0.5 else -1)                # off the frame
        elif kind == 2:
            cu, cv, hu, hv = 0.0, 0.0, float(big), float(big)           # the whole frame
        elif kind == 3:
            cu = float(np.float32(((8.0 * int(rng.integers(0, (W + 7) // 8)) - 1.5) / W - 0.5) * (W / H)))      # an edge on a tile's own edge
        rect = np.array([cu - hu, cv - hv, cu + hu, cv + hv], dtype=np.float32)
        rect = np.clip(rect, -big, big)
        diagonals = trial % 2 == 1
        if diagonals:
            slack = rng.uniform(-0.3, 0.4, size=4) * (hu + hv)
            diag = np.array([cu + cv - (hu + hv) + max(slack[0], 0), cu + cv + (hu + hv) - max(slack[1], 0),
                             cu - cv - (hu + hv) + max(slack[2], 0), cu - cv + (hu + hv) - max(slack[3], 0)], dtype=np.float32)
        else:
            diag = np.array([-big, big, -big, big], dtype=np.float32)
        bounds = np.concatenate([rect, np.clip(diag, -big, big)]).astype(np.float32)
        if kind == 4:
            bounds[0], bounds[2] = np.float32(0.3), np.float32(0.1)     # empty: u0 > u1
        words = ((W + 7) // 8 * ((H + 7) // 8) + 31) // 32
        bits = np.full(words, 0xffffffff, dtype=np.uint32)
        rc = _ffi.hip().rpt_tile_rasterise_host(W, H, lens, int(diagonals), bounds.ctypes.data_as(C.POINTER(C.c_float)), bits.ctypes.data, words)
        got = unpack(bits, W, H)
        if kind == 4:
            assert rc == 0 and not got.any()
            continue
        assert rc == 1
        want = full_row_loop(bounds, W, H, lens, diagonals)
        assert (got == want).all(), f"trial {trial}: {W}x{H} lens {lens} bounds {bounds.tolist()}: {int((got != want).sum())} tiles differ"
        if kind == 2:
            assert got.all()
        if kind == 1:
            assert not got.any()


CHILD = """
import ctypes as C, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from relativitypathtracer_amd import Scene
from tile_bitmap_helpers import bitmap
s = Scene.from_file("bunny")
s.set_camera((0.0, 0.0, 0.0), 0.0)
s.update_objects()
objs = s.objects()
i = [k for k in range(len(objs)) if int(objs["type"][k]) == 2][0]
bm, st, _ = bitmap(s, i, 640, 360)
assert bm is not None
sys.stdout.write(np.packbits(bm).tobytes().hex())
"""


def test_the_bits_do_not_depend_on_the_helper_threads():
    out = []
    for threads in ("0", "4"):
        env = dict(os.environ, RPT_HOST_THREADS=threads)
        env.pop("RPT_TILE_TRIANGLES", None)
        p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        out.append(p.stdout)
    assert out[0] and out[0] == out[1]
