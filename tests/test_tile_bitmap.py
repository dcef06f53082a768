"""csrc/rpt_tile_bitmap.hpp: the per-object tile bitmap is SOUND — every pixel the oracle (the kernel's float arithmetic, restated)
reports as a hit of a mesh lies in a tile whose bit is set — and is not vacuous.  Host code only (no GPU).

* bunny and cube-mesh scenes at 128x72 and 640x360, at rest and on a sweep of camera speeds to 0.95c, under a lens as well;
* generated mesh scenes (tests/scene_fuzz.py: random_scene_text, meshwalls_scene_text, close_scene_text);
* pear.obj (16.2 K = 3.1: the hit margin is unprovable) gets no bitmap;
* a broken sub-tree box — non-finite, inverted, or so large that its region cannot be proven — leaves NO bitmap (the kernel keeps
  today's mask), and a box moved elsewhere only ever ADDS set bits next to the mesh's own: with the mesh's own boxes still in the
  list no tile the oracle hits is cleared.  (A finite, well-formed box that simply leaves triangles out cannot be told from a
  right one by any check on the box alone: the boxes are the library's own, computed at upload from the leaf lists.)"""
import ctypes as C
import numpy as np
import pytest

import oracle_ffi  # noqa: F401  (builds the oracle)
import test_screen_bounds as tsb
from conftest import load_config
from relativitypathtracer_amd import Scene, _ffi
from scene_fuzz import close_scene_text, meshwalls_scene_text, random_scene_text
from tile_bitmap_helpers import bitmap, hit_tiles, mask_tiles

CUBE_MESH = "MModels/cube.obj\nOm0\n p0.3,-0.2,6,0.6,0.2,1,0.3,1.2,0.8,1\n c0.8,0.6,0.3\nOs\n l1\n p2,3,2,0,0,1,0,0.3,0.3,0.3\n c1,1,1\nA0.3\nR\n"
SIZES = [(128, 72), (640, 360)]
_hits = {}


def scene_of(kind, speed):
    if kind == "bunny":
        s = Scene.from_file("bunny")
    else:
        s = Scene()
        s.inputScene(CUBE_MESH)
    s.set_camera((0.0, 0.0, speed), 0.0 if speed == 0.0 else 1.5)
    s.update_objects()
    return s


def meshes(scene):
    objs = scene.objects()
    return [i for i in range(min(len(objs), 64)) if int(objs["type"][i]) == 2]


def check(scene, W, H, label, lens=1.0, key=None):
    """Every mesh of the scene: no hit tile cleared.  Returns the number of bitmaps built and of tiles they cleared inside the mask."""
    built = cleared = 0
    for i in meshes(scene):
        bm, st, _ = bitmap(scene, i, W, H, 64, lens)
        if bm is None:
            continue
        built += 1
        assert lens == 1.0, "the oracle renders the reference's lens only"
        if key is None or (key, i, W, H) not in _hits:
            hit = hit_tiles(tsb.hit_mask(scene, i, W, H), W, H)
            if key is not None:
                _hits[(key, i, W, H)] = hit
        else:
            hit = _hits[(key, i, W, H)]
        bad = hit & ~bm
        assert not bad.any(), f"{label}: object {i}: {int(bad.sum())} tiles with hit pixels have their bit cleared (stats {st})"
        cleared += int((~bm).sum())
    return built, cleared


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("speed", [0.0, 0.3, 0.6, 0.8, 0.95])
@pytest.mark.parametrize("kind", ["bunny", "cube_mesh"])
def test_no_hit_tile_is_cleared(kind, speed, W, H):
    built, cleared = check(scene_of(kind, speed), W, H, f"{kind} v={speed} {W}x{H}", key=(kind, speed))
    if kind == "bunny":
        if speed <= 0.6:
            assert built == 1 and cleared > 0    # not vacuous: a bitmap that clears tiles (a box too near the camera's path has no provable region: no bitmap)
    else:
        assert built == 0                        # cube.obj: |e1| |e2| = 4, far beyond the provable margin


def test_the_bitmap_clears_a_quarter_of_the_masked_tiles_of_the_benchmark_frame():
    """Scenes/bunny.txt at rest, 640x360: of the tiles the root box's octagon keeps, the bitmap clears at least a fifth
    (26 % at 3840x2160, profiles/r13_tile_bitmap_cpu.txt), and never one with a hit pixel."""
    scene = scene_of("bunny", 0.0)
    W, H = 640, 360
    i = meshes(scene)[0]
    objs = scene.objects()
    n = scene.octrees()[int(objs["meshIndex"][i])]
    b = (C.c_float * 8)()
    assert _ffi.hip().rpt_object_screen_bounds(objs[i:i + 1].copy().ctypes.data, scene.params["interval"], (C.c_float * 6)(*n["min"][:3], *n["max"][:3]), b) == 0
    kept = mask_tiles(tuple(b), W, H)
    bm, st, _ = bitmap(scene, i, W, H)
    assert bm is not None and st[0] <= 64 and st[1] == st[0], st
    hit = hit_tiles(tsb.hit_mask(scene, i, W, H), W, H)
    assert not (hit & ~kept).any() and not (hit & ~bm).any()
    assert (kept & ~bm).sum() >= 0.2 * kept.sum(), (int((kept & ~bm).sum()), int(kept.sum()))


def test_the_pear_gets_no_bitmap():
    for name in ("shadows",):
        scene = load_config(name)
        ms = meshes(scene)
        assert ms
        for i in ms:
            for W, H in SIZES:
                assert bitmap(scene, i, W, H)[0] is None


def test_a_lens_scales_the_tiles_and_a_wide_frame_gets_nothing():
    scene = scene_of("bunny", 0.0)
    i = meshes(scene)[0]
    full, _, _ = bitmap(scene, i, 640, 360)
    tele, _, _ = bitmap(scene, i, 640, 360, lens=0.5)
    assert tele is not None and tele.sum() > 2 * full.sum()          # half the field of view: the mesh covers four times the tiles
    assert bitmap(scene, i, 1000, 100)[0] is None                     # beyond 4 : 1 the culled kernels are not launched at all
    assert bitmap(scene, i, 640, 360, lens=1.5)[0] is None            # a wider lens than the proven window


@pytest.mark.parametrize("seed", range(24))
def test_no_hit_tile_is_cleared_generated_scenes(seed):
    scene, text = _generated(seed)
    W, H = [(160, 90), (128, 96), (200, 80)][seed % 3]
    check(scene, W, H, f"seed {seed}\n{text}")


def _generated(seed):
    rng = np.random.default_rng(9100 + seed)
    gen = [random_scene_text, meshwalls_scene_text, close_scene_text][seed % 3]
    out = gen(rng)
    text = out[0] if isinstance(out, tuple) else out
    scene = Scene()
    scene.inputScene(text)
    vel = rng.normal(size=3)
    vel = vel / np.linalg.norm(vel) * rng.choice([0.0, 0.0, 0.5, 0.95])
    scene.set_camera(tuple(float(c) for c in vel), float(rng.uniform(-3, 20)))
    scene.update_objects()
    return scene, text


def _posed_bunny(seed):
    """Scenes/bunny.txt's mesh in a random pose (place, turn, size, sometimes moving) in front of a camera at rest or moving."""
    rng = np.random.default_rng(9500 + seed)
    pos = (rng.uniform(-2.5, 2.5), rng.uniform(-3.5, 0.5), rng.uniform(4.0, 12.0))
    axis = rng.normal(size=3)
    size = float(rng.choice([8.0, 20.0, 35.0]))
    lines = ["MModels/bunny.obj", "Om0",
             " p%.4f,%.4f,%.4f,%.4f,%.4f,%.4f,%.4f,%.3f,%.3f,%.3f" % (*pos, rng.uniform(0, 6.28), *axis, size, size * rng.uniform(0.6, 1.4), size),
             " c0.8,0.5,0.3"]
    if seed % 3 == 1:
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * float(rng.choice([0.3, 0.8]))
        lines.append(" v%.4f,%.4f,%.4f" % tuple(v))
    lines += ["Os", " l1", " p0,2,4,0,0,0,0,0.1,0.1,0.1", " c1,1,1", "A0.2", "R"]
    scene = Scene()
    scene.inputScene("\n".join(lines) + "\n")
    vel = rng.normal(size=3)
    vel = vel / np.linalg.norm(vel) * float(rng.choice([0.0, 0.4, 0.9]))
    scene.set_camera(tuple(float(c) for c in vel), 0.0)
    scene.update_objects()
    return scene


_posed_built = []


@pytest.mark.parametrize("seed", range(12))
def test_no_hit_tile_is_cleared_posed_bunnies(seed):
    """The generators above mostly draw meshes and poses that get no bitmap (the pear, cube.obj, a camera inside the root box); these
    scenes are made to get one.  The last case asserts that most of them did and cleared tiles: the sweep is not vacuous."""
    scene = _posed_bunny(seed)
    W, H = [(160, 90), (128, 96), (200, 80)][seed % 3]
    built, cleared = check(scene, W, H, f"posed bunny {seed}")
    _posed_built.append((built, cleared))
    if seed == 11 and len(_posed_built) == 12:
        assert sum(b for b, _ in _posed_built) >= 6 and sum(c > 0 for _, c in _posed_built) >= 6, _posed_built


def test_a_corrupted_box_never_clears_a_hit_tile():
    scene = scene_of("bunny", 0.0)
    W, H = 128, 72
    i = meshes(scene)[0]
    good, st, _ = bitmap(scene, i, W, H)
    hit = hit_tiles(tsb.hit_mask(scene, i, W, H), W, H)
    # the mesh's own boxes stand behind the library's interface; the root's box (it holds every vertex of bunny.obj) stands in for them
    n = scene.octrees()[int(scene.objects()["meshIndex"][i])]
    own = np.array([[*n["min"][:3], *n["max"][:3]]], dtype=np.float32)
    root_only, _, _ = bitmap(scene, i, W, H, boxes=own)
    assert root_only is not None and not (hit & ~root_only).any() and not (good & ~root_only).any()      # the cut refines the root's region
    good = root_only
    rng = np.random.default_rng(5)
    for trial in range(24):
        boxes = own.copy()
        k = int(rng.integers(0, len(boxes)))
        kind = trial % 6
        extra = boxes[k].copy()
        if kind == 0:
            extra[int(rng.integers(0, 6))] = np.nan
        elif kind == 1:
            extra[int(rng.integers(0, 6))] = np.inf * (1 if rng.random() < 0.5 else -1)
        elif kind == 2:
            extra[0], extra[3] = extra[3] + 1.0, extra[0]           # inverted
        elif kind == 3:
            extra[:3] -= 1.0e6                                      # swallows the camera: its region cannot be proven
            extra[3:] += 1.0e6
        elif kind == 4:
            extra += np.float32(rng.normal(scale=0.5))              # a box moved elsewhere
        else:
            extra[:3] = extra[3:] = 3.0e38                          # a point at the edge of the float range
        bm, _, _ = bitmap(scene, i, W, H, boxes=np.vstack([boxes, extra[None]]))
        if kind in (0, 1, 2, 3, 5):
            assert bm is None, f"trial {trial} (kind {kind}): a broken box left a bitmap"
        if bm is not None:
            assert not (hit & ~bm).any(), f"trial {trial} (kind {kind}): a hit tile was cleared"
            assert not (good & ~bm).any()                           # more boxes only ever set more bits
        # the broken box IN THE PLACE of one of the mesh's own
        boxes[k] = extra
        bm, _, _ = bitmap(scene, i, W, H, boxes=boxes)
        if kind in (0, 1, 2, 3, 5):
            assert bm is None
