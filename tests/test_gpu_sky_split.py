"""The sky split on the device (csrc/rpt_api.hip: launch, csrc/rpt_sky_split.hpp, rpt_sky_fill_kernel): a plain pinhole
frame whose objects lie in a small box of tiles is a fill of everything outside the box plus the frame's own kernel over the box alone.

  * A split frame is the un-culled kernel's frame (variant 3) byte for byte, all 16 bytes of every pixel, both rendered into framebuffers
    filled with 0xAB first — a pixel neither launch wrote would show.
  * rpt_last_sky_split says which path ran, and it ran exactly where the rule says: the box holds every tile with a non-empty object mask
    (rpt_probe_tile_masks) and covers at most half of the frame's tiles; a full-plane rectangle, an empty Object[], a wide union, 65
    objects, the blocking call and every excluded setting keep the single launch (and its frame).
  * The rule's floor — frames in flight of more than 6 000 000 pixels — is checked on the headline frame as it
    stands; every other case runs on a context created with RPT_SKY_SPLIT_MIN_PIXELS=0, the library's way to the small frames where
    a box's placement can go wrong."""
import os

import numpy as np
import pytest

from relativitypathtracer_amd import Scene

pytestmark = pytest.mark.gpu

SMALL_SIZES = [(64, 64), (200, 120), (67, 45), (33, 257)]      # 67x45 and 33x257: partial tiles on both edges
PLACEMENTS = ["middle", "left", "right", "bottom", "top"]      # the cube's centre on the frame's centre / on each edge: its box is clipped there
CUBE_Z = 6.0


def cube_scene(W, H, placement):
    """Scenes/cube.txt's textured cube, half as large, at depth 6: the plane z = 0.5 spans |x| <= 6 W / H, |y| <= 6 there"""
    ex, ey = CUBE_Z * W / H, CUBE_Z
    x, y = {"middle": (0.0, 0.0), "left": (-ex, 0.0), "right": (ex, 0.0), "bottom": (0.0, -ey), "top": (0.0, ey)}[placement]
    s = Scene()
    s.inputScene(f"Oc\n p{x:.6f},{y:.6f},{CUBE_Z},0.6,0,1,0,0.5,0.5,0.5\n t0\nTTextures/box.jpg\nI\nR\n")
    s.set_camera((0.0, 0.0, 0.0), 0.0)
    s.update_objects()
    return s


def renderer(scene, floor=0):
    """a context whose split rule has this pixel floor (read from the environment when the context is created); None: the default"""
    from relativitypathtracer_amd.renderer import Renderer
    saved = os.environ.pop("RPT_SKY_SPLIT_MIN_PIXELS", None)
    try:
        if floor is not None:
            os.environ["RPT_SKY_SPLIT_MIN_PIXELS"] = str(floor)
        r = Renderer(0)
    finally:
        os.environ.pop("RPT_SKY_SPLIT_MIN_PIXELS", None)
        if saved is not None:
            os.environ["RPT_SKY_SPLIT_MIN_PIXELS"] = saved
    r.upload_scene(scene)
    return r


def frame(r, W, H, variant=0, blocking=False):
    """One frame of `variant` into a framebuffer of 0xAB bytes: (bytes [H, W, 16], rpt_last_sky_split, rpt_last_variant)"""
    import torch
    buf = torch.full((H * W * 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.set_output(buf.data_ptr())
    r.set_variant(variant)
    try:
        if blocking:
            r.render()
        else:
            r.render_async()
            r.sync()
        split, ran = r.last_sky_split(), r.last_variant()
    finally:
        r.set_output(None)
        r.set_variant(0)
    return buf.cpu().numpy().reshape(H, W, 16), split, ran


def probe_masks(r, W, H):
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    out = np.zeros(2 * tiles, dtype=np.uint64)
    r._check(r._lib.rpt_probe_tile_masks(r._h, out.ctypes.data, tiles), "rpt_probe_tile_masks")
    out = out.reshape((H + 7) // 8, (W + 7) // 8, 2)
    return out[..., 0], out[..., 1]


def check_box(r, W, H, box):
    """the rule's two halves as the device sees them: no tile outside the box has an object in its mask; the box is at most half the frame"""
    tx, ty = (W + 7) // 8, (H + 7) // 8
    x0, y0, x1, y1 = box
    assert 0 <= x0 < x1 <= tx and 0 <= y0 < y1 <= ty, box
    before, _ = probe_masks(r, W, H)
    outside = before != 0
    outside[y0:y1, x0:x1] = False
    assert not outside.any(), f"tile (x, y) = {np.argwhere(outside)[0][::-1]} outside the box {box} has objects in its mask"
    assert (before != 0).any() and 2 * (x1 - x0) * (y1 - y0) <= tx * ty
    return before


def same_frame(got, want, what):
    differing = np.argwhere((got != want).any(axis=2))
    assert differing.size == 0, f"{what}: {len(differing)} pixels differ, the first at (y, x) = {tuple(differing[0])}: {got[tuple(differing[0])].tolist()} != {want[tuple(differing[0])].tolist()}"


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("W,H", SMALL_SIZES)
def test_a_split_cube_frame_is_the_unculled_frame(W, H, placement):
    scene = cube_scene(W, H, placement)
    r = renderer(scene)
    try:
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        want, none, ran3 = frame(r, W, H, 3)
        assert none is None and ran3 == 3
        assert (want.view(np.uint32)[..., 3] == 0).all() and (want[..., 8:12] != 0xAB).any()
        got, box, ran = frame(r, W, H)
        assert ran == 44, "a frame without a mesh: kernel 44, split or not"
        assert box is not None, "a small cube on a frame: the rule splits"
        check_box(r, W, H, box)
        print(f"{W}x{H} cube {placement}: box {box} of {(W + 7) // 8} x {(H + 7) // 8} tiles")
        same_frame(got, want, f"kernel 44 split at {box}")
        if placement in ("middle", "right"):      # the blocking call keeps the single launch (§6.2d's A/B): the same frame
            got_b, box_b, ran_b = frame(r, W, H, blocking=True)
            assert ran_b == 44 and box_b is None
            same_frame(got_b, want, "the blocking call")
    finally:
        r.close()


@pytest.fixture(scope="module")
def bunny():
    scene = Scene.from_file("bunny")
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r = renderer(scene)
    yield scene, r
    r.close()


@pytest.mark.parametrize("variant", [41, 48, 0, 43, 49])
def test_bunny_still_for_three_frames_then_moved(bunny, variant):
    """640x360: the bitmap of the still mesh goes live with the third identical Object[] (tests/test_gpu_tile_bitmap.py), inside the box.
    Kernels 41 and 48 split; the band-first kernels 43 and 49 — variant 0 on a frame this small is 43 — never do, whatever the floor."""
    scene, r = bunny
    W, H = 640, 360
    r.set_scene_params(scene, W, H)
    for t in (0.29, 0.0, 0.0, 0.0, 0.016):      # another time first (drops what an earlier case left), three still frames, then the clock moves
        scene.set_camera((0.0, 0.0, 0.0), t)
        scene.update_objects()
        r.set_objects(scene)
        want, _, _ = frame(r, W, H, 3)
        got, box, ran = frame(r, W, H, variant)
        assert ran == (43 if variant == 0 else variant)      # (a small frame in flight waits for latency: 43)
        if ran in (41, 48):
            assert box is not None, "the bunny and its light cover a small part of the frame"
            check_box(r, W, H, box)
        else:
            assert box is None, f"kernel {ran} is never split"
        same_frame(got, want, f"kernel {ran} at t = {t}, box {box}")
    before, after = probe_masks(r, W, H)
    assert (before == after).all(), "the clock moved: no bitmap is live"
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()


def test_the_default_floor_on_the_headline_frame():
    """A context as a caller gets it: the headline frame (3840x2160, four in flight in bench.py) splits and renders kernel 41's frame,
    the blocking call and frames of no more than 6 000 000 pixels do not."""
    scene = Scene.from_file("bunny")
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r = renderer(scene, floor=None)
    try:
        W, H = 3840, 2160
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        want, _, _ = frame(r, W, H, 3)
        got, box, ran = frame(r, W, H)
        assert ran == 41 and box is not None
        check_box(r, W, H, box)
        print(f"{W}x{H} bunny: box {box} of {(W + 7) // 8} x {(H + 7) // 8} tiles")
        same_frame(got, want, f"kernel 41 split at {box}")
        got, box, ran = frame(r, W, H, blocking=True)
        assert ran == 43 and box is None
        same_frame(got, want, "the blocking call")
        W, H = 1920, 1080
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        _, box, ran = frame(r, W, H)
        assert ran == 43 and box is None, "2 Mpx in flight: the latency kernel, one launch"
        W, H = 3200, 1800
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        _, box, ran = frame(r, W, H)
        assert ran == 41 and box is None, "5.8 Mpx in flight: the throughput kernel, still one launch (level in the A/B of DESIGN.md §6.2d)"
    finally:
        r.close()


def test_a_16k_frame_in_flight_is_the_unculled_frame():
    """15360x8640, 2.1 GB of framebuffer: the largest frame the suite renders (tests/test_gpu_properties.py), where a pixel's byte offset
    comes within 2 % of 2^31.  Compared on the device; both framebuffers are filled and the fill awaited before a launch."""
    import torch
    scene = Scene.from_file("bunny")
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r = renderer(scene, floor=None)
    bufs, boxes = [], []
    try:
        W, H = 15360, 8640
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        for variant in (0, 3):
            buf = torch.full((H * W * 4,), -0x54545455, dtype=torch.int32, device="cuda:0")      # 0xAB bytes
            torch.cuda.synchronize()
            r.set_output(buf.data_ptr())
            r.set_variant(variant)
            r.render_async()
            r.sync()
            boxes.append((r.last_variant(), r.last_sky_split()))
            r.set_output(None)
            bufs.append(buf)
        r.set_variant(0)
        assert boxes[0][0] == 41 and boxes[0][1] is not None and boxes[1] == (3, None), boxes
        check_box(r, W, H, boxes[0][1])
        differing = int((bufs[0] != bufs[1]).view(H * W, 4).any(dim=1).sum())
        assert differing == 0, f"{differing} pixels differ between kernel 41 split at {boxes[0][1]} and the un-culled kernel"
        xy = bufs[0].view(H, W, 4)[..., :2].view(torch.float32)
        assert bool((xy[..., 0] == torch.arange(W, device="cuda:0", dtype=torch.float32)[None, :]).all())
        assert bool((xy[..., 1] == torch.arange(H, device="cuda:0", dtype=torch.float32)[:, None]).all())
    finally:
        bufs.clear()
        torch.cuda.empty_cache()
        r.close()


def test_the_camera_inside_the_bunnys_root_box_keeps_the_single_launch(bunny):
    scene, r = bunny
    W, H = 200, 120
    objs = scene.objects()
    mesh = [i for i in range(len(objs)) if int(objs["type"][i]) == 2][0]
    root = scene.octrees()[int(objs["meshIndex"][mesh])]
    centre = np.append((root["min"][:3] + root["max"][:3]) / 2, 1.0)
    world = objs["M"][mesh][:3] @ centre            # transformPoint: rows of M times (x, y, z, 1)
    try:
        scene.set_camera((0.0, 0.0, 0.0), 0.0, position=tuple(float(v) for v in world))
        scene.update_objects()
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        before, _ = probe_masks(r, W, H)
        assert ((before >> np.uint64(mesh)) & np.uint64(1)).all(), "the case is not what it claims: the mesh's region is not the full plane"
        want, _, _ = frame(r, W, H, 3)
        got, box, ran = frame(r, W, H)
        assert box is None and ran == 43
        same_frame(got, want, "the single launch")
    finally:
        scene.set_camera((0.0, 0.0, 0.0), 0.0)
        scene.update_objects()


def test_an_empty_object_list_keeps_the_single_launch(bunny):
    scene, r = bunny
    W, H = 67, 45
    r.set_scene_params(scene, W, H)
    r.set_objects(np.zeros(0, dtype=np.uint8))
    try:
        want, _, _ = frame(r, W, H, 3)
        got, box, _ = frame(r, W, H)
        assert box is None
        same_frame(got, want, "no objects")
        assert (got.view(np.uint32)[..., 2] == got.view(np.uint32)[0, 0, 2]).all(), "every pixel is the background"
    finally:
        r.set_objects(scene)


def test_cubes_wide_union_keeps_the_single_launch():
    """Scenes/cubes.txt: 34 objects strung across the frame.  Stated from the device's masks, not from a copy of the host's arithmetic: the
    host's box holds the masks' bounding box grown by a tile, so where that alone is beyond half of the frame the rule must refuse."""
    scene = Scene.from_file("cubes")
    scene.set_camera((0.3, 0.0, 0.1), 3.0)
    scene.update_objects()
    r = renderer(scene)
    try:
        W, H = 200, 120
        tx, ty = (W + 7) // 8, (H + 7) // 8
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        before, _ = probe_masks(r, W, H)
        ys, xs = np.nonzero(before != 0)
        grown = (min(xs.max() + 2, tx) - max(xs.min() - 1, 0)) * (min(ys.max() + 2, ty) - max(ys.min() - 1, 0))
        print(f"cubes {W}x{H}: the masks' bounding box grown by a tile covers {grown} of {tx * ty} tiles")
        assert 2 * grown > tx * ty, "the case is not what it claims: the union of the cubes' regions is not wide"
        want, _, _ = frame(r, W, H, 3)
        got, box, ran = frame(r, W, H)
        assert box is None and ran == 44
        same_frame(got, want, "the single launch")
    finally:
        r.close()


def _lens(r, W, H):
    r.set_field_of_view(1.2)


def _equirect(r, W, H):
    r.set_projection("equirect")


def _raymap(r, W, H):
    r.set_raymap(r.raymap("fisheye", W, H, fov=2.0))
    r.set_projection("raymap")


def _environment(r, W, H):
    y, x = np.mgrid[0:16, 0:32]
    r.set_environment(np.stack([x * 8, y * 16, (x + y) * 5], axis=2).astype(np.uint8))


def _msaa(r, W, H):
    r.set_msaa(2)


def _doppler_debug(r, W, H):
    r.set_doppler(True, True)
    r.set_debug_doppler(True)


def _doppler(r, W, H):
    r.set_doppler(True, True)


def _debug_rgb(r, W, H):
    r.set_debug_rgb(True)


def _aa(r, W, H):
    r.set_adaptive_aa(2, 8)


EXCLUDED = {"lens": _lens, "equirect": _equirect, "raymap": _raymap, "environment": _environment, "msaa": _msaa, "doppler_debug": _doppler_debug,
            "doppler": _doppler, "debug_rgb": _debug_rgb, "adaptive_aa": _aa}


@pytest.mark.parametrize("setting", sorted(EXCLUDED))
def test_excluded_settings_keep_the_single_launch(setting):
    """The cube that splits in the first test, with one excluded setting each: one launch, and the frame of that setting's un-culled kernel"""
    W, H = 200, 120
    scene = cube_scene(W, H, "middle")
    r = renderer(scene)
    try:
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        _, box, _ = frame(r, W, H)
        assert box is not None, "without the setting this frame splits"
        EXCLUDED[setting](r, W, H)
        want, none, _ = frame(r, W, H, 3)
        got, box, ran = frame(r, W, H)
        assert none is None and box is None, f"{setting}: kernel {ran} was split at {box}"
        same_frame(got, want, f"{setting}: kernel {ran}")
        if setting == "debug_rgb":
            rgb = r.read_debug_rgb()
            assert np.isfinite(rgb).all() and (rgb[0, 0] > 0).all(), "a miss pixel's triple is the mapped background"
    finally:
        r.close()


def test_a_sharded_context_and_65_objects_keep_the_single_launch():
    W, H = 200, 120
    scene = cube_scene(W, H, "middle")
    r = renderer(scene)
    try:
        r.set_scene_params(scene, W, H)
        r.set_objects(scene)
        _, box, _ = frame(r, W, H)
        assert box is not None
        # 65 copies of the cube: beyond the mask's 64 bits
        r.set_objects(np.tile(scene.objects().view(np.uint8).reshape(-1)[:320], 65))
        want, _, _ = frame(r, W, H, 3)
        got, box, ran = frame(r, W, H)
        assert box is None and ran == 44
        same_frame(got, want, "65 objects")
        r.set_objects(scene)
        # a rank's share of the rows, as a colour plane
        r.set_rows(1, 2, colour_plane=True)
        r.render_async()
        r.sync()
        assert r.last_sky_split() is None
        assert r.verify_frame() == 0
        r.set_rows(0, 2, colour_plane=False)        # every second tile row, into the framebuffer
        want, _, _ = frame(r, W, H, 3)
        got, box, _ = frame(r, W, H)
        assert box is None
        same_frame(got, want, "rows 0, 2, 4, ...")
        ours = np.zeros(H, dtype=bool)
        for t in range(0, (H + 7) // 8, 2):
            ours[t * 8:t * 8 + 8] = True
        assert (got[~ours] == 0xAB).all(), "rows of another rank were written"
    finally:
        r.close()
