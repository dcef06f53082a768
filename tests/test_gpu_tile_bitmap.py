"""The tile bitmap on the device (csrc/rpt_tile_bitmap.hpp, clear_empty_tiles in csrc/rpt_kernels.hip.h): kernels 41 and 43 with a live
bitmap render what the un-culled kernel renders (rpt_verify_frame), the bitmap is built only after two identical rpt_set_objects calls
and dropped when the camera clock moves, and it really clears tiles the object mask keeps."""
import ctypes as C

import numpy as np
import pytest

from relativitypathtracer_amd import Scene

pytestmark = pytest.mark.gpu

SIZES = [(256, 144), (648, 360)]        # 648 = 81 tiles: a partial last dword in every second row of the bitmap


def state(r, obj=None):
    out = (C.c_uint64 * 4)()
    bits = None
    if obj is not None:
        r._check(r._lib.rpt_tile_bitmap_state(r._h, out, -1, None, 0), "rpt_tile_bitmap_state")
        bits = np.zeros(int(out[3]), dtype=np.uint32)
        r._check(r._lib.rpt_tile_bitmap_state(r._h, out, obj, bits.ctypes.data, bits.size), "rpt_tile_bitmap_state")
    else:
        r._check(r._lib.rpt_tile_bitmap_state(r._h, out, -1, None, 0), "rpt_tile_bitmap_state")
    return [int(x) for x in out], bits


@pytest.fixture(scope="module")
def bunny():
    scene = Scene.from_file("bunny")
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    from relativitypathtracer_amd.renderer import Renderer
    r = Renderer(0)
    r.upload_scene(scene)
    return scene, r


@pytest.mark.parametrize("variant", [41, 43])
@pytest.mark.parametrize("W,H", SIZES)
def test_live_bitmap_changes_no_pixel_and_is_dropped_when_the_clock_moves(bunny, W, H, variant):
    scene, r = bunny
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r.set_scene_params(scene, W, H)
    r.set_variant(variant)
    mesh = [i for i in range(len(scene.objects())) if int(scene.objects()["type"][i]) == 2][0]
    scene.set_camera((0.0, 0.0, 0.0), 0.37)      # a frame of another time first: whatever an earlier case left is dropped
    scene.update_objects()
    r.set_objects(scene)
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r.set_objects(scene)
    assert r.verify_frame() == 0
    st, _ = state(r)
    assert st[0] == 0, "a bitmap after ONE call with these objects"
    builds = st[1]
    r.set_objects(scene)                         # byte-identical a second time: the bitmap goes live with the next frame
    assert r.verify_frame() == 0, f"kernel {r.last_variant()} with the tile bitmap != un-culled"
    assert r.last_variant() == variant
    st, bits = state(r, mesh)
    assert st[0] == 1 << mesh and st[1] == builds + 1
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert st[3] == (tiles + 31) // 32
    set_bits = int(np.unpackbits(bits.view(np.uint8), bitorder="little")[:tiles].sum())
    print(f"{W}x{H} kernel {variant}: {set_bits} of {tiles} tiles set, host build {st[2]} us")
    assert 0 < set_bits < tiles // 4             # the bunny covers a small part of the frame: most tiles are cleared
    r.set_objects(scene)
    assert r.verify_frame() == 0
    assert state(r)[0][1] == builds + 1          # a still view pays once
    scene.set_camera((0.0, 0.0, 0.0), 0.016)     # the camera clock moves: the record changes, the bitmap is dropped
    scene.update_objects()
    r.set_objects(scene)
    assert state(r)[0][0] == 0
    assert r.verify_frame() == 0
    assert state(r)[0][0] == 0


def probe_masks(r, W, H):
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    out = np.zeros(2 * tiles, dtype=np.uint64)
    r._check(r._lib.rpt_probe_tile_masks(r._h, out.ctypes.data, tiles), "rpt_probe_tile_masks")
    out = out.reshape((H + 7) // 8, (W + 7) // 8, 2)
    return out[..., 0], out[..., 1]


def test_the_device_clears_tiles_the_object_mask_keeps(bunny):
    """Not vacuous, observed ON THE DEVICE: rpt_probe_tile_masks forms every tile's object mask with the code kernel 41 runs (the ballot,
    then thin_object_mask<BallotExact>, the function render_pixel_body calls).  Without a live bitmap the two masks are equal; with it
    the mesh's bit is gone from a tenth or more of the tiles that had it, whole waves' masks go to 0, no other bit changes, and the
    cleared tiles are exactly the zero bits of the host's bitmap."""
    from tile_bitmap_helpers import bitmap
    scene, r = bunny
    W, H = 256, 144
    scene.set_camera((0.0, 0.0, 0.0), 0.21)
    scene.update_objects()
    r.set_scene_params(scene, W, H)
    r.set_variant(41)
    r.set_objects(scene)
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r.set_objects(scene)
    before, after = probe_masks(r, W, H)
    assert (before == after).all(), "no bitmap is live after one call with these objects"
    objs = scene.objects()
    mesh = [i for i in range(len(objs)) if int(objs["type"][i]) == 2][0]
    bit = np.uint64(1 << mesh)
    r.set_objects(scene)
    before2, after2 = probe_masks(r, W, H)
    assert (before2 == before).all()
    assert state(r)[0][0] == 1 << mesh
    kept = (before2 & bit) != 0
    still = (after2 & bit) != 0
    assert not (still & ~kept).any() and ((before2 & ~bit) == (after2 & ~bit)).all()       # only the mesh's bit, only ever cleared
    cleared = kept & ~still
    emptied = int(((before2 != 0) & (after2 == 0)).sum())
    print(f"{W}x{H}: the device keeps the mesh in {int(kept.sum())} tiles, the bitmap clears {int(cleared.sum())} of them; {emptied} waves' masks go to 0")
    assert cleared.sum() >= 0.1 * kept.sum() and emptied > 0
    host, _, _ = bitmap(scene, mesh, W, H)
    assert host is not None and (cleared == (kept & ~host)).all()
    assert r.verify_frame() == 0


@pytest.mark.parametrize("what", ["lens", "doppler", "environment"])
def test_live_bitmap_changes_no_pixel_in_the_other_forms(bunny, what):
    """The lens, Doppler and environment forms read the bitmap through the same policy: rpt_verify_frame with it live, and the device's
    masks show that it is."""
    scene, r = bunny
    W, H = 328, 184
    scene.set_camera((0.0, 0.0, 0.0), 0.0)
    scene.update_objects()
    r.set_scene_params(scene, W, H)
    r.set_variant(0)
    try:
        if what == "lens":
            r._check(r._lib.rpt_set_field_of_view(r._h, C.c_float(0.6)), "rpt_set_field_of_view")
        elif what == "doppler":
            r._check(r._lib.rpt_set_doppler(r._h, 3), "rpt_set_doppler")
        else:
            sky = np.random.default_rng(3).integers(0, 256, size=64 * 32 * 3, dtype=np.uint8)
            r._check(r._lib.rpt_set_environment(r._h, sky.ctypes.data, 64, 32), "rpt_set_environment")
        scene.set_camera((0.0, 0.0, 0.0), 0.11)
        scene.update_objects()
        r.set_objects(scene)
        scene.set_camera((0.0, 0.0, 0.0), 0.0)
        scene.update_objects()
        r.set_objects(scene)
        r.set_objects(scene)
        assert r.verify_frame() == 0, f"{what}: kernel {r.last_variant()} with the tile bitmap != un-culled"
        assert state(r)[0][0] != 0
        before, after = probe_masks(r, W, H)
        assert (before != after).any()
        print(f"{what}: kernel {r.last_variant()}, {int((before != after).sum())} tiles thinned")
    finally:
        if what == "lens":
            r._lib.rpt_set_field_of_view(r._h, C.c_float(0.0))
        elif what == "doppler":
            r._lib.rpt_set_doppler(r._h, 0)
        else:
            r._lib.rpt_set_environment(r._h, None, 0, 0)
