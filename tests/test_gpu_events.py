"""rpt_render_events on the MI355X (DESIGN.md "Event pass"): every record bit for bit against tests/native/event_oracle.c through every
camera and kernel form, culled equal to un-culled on thousands of generated scenes, agreement with the colour frame, sharding and frames
in flight, rpt_pick, the refusals, and the default path left as it was."""
import os
import sys

import numpy as np
import pytest

import events_oracle as eo
import oracle_ffi
from relativitypathtracer_amd.events import EVENT_DTYPE
from relativitypathtracer_amd.renderer import RenderError, Renderer, orient_objects

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LATENCY_KERNEL_MAX_PIXELS = 3000000      # RPT_LATENCY_KERNEL_MAX_PIXELS (include/rpt.h)
BIG = (2400, 1256)                       # 3 014 400 pixels: one size above it
YPR = (0.4, -0.25, 0.15)
PANO = dict(h_fov=2.0, v_fov=1.2, yaw=0.3)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("events"))


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def _setup(r, scene, W, H, variant=0, ypr=(0.0, 0.0, 0.0), v_fov=0.0, pano=None, upload=True):
    r.set_variant(variant)
    r.set_msaa(1)
    r.set_doppler(False, False)
    r.set_environment(None)
    r.set_debug_rgb(False)
    r.set_orientation(*ypr)
    r.set_field_of_view(v_fov)
    if pano is None:
        r.set_projection("pinhole")
    else:
        r.set_projection("equirect", **pano)
    if upload:
        r.upload_scene(scene)
    else:
        r.set_objects(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _same(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 32)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 32)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} records differ; first at pixel {k}: got {got.reshape(-1)[k]} want {want.reshape(-1)[k]}")


def _check_against_oracle(r, want, expect_default, what, unculled=903):
    """The records of the context's current state through the default choice and the un-culled form, blocking and async."""
    for variant, expect in ((0, expect_default), (3, unculled)):
        r.set_variant(variant)
        got = r.render_events()
        assert r.last_events_variant() == expect, (what, variant, r.last_events_variant())
        _same(got, want, f"{what} kernel {expect} blocking")
        assert r.render_events(async_=True) is None
        r.sync()
        assert r.last_events_variant() == expect
        _same(r.read_events(), want, f"{what} kernel {expect} async")
    r.set_variant(0)


def _has_mesh(scene):
    return bool((scene.objects()["type"] == 2).any())


# ---- 1. bit for bit against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [-1, 0])
@pytest.mark.parametrize("camera", sorted(eo.CAMERAS))
@pytest.mark.parametrize("name", eo.SHIPPED)
def test_records_equal_the_oracle(renderer, lib, name, camera, interval):
    W, H = 128, 72
    scene = eo.load_scene(name, camera, interval)
    want = eo.oracle_events(lib, scene, W, H)
    _setup(renderer, scene, W, H)
    _check_against_oracle(renderer, want, 941 if _has_mesh(scene) else 944, f"{name} {camera} interval {interval}")


@pytest.mark.parametrize("interval", [-1, 0])
@pytest.mark.parametrize("camera", sorted(eo.CAMERAS))
def test_records_equal_the_oracle_above_the_latency_size(renderer, lib, camera, interval):
    W, H = BIG
    assert W * H > LATENCY_KERNEL_MAX_PIXELS
    scene = eo.load_scene("bunny", camera, interval)
    want = eo.oracle_events(lib, scene, W, H)
    assert (want["object"] >= 0).any()
    _setup(renderer, scene, W, H)
    _check_against_oracle(renderer, want, 941, f"bunny {W}x{H} {camera} interval {interval}")


@pytest.mark.parametrize("name,camera", [("shadows", "0.9c"), ("bunny", "rest"), ("cubes", "rest"), ("arch", "0.9c")])
def test_records_under_an_orientation(renderer, lib, name, camera):
    W, H = 128, 72
    scene = eo.load_scene(name, camera, -1)
    turned = orient_objects(scene, *YPR)
    want = eo.oracle_events(lib, scene, W, H, objects=turned)
    _setup(renderer, scene, W, H, ypr=YPR)
    _check_against_oracle(renderer, want, 941 if _has_mesh(scene) else 944, f"{name} {camera} turned")
    renderer.set_orientation(0.0, 0.0, 0.0)


@pytest.mark.parametrize("name,camera", [("bunny", "rest"), ("shadows", "0.9c"), ("cubes", "rest"), ("arch", "0.9c"), ("soccer", "rest")])
def test_records_in_panorama(renderer, lib, name, camera):
    W, H = 160, 96
    scene = eo.load_scene(name, camera, -1)
    want = eo.oracle_events(lib, scene, W, H, dirs=eo.pano_dirs(W, H, **PANO))
    _setup(renderer, scene, W, H, pano=PANO)
    expect = 911 if _has_mesh(scene) else 914
    _check_against_oracle(renderer, want, expect, f"{name} {camera} panorama", unculled=expect)      # (no un-culled form: variant 3 gets the same kernel)
    renderer.set_projection("pinhole")


@pytest.mark.parametrize("v_fov", [0.3, 2.0])
@pytest.mark.parametrize("name,camera", [("bunny", "rest"), ("shadows", "rest"), ("cubes", "rest"), ("arch", "0.9c")])
def test_records_under_a_lens(renderer, lib, name, camera, v_fov):
    W, H = 128, 72
    scene = eo.load_scene(name, camera, -1)
    want = eo.oracle_events(lib, scene, W, H, dirs=eo.pinhole_dirs(W, H, eo.lens_scale(v_fov)))
    _setup(renderer, scene, W, H, v_fov=v_fov)
    expect = 923 if v_fov == 2.0 else (921 if _has_mesh(scene) else 924)
    _check_against_oracle(renderer, want, expect, f"{name} {camera} lens {v_fov}", unculled=923)
    renderer.set_field_of_view(0.0)


HUGE_OBJ = ("v -2147483648 -2147483648 8589934592\nv 2147483648 -2147483648 8589934592\nv 0 2147483648 8589934592\n"
            "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")      # |e1| |e2| = 2^32 * 2^32.16 > 2^60: outside rcp_exact's domain


def _scene_outside_the_exact_reciprocal_domain(tmp_path, camera):
    """bunny.txt with one more mesh in the scene's pool, named by no object (tests/test_gpu_exact_division.py's construction): its
    triangle alone puts the scene outside the domain, so the walk kernels must run their IEEE-division forms."""
    import ctypes as C
    from relativitypathtracer_amd import Scene, _ffi
    obj = tmp_path / "huge.obj"
    obj.write_text(HUGE_OBJ)
    scene = Scene.from_file("bunny")
    scene.ReadOBJ(str(obj))
    scene.set_interval(-1)
    scene.set_camera(eo.CAMERAS[camera], eo.SCENE_TIMES["bunny"] if camera == "rest" else 0.0)
    scene.update_objects()
    assert _ffi.hip().rpt_scene_exact_rcp(C.byref(scene.desc())) == 0
    return scene


@pytest.mark.parametrize("camera", sorted(eo.CAMERAS))
def test_a_scene_outside_the_exact_reciprocal_domain_gets_the_ieee_forms(renderer, lib, tmp_path, camera):
    """The rule that selects the IEEE forms of 941 / 911 / 921 (a row with an IEEE form, on a scene for which rpt_scene_exact_rcp is 0):
    on a mesh with |e1| |e2| > 2^60 each of the three runs its IEEE form (rpt_last_events_exact_rcp reports 0) and gives the oracle's
    records in all 32 bytes; on bunny.txt itself, inside the domain, the same three report 1, and the kernels with no IEEE form 0."""
    out = _scene_outside_the_exact_reciprocal_domain(tmp_path, camera)
    inside = eo.load_scene("bunny", camera, -1)
    cases = (("pinhole", 128, 72, dict(), None, 941, 903),
             ("panorama", 160, 96, dict(pano=PANO), lambda W, H: eo.pano_dirs(W, H, **PANO), 911, 911),
             ("lens 0.3", 128, 72, dict(v_fov=0.3), lambda W, H: eo.pinhole_dirs(W, H, eo.lens_scale(0.3)), 921, 923))
    for what, W, H, view, dirs, walk, unculled in cases:
        for scene, exact in ((out, False), (inside, True)):
            want = eo.oracle_events(lib, scene, W, H, dirs=dirs(W, H) if dirs else None)
            assert (want["object"] >= 0).any()
            _setup(renderer, scene, W, H, **view)
            got = renderer.render_events()
            assert (renderer.last_events_variant(), renderer.last_events_exact_rcp()) == (walk, exact), (what, exact)
            _same(got, want, f"{what} kernel {walk} exact reciprocal {exact} blocking")
            assert renderer.render_events(async_=True) is None
            renderer.sync()
            assert (renderer.last_events_variant(), renderer.last_events_exact_rcp()) == (walk, exact), (what, exact)
            _same(renderer.read_events(), want, f"{what} kernel {walk} exact reciprocal {exact} async")
            renderer.set_variant(3)              # 903 / 923 have no IEEE form; the panorama's variant 3 is 911 again
            _same(renderer.render_events(), want, f"{what} kernel {unculled}")
            assert (renderer.last_events_variant(), renderer.last_events_exact_rcp()) == (unculled, exact and unculled == walk), what
    _setup(renderer, eo.load_scene("cubes", camera, -1), 128, 72)      # no mesh in Object[]: 944 has no walk at all
    renderer.render_events()
    assert (renderer.last_events_variant(), renderer.last_events_exact_rcp()) == (944, False)
    renderer.set_projection("pinhole")
    renderer.set_field_of_view(0.0)


def test_frames_wider_than_four_to_one_get_the_unculled_kernel(renderer, lib):
    W, H = 520, 64
    scene = eo.load_scene("shadows", "rest", -1)
    want = eo.oracle_events(lib, scene, W, H)
    _setup(renderer, scene, W, H)
    _check_against_oracle(renderer, want, 903, "shadows 520x64")


# ---- 2. culled equals un-culled ---------------------------------------------------------------------------------------------------------
FUZZ_KINDS = ("random", "extreme", "close", "walls", "ellipsoids")      # ellipsoids: spheres scaled into needles and discs
FUZZ_PER_KIND = max(480, int(os.environ.get("RPT_EVENTS_FUZZ_PER_KIND", "480")))      # (a soak run may ask for more, never fewer)


def test_culled_records_equal_unculled_on_generated_scenes(renderer):
    """941 / 944 / 921 / 924 against 903 / 923, record for record, on 5 x 480 generated scenes, each under a random orientation, every
    second one under a random lens.  Only the front end's rejection of a generated scene is caught."""
    import verify_fuzz
    sizes = [(320, 184), (256, 144), (200, 150), (360, 200)]
    total, seen = 0, set()
    for kind in FUZZ_KINDS:
        accepted = 0
        for seed in range(FUZZ_PER_KIND):
            try:
                scene, text = verify_fuzz.build(kind, seed)
            except RuntimeError:         # the front end's rejection of a generated scene (scene.py raises RuntimeError), nothing else
                continue
            accepted += 1
            rng = np.random.default_rng(31000 + seed)
            ypr = tuple(float(a) for a in rng.uniform(-3.0, 3.0, size=3))
            v_fov = float(rng.uniform(0.05, 1.55)) if seed % 2 else 0.0      # tan(v_fov / 2) <= 1: the culled lens kernels
            W, H = sizes[seed % len(sizes)]
            _setup(renderer, scene, W, H, ypr=ypr, v_fov=v_fov)
            culled = renderer.render_events()
            kc = renderer.last_events_variant()
            assert kc in ((921, 924) if v_fov else (941, 944)), (kind, seed, kc)
            renderer.set_variant(3)
            plain = renderer.render_events()
            assert renderer.last_events_variant() == (923 if v_fov else 903)
            _same(culled, plain, f"{kind} seed {seed} {W}x{H} ypr {ypr} v_fov {v_fov} kernel {kc}\n{text}")
            seen.add(kc)
        assert accepted >= (FUZZ_PER_KIND * 3) // 4, f"{kind}: only {accepted} of {FUZZ_PER_KIND} generated scenes were accepted by the front end"
        total += accepted
    assert total >= 2000, total
    assert seen == {941, 944, 921, 924}, seen
    renderer.set_orientation(0.0, 0.0, 0.0)
    renderer.set_field_of_view(0.0)
    renderer.set_variant(0)


# ---- 3. agreement with the colour frame ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eo.SHIPPED)
def test_misses_are_the_background_pixels_and_the_framebuffer_is_not_touched(renderer, lib, name):
    W, H = 128, 72
    scene = eo.load_scene(name, "rest", -1)
    _setup(renderer, scene, W, H)
    renderer.render()
    before = renderer.read_framebuffer().copy()
    colour_variant = renderer.last_variant()
    rec = renderer.render_events()
    after = renderer.read_framebuffer()
    assert before.tobytes() == after.tobytes(), f"{name}: the colour framebuffer changed during an event pass"
    assert renderer.last_variant() == colour_variant
    want = eo.oracle_events(lib, scene, W, H)
    oracle_hit = (want["object"] >= 0)
    miss = rec["object"] == -1
    assert np.array_equal(miss, ~oracle_hit)
    # the packed background: what the oracle gives a pixel whose ray hits nothing
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    assert (~oracle_hit).any()
    bg = opx["rgba"].reshape(H, W, 4)[~oracle_hit][0]
    frame = before["rgba"].reshape(H, W, 4)
    assert (frame[miss] == bg).all(), name
    # a hit pixel may share the background's packed colour by coincidence only where the oracle's frame does too
    same_as_bg = (frame == bg).all(axis=-1)
    assert np.array_equal(same_as_bg & ~miss, (opx["rgba"].reshape(H, W, 4) == bg).all(axis=-1) & oracle_hit)


# ---- 4. sharding and frames in flight --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour_plane", [False, True])
def test_three_contexts_fill_one_external_buffer(lib, colour_plane):
    import torch
    W, H = 200, 150                                  # 19 row tiles, the last one partial
    scene = eo.load_scene("shadows", "rest", -1)
    want = eo.oracle_events(lib, scene, W, H)
    sentinel = 0x5A5A5A5A
    buf = torch.full((W * H * 8,), sentinel, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctxs = [Renderer(0) for _ in range(3)]
    try:
        for k, r in enumerate(ctxs):
            _setup(r, scene, W, H)
            r.set_rows(k, 3, colour_plane)
            r.set_events_output(buf.data_ptr())
        ctxs[0].render_events()
        torch.cuda.synchronize()
        part = buf.cpu().numpy().view(EVENT_DTYPE).reshape(H, W)
        rows0 = (np.arange(H) // 8) % 3 == 0
        _same(part[rows0], want[rows0], "context 0's rows")
        assert (part[~rows0].view(np.int32) == sentinel).all(), "rows that are not this context's were touched"
        for r in ctxs[1:]:
            r.render_events(async_=True)
        for r in ctxs:
            r.sync()
        whole = buf.cpu().numpy().view(EVENT_DTYPE).reshape(H, W)
        _same(whole, want, f"three contexts, colour_plane {colour_plane}")
        # rpt_pick: a row the context owns, one it does not
        assert ctxs[1].pick(5, 8)["object"] == want[8, 5]["object"]
        with pytest.raises(RenderError, match=r"\(1\)"):
            ctxs[1].pick(5, 0)
    finally:
        for r in ctxs:
            r.close()


def test_ring_of_four_shared_contexts_async_equals_blocking():
    W, H = 256, 144
    scene = eo.load_scene("bunny", "rest", -1)
    views = [(0.0, 0.0, 0.0), (0.3, 0.1, 0.0), (-0.4, 0.0, 0.2), (0.1, -0.2, -0.3)]
    ring = [Renderer(0) for _ in views]
    try:
        ring[0].upload_scene(scene)
        for r in ring[1:]:
            r.share_scene(ring[0])
        for r, ypr in zip(ring, views):
            _setup(r, scene, W, H, ypr=ypr, upload=False)
        blocking = [r.render_events().copy() for r in ring]
        for _ in range(3):
            for r in ring:
                r.render_events(async_=True)
        for r in ring:
            r.sync()
        for k, r in enumerate(ring):
            _same(r.read_events(), blocking[k], f"ring slot {k}")
        assert not np.array_equal(blocking[0]["object"], blocking[1]["object"])
    finally:
        for r in ring:
            r.close()


# ---- 5. rpt_pick ------------------------------------------------------------------------------------------------------------------------
def test_pick_equals_the_read_back_record_and_reports_its_statuses():
    W, H = 128, 72
    scene = eo.load_scene("shadows", "rest", -1)
    r = Renderer(0)
    try:
        _setup(r, scene, W, H)
        with pytest.raises(RenderError, match=r"rpt_pick failed \(2\)"):       # RPT_ERR_STATE before the first event frame
            r.pick(3, 3)
        with pytest.raises(RenderError, match=r"rpt_read_events failed \(2\)"):
            r.read_events()
        assert r.last_events_variant() == 0 and not r.last_events_exact_rcp()
        rec = r.render_events()
        rng = np.random.default_rng(7)
        for x, y in zip(rng.integers(0, W, 100), rng.integers(0, H, 100)):
            assert r.pick(int(x), int(y)).tobytes() == rec[y, x].tobytes(), (x, y)
        for x, y in ((-1, 0), (0, -1), (W, 0), (0, H)):
            with pytest.raises(RenderError, match=r"rpt_pick failed \(1\)"):   # RPT_ERR_ARG
                r.pick(x, y)
        r.render()                                  # the context is as usable as before
    finally:
        r.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(r, what):
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_events:") as e:
        r.render_events()
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_events:"):
        r.render_events(async_=True)
    assert what in str(e.value), str(e.value)


def test_refusals_leave_the_context_usable(lib):
    W, H = 128, 72
    scene = eo.load_scene("bunny", "rest", -1)
    want = eo.oracle_events(lib, scene, W, H)
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    r = Renderer(0)
    try:
        _setup(r, scene, W, H)
        r.set_msaa(2)
        _refused(r, "MSAA")
        r.set_msaa(1)
        for variant in (1, 48, 49, 50, 51):
            r.set_variant(variant)
            _refused(r, f"variant {variant}")
        r.set_variant(0)
        r.set_projection("equirect", **PANO)          # a lens together with the panorama: the panorama has fields of view of its own
        r.set_field_of_view(0.3)
        _refused(r, "a lens needs the pinhole")
        r.set_field_of_view(0.0)
        r.set_projection("pinhole")
        r.render()
        assert np.array_equal(r.read_framebuffer()["rgba"], opx["rgba"])
        _same(r.render_events(), want, "after the refusals")
    finally:
        r.close()


def test_a_non_consecutive_octree_is_refused():
    """An octree whose children are not stored consecutively (tests/test_gpu_properties.py's construction: a copy of the root's first
    child appended at the end, the root pointed at it) does not fit the derived layout: colour frames fall back to kernel 1, the event
    pass refuses."""
    from relativitypathtracer_amd import _ffi
    W, H = 128, 72
    scene = eo.load_scene("shadows", "rest", -1)
    oc = scene.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
    root = scene.mesh_roots()[0]
    kids = oc[root, 10:18].copy()
    new = np.vstack([oc, oc[kids[0]][None]])
    new[root, 10] = len(oc)
    d2 = _ffi.SceneDesc.from_buffer_copy(scene.desc())
    raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
    d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    r = Renderer(0)
    try:
        _setup(r, scene, W, H)
        r.upload_desc(d2)
        r.render()
        assert r.last_variant() == 1
        _refused(r, "children not consecutive")
        r.set_variant(3)
        _refused(r, "children not consecutive")
        r.set_variant(0)
        r.render()
        assert np.array_equal(r.read_framebuffer()["rgba"], opx["rgba"])
    finally:
        r.close()


# ---- 7. the default path is untouched ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "cubes"])
def test_rpt_render_is_what_it_was_after_event_passes(renderer, name):
    W, H = 320, 184
    scene = eo.load_scene(name, "rest", -1)
    _setup(renderer, scene, W, H)
    renderer.set_debug_rgb(True)
    renderer.render()
    px, rgb, variant = renderer.read_framebuffer().copy(), renderer.read_debug_rgb().copy(), renderer.last_variant()
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    assert np.array_equal(px["rgba"], opx["rgba"])
    for k in range(5):
        renderer.render_events(async_=bool(k & 1))
    renderer.sync()
    assert renderer.last_variant() == variant
    ms = renderer.last_frame_ms()
    assert ms > 0.0
    renderer.render()
    assert renderer.read_framebuffer().tobytes() == px.tobytes()
    assert renderer.read_debug_rgb().tobytes() == rgb.tobytes()
    assert renderer.last_variant() == variant
    renderer.set_debug_rgb(False)


def test_read_events_keeps_the_shape_of_the_frame_that_was_rendered(renderer, lib):
    """set_scene_params between the pass and the read: the records read back are the rendered frame's, in its shape."""
    W, H = 128, 72
    scene = eo.load_scene("shadows", "rest", -1)
    want = eo.oracle_events(lib, scene, W, H)
    _setup(renderer, scene, W, H)
    renderer.render_events(async_=True)
    renderer.set_scene_params(scene, 200, 150)
    renderer.sync()
    got = renderer.read_events()
    assert got.shape == (H, W)
    _same(got, want, "read after set_scene_params")
    assert renderer.pick(W - 1, H - 1).tobytes() == want[H - 1, W - 1].tobytes()
    big = renderer.render_events()
    assert big.shape == (150, 200)
    _same(big, eo.oracle_events(lib, scene, 200, 150), "the next frame, at the new size")


def test_render_scene_returns_the_records(lib):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 128, 72
    scene = eo.load_scene("cube", "rest", -1)
    px, rgb, rec = render_scene(scene, W, H, events=True)
    assert rgb is None and px.shape == (W * H,)
    _same(rec, eo.oracle_events(lib, scene, W, H), "render_scene(events=True)")
    assert len(render_scene(scene, W, H)) == 2
