"""The free-look camera on the MI355X (rpt_set_orientation, rpt_set_field_of_view; DESIGN.md "Free-look camera"): defaults untouched, the
lens kernels at 90 degrees equal to the plain ones, turned and zoomed frames bit for bit against the CPU oracle fed the same rays and the
objects of rpt_orient_objects (tests/native/panorama_oracle.c, as it stands), the panorama with pitch and roll, the refusals, the culls
under orientation and zoom on generated scenes, row tiles and frames in flight."""
import math
import os
import sys
import time

import numpy as np
import pytest

from conftest import CONFIGS, load_config
from relativitypathtracer_amd import Scene
from relativitypathtracer_amd.renderer import RenderError, Renderer, look_at, orient_matrix, orient_objects
from test_camera_view import VIEWS, lens_dirs, oracle_rays, ray_oracle  # noqa: F401  (ray_oracle: the fixture)
from test_gpu_panorama import pano_dirs

pytestmark = pytest.mark.gpu
HALF_PI = float(np.float32(math.pi / 2))
LENS_OF = {3: 803, 41: 841, 43: 843, 44: 844}
# (yaw, pitch, roll), v_fov or None: a look-back, a pitch-up with roll, a zoom-in below 20 degrees, a wide lens above 90 degrees
SHOTS = [((math.pi, 0.0, 0.0), None), ((0.3, 0.5, 0.4), None), ((0.1, -0.05, 0.0), 0.3), ((-0.4, 0.2, 0.0), 2.0)]


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def _plain(r, scene, W, H, variant=0):
    r.set_variant(variant)
    r.set_msaa(1)
    r.set_projection("pinhole")
    r.set_doppler(False, False)
    r.set_debug_doppler(False)
    r.set_environment(None)
    r.set_environment_frame(None)
    r.set_orientation(0, 0, 0)
    r.set_field_of_view(0)
    r.upload_scene(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_debug_rgb(True)


def _frame(r, in_flight=False):
    if in_flight:
        r.render_async()
        r.sync()
    else:
        r.render()
    return r.read_framebuffer().copy(), r.read_debug_rgb().copy(), r.last_variant(), r.last_exact_rcp()


def _same(a, b, what):
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), f"{what}: {int(np.sum(a[0]['rgba'] != b[0]['rgba']))} colour bytes differ"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: debug_rgb differs"


def _config(name, v=None, interval=None):
    c = CONFIGS[name]
    s = Scene.from_file(c["scene"])
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(c["v"] if v is None else v, c["t"])
    s.update_objects()
    return s


# ---- 6. defaults ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_defaults_are_untouched_and_come_back(name):
    W, H = 320, 184
    scene = load_config(name)
    fresh, used = Renderer(0), Renderer(0)
    try:
        fresh.upload_scene(scene)
        fresh.set_scene_params(scene, W, H)
        fresh.set_output(None)
        fresh.set_debug_rgb(True)
        want = [_frame(fresh), _frame(fresh, in_flight=True)]
        assert want[0][2] in (41, 43, 44, 1)
        used.set_orientation(0.7, -0.3, 1.1)
        used.set_field_of_view(0.6)
        used.upload_scene(scene)
        used.set_scene_params(scene, W, H)
        used.set_output(None)
        used.set_debug_rgb(True)
        turned = _frame(used)
        assert turned[2] in (841, 843, 844)
        assert not np.array_equal(turned[0]["rgba"], want[0][0]["rgba"])
        used.set_orientation(0, 0, 0)           # after the objects: re-derived at once
        used.set_field_of_view(0)
        for k, in_flight in enumerate((False, True)):
            got = _frame(used, in_flight)
            _same(got, want[k], f"{name} after reset")
            assert got[2:] == want[k][2:]
    finally:
        fresh.close()
        used.close()


# ---- 7. the lens kernels at 90 degrees are the plain kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_lens_at_90_degrees_is_the_reference_frame(renderer, name):
    W, H = 384, 216
    scene = load_config(name)
    for variant, in_flight in ((0, False), (41, True), (43, False), (44, False), (3, False)):
        _plain(renderer, scene, W, H, variant)
        want = _frame(renderer, in_flight)
        renderer.set_field_of_view(HALF_PI)
        got = _frame(renderer, in_flight)
        _same(got, want, f"{name} variant {variant}")
        assert got[2] == LENS_OF[want[2]] and got[3] == want[3], (name, variant, got[2:], want[2:])
        assert renderer.verify_frame() == 0
    renderer.set_field_of_view(0)


# ---- 8. parity with the oracle -------------------------------------------------------------------------------------------------------
def _expect(lib, scene, W, H, ypr, v_fov, rows=None):
    dirs = lens_dirs(W, H, HALF_PI if v_fov is None else v_fov)
    return oracle_rays(lib, scene, W, H, dirs, orient_objects(scene, *ypr))


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("speed", [0.0, 0.9])
@pytest.mark.parametrize("interval", [-1, 0])
def test_views_equal_the_oracle(renderer, ray_oracle, name, speed, interval):
    W, H = 256, 144
    scene = _config(name, v=(0.0, 0.0, speed), interval=interval)
    has_mesh = bool((scene.objects()["type"] == 2).any())
    for ypr, v_fov in SHOTS:
        opx, orgb = _expect(ray_oracle, scene, W, H, ypr, v_fov)
        wide = v_fov is not None and v_fov > HALF_PI
        # the blocking call (43's form, or 44's on a scene without a mesh), 41's form, the un-culled kernel
        for variant, in_flight in ((0, False), (41, True), (3, False)):
            _plain(renderer, scene, W, H, variant)
            renderer.set_orientation(*ypr)
            renderer.set_field_of_view(0 if v_fov is None else v_fov)
            px, rgb, kernel, _ = _frame(renderer, in_flight)
            what = f"{name} v={speed} interval={interval} view {ypr} fov {v_fov} variant {variant} (kernel {kernel})"
            base = 3 if (variant == 3 or wide) else (41 if variant == 41 else (43 if has_mesh else 44))
            assert kernel == (base if v_fov is None else LENS_OF[base]), what
            assert np.array_equal(px.view(np.uint8), opx.view(np.uint8)), f"{what}: {int(np.sum(px['rgba'] != opx['rgba']))} colour bytes differ"
            assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32)), what
    renderer.set_orientation(0, 0, 0)
    renderer.set_field_of_view(0)


@pytest.mark.parametrize("name", ["bunny", "shadows"])
def test_in_flight_call_above_the_latency_limit(renderer, ray_oracle, name):
    """rpt_render_async on more than RPT_LATENCY_KERNEL_MAX_PIXELS pixels: 41's lens form, against the oracle on every 16th row."""
    W, H = 2560, 1280
    scene = load_config(name)
    ypr, v_fov = (0.2, 0.1, -0.3), 0.9
    _plain(renderer, scene, W, H)
    renderer.set_orientation(*ypr)
    renderer.set_field_of_view(v_fov)
    px, rgb, kernel, _ = _frame(renderer, in_flight=True)
    assert kernel == 841
    dirs, objs = lens_dirs(W, H, v_fov), orient_objects(scene, *ypr)
    px, rgb = px.reshape(H, W), rgb
    for y in range(0, H, 16):
        opx, orgb = oracle_rays(ray_oracle, scene, W, H, dirs, objs, rows=(y, y + 1))
        assert np.array_equal(px[y].view(np.uint8), opx.reshape(H, W)[y].view(np.uint8)), f"{name} row {y}"
        assert np.array_equal(rgb[y].view(np.uint32), orgb[y].view(np.uint32)), f"{name} row {y}"
    renderer.set_orientation(0, 0, 0)
    renderer.set_field_of_view(0)


@pytest.mark.parametrize("name", ["arch", "cubes", "bunny", "shadows"])
def test_doppler_and_sky_under_a_turned_head(renderer, name):
    """Orientation with Doppler and with a sky at rest in the scene: the turned context equals, bit for bit, a plain context handed the
    objects of rpt_orient_objects and the E of rpt_orient_matrix (those kernels are held to the Doppler model and to the sky's oracle by
    their own tests): a turned head sees the sky turn with the scene.  The lens forms at 90 degrees equal them too, and under a zoom the
    culled lens kernels agree with the un-culled one."""
    W, H = 320, 184
    scene = _config(name, v=(0.0, 0.0, 0.9), interval=-1)
    rng = np.random.default_rng(3)
    sky = rng.integers(0, 256, size=(64, 128, 3), dtype=np.uint8)
    E = scene.camera_lorentz()[1]
    ypr = (2.5, 0.4, -0.6)
    for doppler, env in (((True, True), False), ((False, False), True), ((True, False), True)):
        _plain(renderer, scene, W, H)
        renderer.set_doppler(*doppler)
        if env:
            renderer.set_environment(sky)
            renderer.set_environment_frame(orient_matrix(E, *ypr))
        renderer.set_objects(orient_objects(scene, *ypr))
        want = _frame(renderer)
        renderer.set_environment_frame(E if env else None)
        renderer.set_objects(scene)
        straight = _frame(renderer)
        assert not np.array_equal(straight[0]["rgba"], want[0]["rgba"])
        renderer.set_orientation(*ypr)
        got = _frame(renderer)
        _same(got, want, f"{name} doppler {doppler} sky {env}")
        assert got[2] == want[2]
        renderer.set_field_of_view(HALF_PI)
        lens = _frame(renderer)
        _same(lens, want, f"{name} doppler {doppler} sky {env}, lens kernels")
        assert lens[2] == want[2] % 100 + (820 if env else 810), (lens[2], want[2])
        renderer.set_field_of_view(0.5)
        assert renderer.verify_frame() == 0
        assert renderer.last_variant() == lens[2]
    _plain(renderer, scene, W, H)


# ---- 9. panorama, refusals, the wide lens ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "cubes", "shadows"])
def test_panorama_with_pitch_and_roll(renderer, ray_oracle, name):
    W, H = 384, 192
    scene = load_config(name)
    ypr, proj = (0.5, 0.7, -0.9), dict(h_fov=4.0, v_fov=2.0, yaw=0.6)
    for variant in (0, 3):
        _plain(renderer, scene, W, H, variant)
        renderer.set_projection("equirect", **proj)
        renderer.set_orientation(*ypr)
        px, rgb, kernel, _ = _frame(renderer)
        assert kernel in ((341, 344) if variant == 0 else (303,))
        opx, orgb = oracle_rays(ray_oracle, scene, W, H, pano_dirs(W, H, **proj), orient_objects(scene, *ypr))
        assert np.array_equal(px.view(np.uint8), opx.view(np.uint8)), f"{name} variant {variant}"
        assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32))
    _plain(renderer, scene, W, H)


def test_refusals_and_the_wide_lens(renderer):
    W, H = 256, 144
    scene = load_config("bunny")
    _plain(renderer, scene, W, H)
    lib, h = renderer._lib, renderer._h
    for bad in (0.009, 3.01, -1.0, float("nan"), float("inf")):
        with pytest.raises(RenderError, match="0.01 <= v_fov <= 3.0"):
            renderer.set_field_of_view(bad)
    for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, float("-inf"))):
        with pytest.raises(RenderError, match="finite"):
            renderer.set_orientation(*bad)
    assert lib.rpt_set_orientation(h, None) == 0
    renderer.set_field_of_view(0.01)
    renderer.set_field_of_view(3.0)
    renderer.render()
    assert renderer.last_variant() == 803                 # wider than the proven window: the un-culled lens kernel
    renderer.set_field_of_view(HALF_PI + 1e-3)
    renderer.render()
    assert renderer.last_variant() == 803
    renderer.set_field_of_view(1.0)
    renderer.render()
    assert renderer.last_variant() == 843

    def refused(match, calls=None):
        for call in calls or (renderer.render, renderer.render_async, renderer.verify_frame):
            with pytest.raises(RenderError, match=match):
                call()
    renderer.set_projection("equirect")
    refused("rpt_set_field_of_view: the panorama")
    renderer.set_projection("pinhole")
    renderer.set_msaa(2)
    refused("rpt_set_field_of_view: MSAA")
    renderer.set_msaa(1)
    for v in (1, 48, 49, 50, 51):
        renderer.set_variant(v)
        refused(f"rpt_set_field_of_view: variant {v} has no lens kernel")
    renderer.set_variant(0)
    renderer.set_doppler(True, True)
    renderer.set_debug_doppler(True)
    refused("rpt_set_field_of_view: the Doppler debug kernel", (renderer.render, renderer.render_async))
    # rpt_verify_frame never launches the record kernel: it sets the hook aside and compares the twins, with a lens as without
    assert renderer.verify_frame() == 0 and renderer.last_variant() == 853
    renderer.set_debug_doppler(False)
    renderer.render()
    assert renderer.last_variant() == 853
    renderer.set_doppler(False, False)
    # orientation alone is refused nowhere: it changes no kernel choice
    renderer.set_field_of_view(0)
    renderer.set_orientation(1, 2, 3)
    for v, want in ((1, 1), (48, 48), (50, 50), (0, 43)):
        renderer.set_variant(v)
        renderer.render()
        assert renderer.last_variant() == want
    renderer.set_msaa(2)
    renderer.render()
    assert renderer.last_variant() == 46
    _plain(renderer, scene, W, H)
    renderer.render()
    assert renderer.last_variant() == 43


def test_octree_with_scattered_children_refuses_the_lens(renderer):
    """An octree whose children are not consecutive (test_gpu_properties' construction) gets kernel 1, which has no lens form;
    orientation alone still renders it."""
    from relativitypathtracer_amd import _ffi
    W, H = 128, 72
    shadows = load_config("shadows")
    _plain(renderer, shadows, W, H)
    oc = shadows.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
    root = shadows.mesh_roots()[0]
    new = np.vstack([oc, oc[oc[root, 10]][None]])
    new[root, 10] = len(oc)
    d2 = _ffi.SceneDesc.from_buffer_copy(shadows.desc())
    raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
    d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
    renderer.set_orientation(0.3, 0.1, 0)
    renderer.upload_desc(d2)
    renderer.set_scene_params(shadows, W, H)
    renderer.render()
    assert renderer.last_variant() == 1
    renderer.set_field_of_view(1.0)
    with pytest.raises(RenderError, match="rpt_set_field_of_view: the lens kernels need the derived octree layout"):
        renderer.render()
    _plain(renderer, shadows, W, H)


# ---- 10. the culls under orientation and zoom --------------------------------------------------------------------------------------
def test_culls_change_nothing_on_generated_scenes(renderer):
    """rpt_verify_frame == 0 on generated scenes of every generator, each with a random orientation, every second one with a random
    v_fov <= pi/2, for the kernel selections (0 blocking, 0 in flight = 41's form, 44).  Seeds rotate from day to day (RPT_SOAK_DAY
    overrides, RPT_VIEW_SCENES the count per generator); a differing pixel is to be diagnosed from the printed seed."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import verify_fuzz
    day = int(os.environ.get("RPT_SOAK_DAY", time.time() // 86400))
    per_kind = int(os.environ.get("RPT_VIEW_SCENES", "350"))
    kinds = ("random", "extreme", "close", "walls", "ellipsoids", "meshwalls")
    print(f"rotating seeds: RPT_SOAK_DAY={day}, seeds {300000 + (day * per_kind) % 400000} .. +{per_kind - 1} of {kinds}")
    done = zoomed = 0
    kernels = set()
    for kind in kinds:
        for k in range(per_kind):
            seed = 300000 + (day * per_kind + k) % 400000
            try:
                scene, text = verify_fuzz.build(kind, seed)
            except RuntimeError:         # the front end's rejection of a generated scene, nothing else
                continue
            rng = np.random.default_rng(seed)
            ypr = tuple(float(a) for a in rng.uniform(-math.pi, math.pi, size=3))
            v_fov = float(rng.uniform(0.02, HALF_PI)) if k % 2 else 0.0
            W, H = [(320, 184), (256, 144), (200, 150), (640, 360)][seed % 4]
            renderer.set_orientation(*ypr)
            renderer.set_field_of_view(v_fov)
            renderer.upload_scene(scene)
            renderer.set_scene_params(scene, W, H)
            for variant in (0, 41, 44):
                renderer.set_variant(variant)
                n = renderer.verify_frame()
                kernels.add(renderer.last_variant())
                assert n == 0, (f"rpt_verify_frame: kernel {renderer.last_variant()} (variant {variant}) != un-culled on {n} pixels: {kind} seed {seed} "
                                f"(RPT_SOAK_DAY={day}) view {ypr} v_fov {v_fov} {W}x{H}\n{text}")
            done += 1
            zoomed += 1 if v_fov else 0
    renderer.set_variant(0)
    renderer.set_orientation(0, 0, 0)
    renderer.set_field_of_view(0)
    print(f"{done} scenes ({zoomed} zoomed), kernels {sorted(kernels)}")
    # (RPT_VIEW_SCENES below 350 is a local knob for a quick look: the suite's own run asks for the 2 000)
    assert done >= (2000 if per_kind >= 350 else 1) and {841, 843, 844, 41, 43, 44} <= kernels


# ---- 11. row tiles and frames in flight ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "cubes"])
def test_row_shards_and_a_ring_of_views(name):
    W, H = 320, 200
    scene = load_config(name)
    views = [((0.4, 0.2, 0.1), 0.8), ((math.pi, 0.0, 0.0), 0.0), ((-0.9, -0.3, 1.0), 1.2), ((0.0, 0.0, 0.0), 0.0)]
    owner = Renderer(0)
    ring = [owner] + [Renderer(0) for _ in range(3)]
    shards = [Renderer(0) for _ in range(3)]
    try:
        owner.set_orientation(*views[0][0])
        owner.set_field_of_view(views[0][1])
        owner.upload_scene(scene)
        for r, (ypr, fov) in zip(ring[1:], views[1:]):
            r.set_orientation(*ypr)
            r.set_field_of_view(fov)
            r.share_scene(owner)               # the owner's objects as given to it: this slot applies its own view
        for r in ring:
            r.set_scene_params(scene, W, H)
            r.set_output(None)
        for _ in range(2):                     # two laps: per-frame rpt_set_objects in every slot, all in flight together
            for r in ring:
                r.set_objects(scene)
                r.render_async()
        frames = []
        for r in ring:
            r.sync()
            frames.append(r.read_framebuffer().copy())
        single = Renderer(0)
        try:
            single.upload_scene(scene)
            single.set_scene_params(scene, W, H)
            single.set_output(None)
            for (ypr, fov), got in zip(views, frames):
                single.set_orientation(*ypr)
                single.set_field_of_view(fov)
                single.render()
                assert np.array_equal(single.read_framebuffer().view(np.uint8), got.view(np.uint8)), (name, ypr, fov)
            assert not np.array_equal(frames[0]["rgba"], frames[1]["rgba"]) and not np.array_equal(frames[1]["rgba"], frames[3]["rgba"])
            # a 3-way shard of the first view equals the whole frame
            whole = np.ascontiguousarray(frames[0]["rgba"]).view(np.uint32).reshape(H, W)
            for k, r in enumerate(shards):
                r.set_orientation(*views[0][0])
                r.set_field_of_view(views[0][1])
                r.share_scene(owner)
                r.set_scene_params(scene, W, H)
                r.set_rows(k, 3, True)
                r.render()
                plane = r.read_colour_plane()
                tiles = (H + 7) // 8
                for t, g in enumerate(range(k, tiles, 3)):
                    rows = min(8, H - 8 * g)
                    assert np.array_equal(plane[8 * t:8 * t + rows], whole[8 * g:8 * g + rows]), (name, k, g)
        finally:
            single.close()
    finally:
        for r in ring + shards:
            r.close()
