"""rpt_set_raymap on the MI355X (DESIGN.md "Ray-map camera"): the ray-map kernels' frames bit for bit against the CPU references fed the
uploaded map (tests/native/*.c take the camera ray per pixel), the pixels without a ray, the pinhole's and the panorama's own directions
through the map against those cameras' kernels, aberration in a fisheye, the culls, and the plumbing."""
import ctypes as C
import math

import numpy as np
import pytest

import doppler_oracle
import events_oracle
import oracle_ffi
import raymap_cases as rc
from relativitypathtracer_amd import Scene, _ffi
from relativitypathtracer_amd.events import EVENT_DTYPE
from relativitypathtracer_amd.renderer import RenderError, Renderer, orient_objects, raymap, render_scene
from scene_fuzz import close_scene_text, extreme_scene_text, meshwalls_scene_text, random_scene_text, walls_scene_text

pytestmark = pytest.mark.gpu
MESH = {"cubes": False, "shadows": True, "bunny": True}
HUGE_OBJ = ("v -2147483648 -2147483648 8589934592\nv 2147483648 -2147483648 8589934592\nv 0 2147483648 8589934592\n"
            "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")          # |e1| |e2| > 2^60 (tests/test_gpu_exact_division.py)


def _exact(scene):
    """rpt_last_exact_rcp as for 41: the walk takes 1 / det through the exact reciprocal iff the scene lies in its domain (host code)"""
    d = scene.desc()
    return _ffi.hip().rpt_scene_exact_rcp(C.byref(d)) == 1


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("raymap")
    return dict(pano=rc.panorama_oracle(d), env=rc.environment_oracle(d), events=events_oracle.build_library(d),
                doppler=doppler_oracle.build_oracle(d))


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def _setup(r, scene, dirs, W, H, variant=0, doppler=(False, False), upload=True):
    r.set_variant(variant)
    r.set_msaa(1)
    r.set_adaptive_aa(1)
    r.set_field_of_view(0.0)
    r.set_orientation(0, 0, 0)
    r.set_environment(None)
    r.set_raymap(dirs)
    r.set_projection("raymap")
    if upload:
        r.upload_scene(scene)
    else:
        r.set_objects(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_debug_rgb(True)
    r.set_debug_doppler(False)
    r.set_doppler(*doppler)


def _frame(r, in_flight=False):
    if in_flight:
        r.render_async()
        r.sync()
    else:
        r.render()
    return r.read_framebuffer().copy(), r.read_debug_rgb().copy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _assert_frame(got, want, dirs, W, H, what):
    """All 16 bytes of every pixel and the float triple: the reference where the map has a ray, the sentinel where it has none"""
    epx, ergb = rc.expected_frame(want[0], want[1], dirs, W, H)
    bad = (got[0].view(np.uint8).reshape(-1, 16) != epx.view(np.uint8).reshape(-1, 16)).any(axis=1)
    ray = rc.has_ray(dirs)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ ({int((bad & ~ray).sum())} of them without a ray), first at {np.flatnonzero(bad)[:5]}"
    ok = _same_bits(got[1], ergb).reshape(-1, 3).all(axis=1)
    assert ok.all(), f"{what}: debug_rgb differs on {int((~ok).sum())} pixels, first at {np.flatnonzero(~ok)[:5]}"


def _expected_events(lib, scene, W, H, dirs, objects=None):
    ev = events_oracle.oracle_events(lib, scene, W, H, dirs=rc.oracle_dirs(dirs), objects=objects)
    miss = np.zeros((), dtype=EVENT_DTYPE)
    miss["object"] = -1
    ev.reshape(-1)[~rc.has_ray(dirs)] = miss
    return ev


# ---- 1. bit-exact against the CPU references, ray by ray -----------------------------------------------------------------------------
@pytest.mark.parametrize("camera", list(rc.CAMERAS))
@pytest.mark.parametrize("motion", ["rest", "fast"])
@pytest.mark.parametrize("name", list(rc.SCENES))
def test_frames_and_records_equal_the_references(renderer, libs, name, motion, camera):
    dirs, W, H = rc.camera_map(camera)
    scene = rc.load_scene(name, motion)
    ray = rc.has_ray(dirs)
    want_events = _expected_events(libs["events"], scene, W, H, dirs)
    # the conditions on the inputs, from the reference alone: the case has objects and background among its rays
    hit_share = float((want_events["object"].reshape(-1) >= 0)[ray].mean())
    print(f"{name} {motion} {camera}: {int(ray.sum())} of {W * H} pixels have a ray, {hit_share:.3f} of them hit an object")
    assert 0.05 <= hit_share <= 0.95, (name, motion, camera, hit_share)
    want = rc.panorama_frame(libs["pano"], scene, W, H, dirs)
    _setup(renderer, scene, dirs, W, H)
    for variant, in_flight, kernel in ((0, False, 1241 if MESH[name] else 1244), (0, True, 1241 if MESH[name] else 1244), (3, False, 1203)):
        renderer.set_variant(variant)
        got = _frame(renderer, in_flight)
        assert renderer.last_variant() == kernel
        assert renderer.last_exact_rcp() == (kernel == 1241 and _exact(scene))
        _assert_frame(got, want, dirs, W, H, f"{name} {motion} {camera} kernel {kernel}")
    renderer.set_variant(0)
    assert renderer.verify_frame() == 0
    got_events = renderer.render_events()
    assert renderer.last_events_variant() == (1291 if MESH[name] else 1294)
    assert renderer.last_events_exact_rcp() == (MESH[name] and _exact(scene))
    assert got_events.tobytes() == want_events.tobytes(), f"{int((got_events != want_events).sum())} records differ"


def _sky(W=64, H=32):
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(np.stack([40 + 3 * x, 30 + 6 * y, 220 - 2 * ((x + y) % W)], -1).astype(np.uint8))


@pytest.mark.parametrize("camera", list(rc.CAMERAS))
@pytest.mark.parametrize("name", list(rc.SCENES))
def test_doppler_twins_and_environment_forms_equal_their_references(renderer, libs, name, camera):
    dirs, W, H = rc.camera_map(camera)
    scene = rc.load_scene(name, "fast")
    want = doppler_oracle.render(libs["doppler"], scene, W, H, 3, dirs=rc.oracle_dirs(dirs))[:2]
    _setup(renderer, scene, dirs, W, H, doppler=(True, True))
    for variant, kernel in ((0, 1251 if MESH[name] else 1254), (3, 1213)):
        renderer.set_variant(variant)
        got = _frame(renderer)
        assert renderer.last_variant() == kernel and renderer.last_exact_rcp() == (kernel == 1251 and _exact(scene))
        _assert_frame(got, want, dirs, W, H, f"{name} {camera} kernel {kernel}")
    renderer.set_variant(0)
    assert renderer.verify_frame() == 0
    img, E = _sky(), scene.camera_lorentz()[1]
    renderer.set_environment(img)
    renderer.set_environment_frame(E)
    for flags in (0, 3):
        want = rc.environment_frame(libs["env"], scene, W, H, dirs, E, img, flags)
        renderer.set_doppler(bool(flags & 1), bool(flags & 2))
        for variant, kernel in ((0, 1261 if MESH[name] else 1264), (3, 1223)):
            renderer.set_variant(variant)
            got = _frame(renderer)
            assert renderer.last_variant() == kernel and renderer.last_exact_rcp() == (kernel == 1261 and _exact(scene))
            _assert_frame(got, want, dirs, W, H, f"{name} {camera} kernel {kernel} flags {flags}")
        renderer.set_variant(0)
        assert renderer.verify_frame() == 0
    renderer.set_environment(None)
    renderer.set_environment_frame(None)


def test_the_ieee_forms_outside_the_exact_reciprocals_domain(renderer, libs, tmp_path):
    """A triangle outside rcp_exact's domain in the mesh pool (named by no object): every walk kernel runs its IEEE-division form"""
    dirs, W, H = rc.camera_map("fisheye180")
    huge = tmp_path / "huge.obj"
    huge.write_text(HUGE_OBJ)
    scene = Scene.from_file("bunny")
    scene.ReadOBJ(str(huge))
    c = rc.SCENES["bunny"]["fast"]
    scene.set_camera(c["v"], c["t"], c["p"])
    scene.update_objects()
    assert not _exact(scene) and _exact(rc.load_scene("bunny", "fast"))
    _setup(renderer, scene, dirs, W, H)
    got = _frame(renderer)
    assert renderer.last_variant() == 1241 and not renderer.last_exact_rcp()
    _assert_frame(got, rc.panorama_frame(libs["pano"], scene, W, H, dirs), dirs, W, H, "1241 (IEEE)")
    ev = renderer.render_events()
    assert renderer.last_events_variant() == 1291 and not renderer.last_events_exact_rcp()
    assert ev.tobytes() == _expected_events(libs["events"], scene, W, H, dirs).tobytes()
    renderer.set_doppler(True, True)
    got = _frame(renderer)
    assert renderer.last_variant() == 1251 and not renderer.last_exact_rcp()
    _assert_frame(got, doppler_oracle.render(libs["doppler"], scene, W, H, 3, dirs=rc.oracle_dirs(dirs))[:2], dirs, W, H, "1251 (IEEE)")
    img, E = _sky(), scene.camera_lorentz()[1]
    renderer.set_environment(img)
    renderer.set_environment_frame(E)
    got = _frame(renderer)
    assert renderer.last_variant() == 1261 and not renderer.last_exact_rcp()
    _assert_frame(got, rc.environment_frame(libs["env"], scene, W, H, dirs, E, img, 3), dirs, W, H, "1261 (IEEE)")
    renderer.set_environment(None)
    renderer.set_environment_frame(None)


# ---- 2. device against device: another camera's own directions through the map ------------------------------------------------------
@pytest.mark.parametrize("name", ["shadows", "bunny", "cubes"])
def test_the_pinholes_directions_render_kernel_3s_frame(renderer, name):
    W, H = 100, 52
    scene = rc.load_scene(name, "rest")
    dirs = events_oracle.pinhole_dirs(W, H).reshape(H, W, 3)            # (fx2, fy2, 0.5) in the reference's float operations
    _setup(renderer, scene, dirs, W, H, variant=3)
    got = _frame(renderer)
    assert renderer.last_variant() == 1203
    renderer.set_variant(0)
    got0 = _frame(renderer)
    renderer.set_projection("pinhole")
    renderer.set_variant(3)
    want = _frame(renderer)
    assert renderer.last_variant() == 3
    for g in (got, got0):
        assert g[0].tobytes() == want[0].tobytes() and _same_bits(g[1], want[1]).all()


@pytest.mark.parametrize("name", ["shadows", "bunny", "cubes"])
def test_the_panoramas_directions_render_the_panoramas_frame(renderer, name):
    W, H = 104, 52
    proj = dict(h_fov=5.0, v_fov=2.5, yaw=0.4)
    scene = rc.load_scene(name, "fast")
    dirs = events_oracle.pano_dirs(W, H, **proj).reshape(H, W, 3)
    img, E = _sky(), scene.camera_lorentz()[1]
    for doppler, sky, pano_kernels, map_kernels in ((False, False, (341, 344), (1241, 1244)), (True, False, (541, 544), (1251, 1254)),
                                                    (False, True, (741, 744), (1261, 1264)), (True, True, (741, 744), (1261, 1264))):
        _setup(renderer, scene, dirs, W, H, doppler=(doppler, doppler))
        if sky:
            renderer.set_environment(img)
            renderer.set_environment_frame(E)
        got = _frame(renderer)
        assert renderer.last_variant() == map_kernels[0 if MESH[name] else 1]
        renderer.set_projection("equirect", **proj)
        want = _frame(renderer)
        assert renderer.last_variant() == pano_kernels[0 if MESH[name] else 1]
        assert got[0].tobytes() == want[0].tobytes() and _same_bits(got[1], want[1]).all(), (name, doppler, sky)
    renderer.set_environment(None)
    renderer.set_environment_frame(None)


# ---- 3. the culls ------------------------------------------------------------------------------------------------------------------
GENERATORS = {"random": lambda rng: random_scene_text(rng)[0], "extreme": extreme_scene_text, "close": close_scene_text,
              "walls": walls_scene_text, "meshwalls": meshwalls_scene_text}


def _scene(text, v=(0.0, 0.0, 0.0), t=0.0, interval=None):
    s = Scene()
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


@pytest.mark.parametrize("gen", list(GENERATORS))
def test_verify_frame_on_thirty_generated_scenes(renderer, gen):
    """Six scenes of each of the five generators through one fisheye: the shadow-ray culls change no pixel"""
    rng = np.random.default_rng(1400 + len(gen))
    W, H = 100, 52
    dirs = raymap("fisheye", W, H, fov=220.0 * rc.DEG, fit=0)
    seen = set()
    for i in range(6):
        scene = _scene(GENERATORS[gen](rng))
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.95])
        scene.set_camera(tuple(float(c) for c in v), float(rng.uniform(-3, 20)))
        scene.update_objects()
        _setup(renderer, scene, dirs, W, H, doppler=(bool(i & 1), bool(i & 1)))
        assert renderer.verify_frame() == 0, f"{gen} scene {i}"
        seen.add(renderer.last_variant())
    assert seen and seen <= {1241, 1244, 1251, 1254}


# ---- 4. aberration -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta_deg", [40.0, 90.0, 140.0])
def test_aberration_puts_a_sphere_where_special_relativity_does(renderer, theta_deg):
    """A sphere at rest at polar angle theta from +z, the camera passing the origin at 0.9 c along +z: in an equidistant fisheye the
    centroid of its pixels lies at rho = theta' / (fov / 2), cos theta' = (cos theta + beta) / (1 + beta cos theta)."""
    beta, W, H, fov, dist, radius = 0.9, 128, 128, 200.0 * rc.DEG, 10.0, 2.0
    theta, phi = theta_deg * rc.DEG, 0.7
    pos = (dist * math.sin(theta) * math.cos(phi), dist * math.sin(theta) * math.sin(phi), dist * math.cos(theta))
    scene = _scene(f"Os\n p{pos[0]},{pos[1]},{pos[2]},0,0,1,0,{radius},{radius},{radius}\n c1,0.8,0.6\n l1\n v0,0,0\nA0.2\nR\n", v=(0.0, 0.0, beta), t=0.0, interval=-1)
    dirs = raymap("fisheye", W, H, fov=fov, fit=0)
    _setup(renderer, scene, dirs, W, H)
    ev = renderer.render_events()
    ys, xs = np.nonzero(ev["object"] >= 0)
    assert len(xs) >= 4

    def aberrated(t):
        return math.acos((math.cos(t) + beta) / (1.0 + beta * math.cos(t)))

    # the limb: rays that leave the origin's light cone at alpha = asin(radius / dist) from the centre's direction arrive between
    # theta'(theta - alpha) and theta'(theta + alpha) in polar angle (theta' is monotone) and, across, within alpha times the
    # transverse scale sin theta' / sin theta: the apparent angular radius is at most the larger of the two
    alpha = math.asin(radius / dist)
    tp = aberrated(theta)
    apparent = max(abs(aberrated(theta - alpha) - tp), abs(aberrated(theta + alpha) - tp), alpha * math.sin(tp) / math.sin(theta))
    px_per_rad = (min(W, H) / 2.0) / (fov / 2.0)                  # rho = theta' / (fov / 2), one unit of rho = min(W, H) / 2 pixels
    cx, cy = (xs + 0.5).mean() - W / 2.0, (ys + 0.5).mean() - H / 2.0
    want = tp * px_per_rad
    assert abs(math.hypot(cx, cy) - want) <= 1.0 + apparent * px_per_rad, (theta_deg, math.hypot(cx, cy), want)
    assert abs(math.atan2(cy, cx) - phi) * want <= 1.0 + apparent * px_per_rad           # ... and at the sphere's own azimuth


# ---- 5. plumbing ---------------------------------------------------------------------------------------------------------------------
def test_a_map_without_any_ray_renders_a_black_frame(renderer):
    W, H = 100, 52
    scene = rc.load_scene("bunny", "rest")
    dirs = np.zeros((H, W, 3), dtype=np.float32)
    for doppler, sky in ((False, False), (True, False), (True, True)):
        _setup(renderer, scene, dirs, W, H, doppler=(doppler, doppler))
        if sky:
            renderer.set_environment(_sky())
        px, rgb = _frame(renderer)
        assert px.tobytes() == rc.sentinel_pixels(W, H).tobytes() and not rgb.any()
        ev = renderer.render_events()
        assert (ev["object"] == -1).all() and not ev["dist"].any() and not ev["event"].any() and not ev["uv"].any()
    renderer.set_environment(None)


@pytest.mark.parametrize("name,doppler", [("bunny", False), ("cubes", True)])
def test_row_tiles_equal_the_whole_frame(renderer, name, doppler):
    dirs, W, H = rc.camera_map("fisheye180")
    scene = rc.load_scene(name, "fast")
    _setup(renderer, scene, dirs, W, H, doppler=(doppler, doppler))
    renderer.set_debug_rgb(False)
    renderer.render()
    whole32 = renderer.read_framebuffer()["rgba"].reshape(H, W, 4).copy().view(np.uint32).reshape(H, W)
    assert (whole32 == 0x01000000).any() and (whole32 != 0x01000000).any()
    tiles = (H + 7) // 8
    for first, step, run in ((0, 3, 1), (1, 3, 1), (2, 3, 1), (0, 5, 2), (1, 4, 4)):
        if run == 1:
            renderer.set_rows(first, step, True)
        else:
            renderer.set_tile_pattern(first, step, run, True)
        renderer.render()
        plane = renderer.read_colour_plane()
        local = [t for t in range(tiles) if (t - first) % step < run and t >= first]
        for k, t in enumerate(local):
            rows = slice(t * 8, min(H, t * 8 + 8))
            assert np.array_equal(plane[k * 8:k * 8 + (rows.stop - rows.start)], whole32[rows]), (first, step, t)
    renderer.set_rows(0, 1, False)


def test_two_contexts_share_a_scene_and_keep_their_own_maps(libs):
    W, H = 100, 52
    scene = rc.load_scene("bunny", "rest")
    maps = [raymap("fisheye", W, H, fov=math.pi, fit=0), raymap("stereographic", W, H, fov=4.0, fit=1)]
    slots = [Renderer(0) for _ in range(2)]
    try:
        slots[0].upload_scene(scene)
        slots[1].share_scene(slots[0])
        for s, m in zip(slots, maps):
            s.set_scene_params(scene, W, H)
            s.set_output(None)
            s.set_debug_rgb(True)
            s.set_raymap(m)
            s.set_projection("raymap")
        for s in slots:
            s.render_async()
        for s, m in zip(slots, maps):
            s.sync()
            assert s.last_variant() == 1241
            _assert_frame((s.read_framebuffer(), s.read_debug_rgb()), rc.panorama_frame(libs["pano"], scene, W, H, m), m, W, H, "slot")
        # the map is not shared: a third context on the same scene is a pinhole, and asking it for the ray-map camera is refused
        other = Renderer(0)
        try:
            other.share_scene(slots[0])
            other.set_scene_params(scene, W, H)
            other.set_output(None)
            other.render()
            assert other.last_variant() == 43
            with pytest.raises(RenderError, match="rpt_set_raymap"):
                other.set_projection("raymap")
        finally:
            other.close()
    finally:
        for s in slots:
            s.close()


@pytest.mark.parametrize("name", ["bunny", "cubes"])
def test_an_orientation_turns_the_fisheye(renderer, libs, name):
    dirs, W, H = rc.camera_map("fisheye180")
    scene = rc.load_scene(name, "fast")
    ypr = (2.4, -0.5, 0.9)
    _setup(renderer, scene, dirs, W, H)
    plain = _frame(renderer)
    renderer.set_orientation(*ypr)
    got = _frame(renderer)
    objects = orient_objects(scene, *ypr)
    _assert_frame(got, rc.panorama_frame(libs["pano"], scene, W, H, dirs, objects), dirs, W, H, name)
    assert got[0].tobytes() != plain[0].tobytes()
    assert renderer.render_events().tobytes() == _expected_events(libs["events"], scene, W, H, dirs, objects).tobytes()
    renderer.set_orientation(0, 0, 0)


def test_replacing_the_map_takes_effect_at_the_next_launch(renderer, libs):
    W, H = 100, 52
    scene = rc.load_scene("shadows", "rest")
    first, second = raymap("fisheye", W, H, fov=math.pi, fit=0), raymap("equisolid", W, H, fov=5.0, fit=1)
    _setup(renderer, scene, first, W, H)
    renderer.render_async()
    renderer.set_raymap(second)              # behind the frame in flight, which keeps the map it was launched with
    renderer.sync()
    _assert_frame((renderer.read_framebuffer(), renderer.read_debug_rgb()), rc.panorama_frame(libs["pano"], scene, W, H, first), first, W, H, "first")
    _assert_frame(_frame(renderer), rc.panorama_frame(libs["pano"], scene, W, H, second), second, W, H, "second")
    renderer.set_raymap(first.reshape(-1, 3), W, H)              # the (H W, 3) form
    _assert_frame(_frame(renderer), rc.panorama_frame(libs["pano"], scene, W, H, first), first, W, H, "first again")


def test_render_scene_takes_a_ray_map(libs):
    W, H = 120, 20
    scene = rc.load_scene("cubes", "rest")
    want = rc.panorama_frame(libs["pano"], scene, W, H, raymap("cube_strip", W, H))
    px, rgb = render_scene(scene, W, H, debug_rgb=True, projection="cube_strip")
    _assert_frame((px, rgb), want, raymap("cube_strip", W, H), W, H, "cube_strip")
    m = raymap("stereographic", 100, 52, fov=4.0, fit=1)
    px, rgb = render_scene(scene, 100, 52, debug_rgb=True, projection="stereographic", fov=4.0, fit=1)
    px2, rgb2 = render_scene(scene, 100, 52, debug_rgb=True, projection=m)
    assert px.tobytes() == px2.tobytes() and _same_bits(rgb, rgb2).all()
    _assert_frame((px, rgb), rc.panorama_frame(libs["pano"], scene, 100, 52, m), m, 100, 52, "stereographic")


def test_back_to_the_pinhole_restores_the_kernel_choice(renderer):
    W, H = 100, 52
    scene = rc.load_scene("bunny", "rest")
    dirs = raymap("fisheye", W, H, fov=math.pi, fit=0)
    _setup(renderer, scene, dirs, W, H)
    renderer.render()
    assert renderer.last_variant() == 1241
    renderer.set_projection("pinhole")
    px, rgb = _frame(renderer)
    assert renderer.last_variant() == 43
    opx, orgb, _ = oracle_ffi.render(scene, W, H)
    assert px.tobytes() == opx.tobytes() and _same_bits(rgb, orgb).all()
    renderer.render_async()
    renderer.sync()
    assert renderer.last_variant() == 43                  # (a small frame in flight)
    renderer.set_projection("equirect")
    renderer.render()
    assert renderer.last_variant() == 341
    renderer.set_projection("raymap")
    renderer.render()
    assert renderer.last_variant() == 1241


def test_refusals_leave_the_context_rendering(renderer, libs):
    W, H = 100, 52
    bunny = rc.load_scene("bunny", "rest")
    dirs = raymap("fisheye", W, H, fov=math.pi, fit=0)
    want = rc.panorama_frame(libs["pano"], bunny, W, H, dirs)
    lib, h = renderer._lib, renderer._h
    launches = (renderer.render, renderer.render_async, renderer.verify_frame, renderer.render_events, lambda: renderer.render_events(async_=True))

    def refused(match, calls=launches):
        for call in calls:
            with pytest.raises(RenderError, match=match):
                call()

    def renders():
        _assert_frame(_frame(renderer), want, dirs, W, H, "after a refusal")
        assert renderer.last_variant() == 1241

    _setup(renderer, bunny, dirs, W, H)
    renders()
    # at the launch: no map, a map of another size
    renderer.set_raymap(None)
    refused(r"\(1\).*rpt_set_raymap: .*no ray map")
    renderer.set_raymap(raymap("fisheye", W + 4, H, fov=math.pi))
    refused(r"\(1\).*rpt_set_raymap: the map is 104 x 52, the frame 100 x 52")
    renderer.set_raymap(dirs)
    renders()
    colour = launches[:3]
    # a lens
    renderer.set_field_of_view(1.0)
    refused(r"\(1\).*rpt_set_field_of_view: the ray map", colour)
    refused(r"\(1\).*rpt_render_events: the ray map", launches[3:])
    renderer.set_field_of_view(0.0)
    # MSAA
    renderer.set_msaa(2)
    refused(r"\(1\).*MSAA", launches)
    renderer.set_msaa(1)
    # adaptive anti-aliasing acts on rpt_render / rpt_render_async
    renderer.set_adaptive_aa(2, 8)
    refused(r"\(1\).*rpt_set_adaptive_aa: the ray-map camera", launches[:2])
    renderer.set_adaptive_aa(1)
    # variants without a ray-map kernel; 41, 43 and 44 have one
    for variant in (1, 48, 49, 50, 51):
        renderer.set_variant(variant)
        refused(r"\(1\).*variant " + str(variant), launches)
    for variant in (41, 43, 44):
        renderer.set_variant(variant)
        renders()
    renderer.set_variant(0)
    # the Doppler debug kernel (rpt_verify_frame sets the hook aside, as everywhere)
    renderer.set_doppler(True, True)
    renderer.set_debug_doppler(True)
    refused(r"\(1\).*rpt_set_raymap: the Doppler debug kernel", launches[:2])
    renderer.set_debug_doppler(False)
    renderer.set_doppler(False, False)
    renders()
    # the calls themselves
    f3 = lambda *v: (C.c_float * 3)(*v)
    assert lib.rpt_set_projection(h, 2, f3(1, 1, 0)) == 1                  # the ray map takes no parameters
    bad = dirs.copy()
    for value in (math.nan, math.inf, -math.inf):
        bad[H - 1, W - 1, 2] = value
        assert lib.rpt_set_raymap(h, bad.ctypes.data, W, H) == 1 and b"rpt_set_raymap" in lib.rpt_last_error(h)
    assert lib.rpt_set_raymap(h, dirs.ctypes.data, 0, H) == 1 and lib.rpt_set_raymap(h, dirs.ctypes.data, W, -1) == 1
    assert lib.rpt_set_raymap(h, dirs.ctypes.data, 1 << 15, 1 << 15) == 1     # 3 W H >= 2^31 (refused before anything is read)
    assert lib.rpt_set_raymap(None, dirs.ctypes.data, W, H) == 1
    with pytest.raises(ValueError):
        renderer.set_raymap(np.zeros((H, W, 2), dtype=np.float32))
    renders()                                                             # (a refused map leaves the one in place)
    # an octree whose children are not consecutive (test_gpu_panorama's construction): no derived layout, no ray-map kernel with a mesh
    shadows = rc.load_scene("shadows", "rest")
    oc = shadows.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
    root = shadows.mesh_roots()[0]
    new = np.vstack([oc, oc[oc[root, 10]][None]])
    new[root, 10] = len(oc)
    d2 = _ffi.SceneDesc.from_buffer_copy(shadows.desc())
    raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
    d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
    renderer.upload_desc(d2)
    renderer.set_scene_params(shadows, W, H)
    refused(r"\(1\).*octree", launches)
    renderer.set_projection("pinhole")
    renderer.render()
    assert renderer.last_variant() == 1
    _setup(renderer, bunny, dirs, W, H)
    renders()
    # a context without a map has no ray-map camera to select
    renderer.set_projection("pinhole")
    renderer.set_raymap(None)
    with pytest.raises(RenderError, match="rpt_set_raymap first"):
        renderer.set_projection("raymap")
    renderer.render()
    assert renderer.last_variant() == 43
