"""rpt_set_object_windows on the MI355X (DESIGN.md "Time windows"): with every window at its default the windowed kernels give the
un-windowed frame byte for byte; with windows that act (window_oracle.choose_windows; tests/test_window_oracle.py shows on the CPU that
they do) every frame and every event record equals tests/native/window_oracle.c in every byte, through every camera, colour and kernel
form; culled equals un-culled; shards, shared scenes, clearing, the refusals; and a sphere that turns round is seen to do so when
special relativity says."""
import ctypes as C
import math

import numpy as np
import pytest

import events_oracle as eo
import raymap_cases as rc
import window_oracle as wo
from relativitypathtracer_amd import Scene, _ffi, worldline
from relativitypathtracer_amd.events import EVENT_DTYPE, overlay
from relativitypathtracer_amd.renderer import RenderError, Renderer, orient_objects, raymap

pytestmark = pytest.mark.gpu

W, H = 128, 72
YPR = (0.4, -0.25, 0.15)
PANO = dict(h_fov=2.0, v_fov=1.2, yaw=0.3)
LENS60, LENS100 = 60.0 * math.pi / 180.0, 100.0 * math.pi / 180.0
HUGE_OBJ = ("v -2147483648 -2147483648 8589934592\nv 2147483648 -2147483648 8589934592\nv 0 2147483648 8589934592\n"
            "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")          # |e1| |e2| > 2^60 (tests/test_gpu_exact_division.py)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return wo.build_library(tmp_path_factory.mktemp("windows"))


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.set_object_windows(None)
    r.close()


@pytest.fixture(scope="module")
def cases(lib):
    """name -> (scene, windows): the windows chosen once per scene on the CPU, from the pinhole's 128 x 72 event frame"""
    out = {}
    for name in wo.SCENES:          # (cubes and rulers with a lamp and a shadow-taking surface added: window_oracle.LIT)
        scene = wo.load(name)
        assert scene.params["interval"] == (0 if name == "rulers" else -1)          # (rulers.txt's `I`; rulers_delay: the same file with light delay on)
        out[name] = (scene, wo.choose_windows(lib, scene, W, H, flip=wo.FLIP.get(name, False)))
    return out


def _sky(w=64, h=32):
    y, x = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([40 + 3 * x, 30 + 6 * y, 220 - 2 * ((x + y) % w)], -1).astype(np.uint8))


def _camera(kind, w, h):
    """(what the renderer is set to, the CPU reference's per-pixel directions, the map or None)"""
    if kind == "pinhole":
        return dict(), eo.pinhole_dirs(w, h), None
    if kind in ("lens60", "lens100"):
        v = LENS60 if kind == "lens60" else LENS100
        return dict(v_fov=v), eo.pinhole_dirs(w, h, s=eo.lens_scale(v)), None
    if kind == "equirect":
        return dict(pano=PANO), eo.pano_dirs(w, h, **PANO), None
    assert kind == "fisheye"
    m = raymap("fisheye", w, h, fov=math.pi, fit=0)
    return dict(map=m), rc.oracle_dirs(m), m


def _setup(r, scene, w, h, cam=None, variant=0, doppler=0, sky=None, ypr=(0.0, 0.0, 0.0), windows=None, upload=True):
    cam = cam or {}
    r.set_variant(variant)
    r.set_msaa(1)
    r.set_adaptive_aa(1)
    r.set_debug_doppler(False)
    r.set_doppler(bool(doppler & 1), bool(doppler & 2))
    r.set_orientation(*ypr)
    r.set_field_of_view(cam.get("v_fov", 0.0))
    if "pano" in cam:
        r.set_projection("equirect", **cam["pano"])
    elif "map" in cam:
        r.set_raymap(cam["map"])
        r.set_projection("raymap")
    else:
        r.set_projection("pinhole")
    if sky is None:
        r.set_environment(None)
        r.set_environment_frame(None)
    else:
        r.set_environment(sky)
        r.set_environment_frame(scene.camera_lorentz()[1])
    r.set_object_windows(windows)
    if upload:
        r.upload_scene(scene)
    else:
        r.set_objects(scene)
    r.set_scene_params(scene, w, h)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)
    r.set_debug_rgb(True)


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


def _assert_frame(got, want, what, m=None, w=W, h=H):
    """All 16 bytes of every pixel and the float triple (through a ray map: the sentinel where the map has no ray)"""
    wpx, wrgb = (want[0], want[1]) if m is None else rc.expected_frame(want[0], want[1], m, w, h)
    bad = (np.ascontiguousarray(got[0]).view(np.uint8).reshape(-1, 16) != np.ascontiguousarray(wpx).view(np.uint8).reshape(-1, 16)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at {np.flatnonzero(bad)[:5]}"
    ok = _same_bits(got[1], wrgb).reshape(-1, 3).all(axis=1)
    assert ok.all(), f"{what}: debug_rgb differs on {int((~ok).sum())} pixels, first at {np.flatnonzero(~ok)[:5]}"


def _want_events(ev, m):
    if m is not None:
        miss = np.zeros((), dtype=EVENT_DTYPE)
        miss["object"] = -1
        ev = ev.copy()
        ev.reshape(-1)[~rc.has_ray(m)] = miss
    return ev


BAND_FIRST = {43: 41, 49: 48, 243: 241, 249: 248, 643: 641, 843: 841, 853: 851, 863: 861}      # a band-first row -> the walk row of its camera and colour


def _windowed(base):
    """2000 + the variant of the row of the same camera and colour whose form ran: a band-first choice gets the walk"""
    return 2000 + BAND_FIRST.get(base, base)


def _check(r, lib, scene, windows, kind, what, w=W, h=H, doppler=0, sky=None, ypr=None, launches=((0, False), (0, True), (3, False)),
           events=True, verify=True):
    cam, dirs, m = _camera(kind, w, h)
    objects = None if ypr is None else orient_objects(scene, *ypr)
    E = None if sky is None else scene.camera_lorentz()[1]
    want = wo.render(lib, scene, w, h, windows, dirs=dirs, flags=doppler, objects=objects, sky=sky, sky_frame=E)
    _setup(r, scene, w, h, cam, doppler=doppler, sky=sky, ypr=ypr or (0.0, 0.0, 0.0), windows=None)
    base = {}
    for variant, in_flight in launches:          # the kernels the same launches get without windows
        r.set_variant(variant)
        _frame(r, in_flight)
        base[(variant, in_flight)] = r.last_variant()
    r.set_variant(0)
    r.render_events()
    base_events = r.last_events_variant()
    r.set_object_windows(windows)
    for variant, in_flight in launches:
        r.set_variant(variant)
        got = _frame(r, in_flight)
        assert r.last_variant() == _windowed(base[(variant, in_flight)]), (what, variant, in_flight, r.last_variant(), base)
        _assert_frame(got, want, f"{what} variant {variant} in flight {in_flight} kernel {r.last_variant()}", m, w, h)
    r.set_variant(0)
    if verify:
        assert r.verify_frame() == 0, what
    if events:
        got = r.render_events()
        assert r.last_events_variant() == 2000 + base_events
        ev = _want_events(want[2], m)
        assert got.tobytes() == ev.tobytes(), f"{what}: {int((got != ev).sum())} event records differ"
        hit = got["object"] >= 0
        assert wo.accepts(windows, got["object"][hit], got["event"][..., 0][hit]).all()
    r.set_object_windows(None)


# ---- 1. default windows: the windowed kernels run and give the un-windowed frame ---------------------------------------------------------
@pytest.mark.parametrize("name", ["arch", "shadows", "cubes"])
def test_default_windows_give_the_unwindowed_frame(renderer, cases, name):
    scene = cases[name][0]
    n = len(scene.objects())
    for kind, w, h in (("pinhole", W, H), ("pinhole", 70, 45), ("equirect", W, H), ("fisheye", 64, 48)):
        cam, _, _ = _camera(kind, w, h)
        for doppler, sky in ((0, None), (3, None), (3, _sky())):
            _setup(renderer, scene, w, h, cam, doppler=doppler, sky=sky)
            plain, base = _frame(renderer), renderer.last_variant()
            plain_events, base_events = renderer.render_events().copy(), renderer.last_events_variant()
            assert base < 2000
            renderer.set_object_windows(wo.default_windows(n))
            got = _frame(renderer)
            assert renderer.last_variant() == _windowed(base), (name, kind, doppler, renderer.last_variant(), base)
            _assert_frame(got, plain, f"{name} {kind} {w}x{h} doppler {doppler} sky {sky is not None}")
            ev = renderer.render_events()
            assert renderer.last_events_variant() == 2000 + base_events and ev.tobytes() == plain_events.tobytes()
            renderer.set_object_windows(None)


# ---- 2. parity with the window oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wo.SCENES)
def test_every_camera_equals_the_window_oracle(renderer, lib, cases, name):
    scene, windows = cases[name]
    assert np.isfinite(windows).sum() >= 2
    if name == "many":
        assert np.isfinite(windows[64:]).sum() == 2, "objects 64 and 65 (beyond the 64-bit object mask) have windows"
    _check(renderer, lib, scene, windows, "pinhole", f"{name} pinhole")
    _check(renderer, lib, scene, windows, "pinhole", f"{name} pinhole 70x45", w=70, h=45)
    _check(renderer, lib, scene, windows, "lens60", f"{name} lens 60")
    _check(renderer, lib, scene, windows, "lens100", f"{name} lens 100 (un-culled)", launches=((0, False),))
    _check(renderer, lib, scene, windows, "equirect", f"{name} equirect", launches=((0, False), (3, False)))
    _check(renderer, lib, scene, windows, "fisheye", f"{name} fisheye", w=64, h=48, launches=((0, False), (3, False)))


@pytest.mark.parametrize("name", ["arch", "shadows", "cubes", "rulers_delay", "many"])
def test_doppler_the_sky_and_a_turned_camera_equal_the_window_oracle(renderer, lib, cases, name):
    scene, windows = cases[name]
    _check(renderer, lib, scene, windows, "pinhole", f"{name} Doppler", doppler=3, events=False)
    _check(renderer, lib, scene, windows, "pinhole", f"{name} shift only", doppler=1, events=False, launches=((0, True),))
    _check(renderer, lib, scene, windows, "pinhole", f"{name} sky", sky=_sky(), events=False)
    _check(renderer, lib, scene, windows, "equirect", f"{name} sky Doppler equirect", sky=_sky(), doppler=3, events=False, launches=((0, False), (3, False)))
    _check(renderer, lib, scene, windows, "fisheye", f"{name} Doppler fisheye", w=64, h=48, doppler=3, events=False, launches=((0, False),))
    _check(renderer, lib, scene, windows, "fisheye", f"{name} sky fisheye", w=64, h=48, sky=_sky(), events=False, launches=((0, False),))
    _check(renderer, lib, scene, windows, "pinhole", f"{name} turned", ypr=YPR)
    _check(renderer, lib, scene, windows, "lens60", f"{name} turned lens Doppler", ypr=YPR, doppler=3, events=False, launches=((0, False),))


def test_the_ieee_forms_outside_the_exact_reciprocals_domain(renderer, lib, cases, tmp_path):
    """A triangle outside rcp_exact's domain in the mesh pool (named by no object): every windowed walk kernel runs its IEEE form"""
    huge = tmp_path / "huge.obj"
    huge.write_text(HUGE_OBJ)
    scene = Scene.from_file("shadows")
    scene.ReadOBJ(str(huge))
    scene.set_camera((0.0, 0.0, 0.0), 16.0)
    scene.update_objects()
    d = scene.desc()
    assert _ffi.hip().rpt_scene_exact_rcp(C.byref(d)) == 0
    windows = cases["shadows"][1]
    for kind, w, h in (("pinhole", W, H), ("equirect", W, H), ("fisheye", 64, 48)):
        for doppler, sky in ((0, None), (3, None), (0, _sky())):
            _check(renderer, lib, scene, windows, kind, f"IEEE {kind} doppler {doppler} sky {sky is not None}", w=w, h=h, doppler=doppler, sky=sky,
                   launches=((0, True),), events=sky is None and doppler == 0)
            assert not renderer.last_exact_rcp()
    # the forced-IEEE arms of the pinhole: 48 and 49 both get the windowed walk's IEEE kernel
    cam, dirs, _ = _camera("pinhole", W, H)
    want = wo.render(lib, scene, W, H, windows, dirs=dirs)
    _setup(renderer, scene, W, H, cam, windows=windows)
    for variant in (48, 49):
        renderer.set_variant(variant)
        got = _frame(renderer)
        assert renderer.last_variant() == 2048
        _assert_frame(got, want, f"variant {variant}")
    renderer.set_variant(0)
    renderer.set_object_windows(None)


# ---- 3. the overlay pass reads records only: it works on a windowed event frame ---------------------------------------------------------
def test_the_overlay_on_a_windowed_frame_equals_its_numpy_reference(renderer, cases):
    scene, windows = cases["arch"]
    _setup(renderer, scene, W, H, windows=windows)
    renderer.set_debug_rgb(False)
    renderer.render()
    before = renderer.read_framebuffer().copy()
    records = renderer.render_events().copy()
    kw = dict(outlines=True, clock_step=0.5)
    renderer.set_overlay(**kw)
    renderer.render_overlay()
    after = renderer.read_framebuffer().copy()
    rgba, count = overlay(before["rgba"], records, scene.params["interval"], **kw)
    assert count > 0 and renderer.last_overlay_pixels() == count
    assert np.array_equal(after["rgba"], rgba.reshape(-1, 4))
    renderer.set_overlay()
    renderer.set_object_windows(None)


# ---- 4. shards, frames in flight, shared scenes, clearing -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shadows", "many"])
def test_row_tiles_and_tile_patterns_equal_the_whole_frame(renderer, cases, name):
    scene, windows = cases[name]
    _setup(renderer, scene, W, H, windows=windows)
    renderer.set_debug_rgb(False)
    renderer.render()
    whole32 = renderer.read_framebuffer()["rgba"].reshape(H, W, 4).copy().view(np.uint32).reshape(H, W)
    tiles = (H + 7) // 8
    for first, step, run in ((0, 2, 1), (1, 2, 1), (0, 5, 2), (2, 5, 2), (4, 5, 1), (1, 4, 4)):       # a 2-way shard, a weighted 2 : 2 : 1 pattern, a run of 4
        if run == 1:
            renderer.set_rows(first, step, True)
        else:
            renderer.set_tile_pattern(first, step, run, True)
        renderer.render()
        assert renderer.last_variant() >= 2000
        plane = renderer.read_colour_plane()
        local = [t for t in range(tiles) if (t - first) % step < run and t >= first]
        for k, t in enumerate(local):
            rows = slice(t * 8, min(H, t * 8 + 8))
            assert np.array_equal(plane[k * 8:k * 8 + (rows.stop - rows.start)], whole32[rows]), (first, step, t)
    renderer.set_rows(0, 1, False)
    renderer.set_object_windows(None)


def test_two_contexts_share_a_scene_and_keep_their_own_windows(lib, cases):
    scene, windows = cases["shadows"]
    other = windows.copy()
    other[:, 0], other[:, 1] = -np.inf, windows[:, 0]          # what begins in one context ends in the other
    other[~np.isfinite(windows[:, 0]), 1] = np.inf
    a, b, c = Renderer(0), Renderer(0), Renderer(0)
    try:
        _setup(a, scene, W, H, windows=windows)
        b.share_scene(a)
        c.share_scene(a)
        _setup(b, scene, W, H, windows=other, upload=False)
        _setup(c, scene, W, H, windows=None, upload=False)          # sharing takes no windows over
        for _ in range(2):
            for r in (a, b, c):
                r.render_async()
        frames = []
        for r in (a, b, c):
            r.sync()
            frames.append((r.read_framebuffer().copy(), r.read_debug_rgb().copy()))
        assert a.last_variant() == b.last_variant() == 2041 and c.last_variant() == 43          # (a small frame in flight: the latency kernel)
        dirs = eo.pinhole_dirs(W, H)
        for got, w, what in zip(frames, (windows, other, None), "abc"):
            _assert_frame(got, wo.render(lib, scene, W, H, w, dirs=dirs), f"context {what}")
        assert frames[0][0].tobytes() != frames[1][0].tobytes() != frames[2][0].tobytes()
    finally:
        for r in (a, b, c):
            r.close()


def test_clearing_the_windows_brings_the_parents_kernels_back(renderer, cases):
    scene, windows = cases["shadows"]
    _setup(renderer, scene, W, H)
    plain = _frame(renderer)
    assert renderer.last_variant() == 43
    renderer.set_object_windows(windows)
    assert _frame(renderer)[0].tobytes() != plain[0].tobytes() and renderer.last_variant() == 2041
    renderer.render_events()
    assert renderer.last_events_variant() == 2941
    renderer.set_object_windows(None)
    _assert_frame(_frame(renderer), plain, "cleared")
    assert renderer.last_variant() == 43
    _frame(renderer, in_flight=True)
    assert renderer.last_variant() == 43          # (128 x 72 in flight is a small frame: the latency kernel)
    renderer.render_events()
    assert renderer.last_events_variant() == 941


# ---- 5. the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_context_rendering(renderer, cases):
    scene, windows = cases["shadows"]
    _setup(renderer, scene, W, H, windows=windows)
    good = _frame(renderer)
    assert renderer.last_variant() == 2041

    RPT_ERR_ARG = 1          # include/rpt.h

    def refused(launch=renderer.render):
        with pytest.raises(RenderError, match="rpt_set_object_windows") as e:
            launch()
        assert e.value.code == RPT_ERR_ARG
        assert renderer.last_variant() == 2041
        assert renderer.read_framebuffer().tobytes() == good[0].tobytes()

    with pytest.raises(RenderError, match="NaN") as e:
        renderer.set_object_windows(np.array([[0.0, np.nan]] * len(windows), dtype=np.float32))
    assert e.value.code == RPT_ERR_ARG
    _assert_frame(_frame(renderer), good, "after a NaN bound: the windows are the old ones")
    renderer.set_msaa(2)
    refused()
    refused(renderer.render_async)
    renderer.set_msaa(1)
    renderer.set_adaptive_aa(2, 8)
    refused()
    renderer.set_adaptive_aa(1)
    for variant in (1, 50, 51):
        renderer.set_variant(variant)
        refused()
    renderer.set_variant(0)
    renderer.set_doppler(True, True)
    renderer.set_debug_doppler(True)
    refused()
    renderer.set_debug_doppler(False)
    renderer.set_doppler(False, False)
    renderer.set_object_windows(windows[:-1])          # a count that is not the Object[]'s: refused at the launch, frames and events
    refused()
    renderer.set_object_windows(windows)
    records = renderer.render_events().copy()
    assert renderer.last_events_variant() == 2941
    renderer.set_object_windows(None)
    renderer.render_events()
    assert renderer.last_events_variant() == 941          # (so that a refused pass that launched or reported anything would show)
    renderer.set_object_windows(windows[:-1])
    refused(renderer.render_events)
    assert renderer.last_events_variant() == 941 and renderer.read_events().tobytes() != records.tobytes()
    refused(renderer.verify_frame)
    renderer.set_object_windows(windows)
    _assert_frame(_frame(renderer), good, "after the refusals")
    renderer.set_object_windows(None)


# ---- 6. physics: a sphere that goes out along +z at 0.6 c and comes back -----------------------------------------------------------------
def test_a_turnaround_is_seen_when_its_light_arrives(renderer):
    t_k, z_k = 10.0, 10.0
    wl = worldline.piecewise([(0.0, 0.0, 0.0, 4.0), (t_k, 0.0, 0.0, z_k), (2 * t_k, 0.0, 0.0, 4.0)])
    assert np.allclose(wl[0].velocity, (0, 0, 0.6)) and np.allclose(wl[1].velocity, (0, 0, -0.6))
    text = wl.to_dsl("Os", scale=(0.5, 0.5, 0.5), extra="c1,0.5,0.2") + "R\n"
    seen_at = t_k + z_k          # the turnaround's light reaches a camera at rest at the origin at t_k + |z_k|
    for camera_time, leg in ((seen_at - 1.5, 0), (seen_at + 1.5, 1)):
        scene = eo.scene_from_text(text, t=camera_time)
        assert scene.windows() is not None
        _setup(renderer, scene, W, H)
        renderer.set_object_windows(None)
        renderer.set_objects(scene)           # the scene's own `w` commands are passed on
        ev = renderer.render_events()
        assert renderer.last_events_variant() == 2944
        assert ev[H // 2, W // 2]["object"] == leg, (camera_time, ev[H // 2, W // 2])
        assert set(np.unique(ev["object"]).tolist()) == {-1, leg}, "exactly one leg is visible"
        hit = ev["object"] >= 0
        assert wo.accepts(scene.windows(), ev["object"][hit], ev["event"][..., 0][hit]).all()
        renderer.set_object_windows(None)


def test_set_objects_follows_the_scenes_windows_and_leaves_hand_set_ones_alone(renderer):
    body = "Os p0,0,6,0,0,1,0,1,1,1 c1,0.5,0.2{}\nOc p2,0,8,0,0,1,0,1,1,1 c0.2,0.5,1\nR\n"
    with_w, without = eo.scene_from_text(body.format(" w-inf,0")), eo.scene_from_text(body.format(""))
    _setup(renderer, without, W, H)
    renderer.render()
    assert renderer.last_variant() == 44
    renderer.set_objects(with_w)
    renderer.render()
    assert renderer.last_variant() == 2044
    renderer.set_objects(without)            # a scene without `w` after one with: the windows it passed on are cleared
    renderer.render()
    assert renderer.last_variant() == 44
    renderer.set_object_windows(with_w.windows())
    renderer.set_objects(without)            # windows set by hand stay
    renderer.render()
    assert renderer.last_variant() == 2044
    renderer.set_object_windows(None)
