"""rpt_render_ballistics on the MI355X: the device's own pre-pass framebuffer and records go through
tests/native/ballistics_oracle.c, the C restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and both
counts of rpt_last_ballistics, and leave the record buffer as it was.  Feeding the reference what the device rendered isolates kernels
1150, 1152 and 1131 from every other.  Scenes, cameras, sizes and sets are those of tests/ballistics_cases.py — the particle cases'
crafted set, set in motion —, built from the device's own records; their non-vacuity is asserted here on those records and in
tests/test_ballistics_model.py on CPU frames.  Frames are 128 x 72 at most, sets 4096 records at most."""
import numpy as np
import pytest

import ballistics_cases as bc
import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
from relativitypathtracer_amd import ballistics
from relativitypathtracer_amd.renderer import RenderError, Renderer, raymap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bc.build_library(tmp_path_factory.mktemp("ballistics"))


@pytest.fixture(scope="module")
def particles_lib(tmp_path_factory):
    return pc.build_library(tmp_path_factory.mktemp("ballistics_particles"))


@pytest.fixture(scope="module")
def stars_lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("ballistics_stars"))


_SCENES = {}


def _scene(name, motion, interval=-1):
    key = (name, motion, interval)
    if key not in _SCENES:
        _SCENES[key] = eo.load_scene(name, motion, interval)
    return _SCENES[key]


def _setup(r, scene, W, H, camera, flags=0):
    r.set_variant(0)
    r.set_msaa(1)
    r.set_adaptive_aa(1, 8)
    r.set_doppler(bool(flags & 1), bool(flags & 2))
    r.set_environment(None)
    r.set_environment_frame(scene.camera_lorentz()[1])
    r.set_debug_rgb(False)
    r.set_overlay()
    r.set_stars(None)
    r.set_particles(None)
    r.set_particle_options()
    r.set_particle_lighting()
    r.set_ballistic_options()
    r.set_ballistic_temperatures(None)
    sc.setup_camera(r, camera)
    r.upload_scene(scene)
    r.set_object_windows(scene.windows())
    r.set_readouts(None)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _view(scene, camera, W, H, flags, **options):
    return bc.view(camera, W, H, scene.params["interval"], flags, scene.params["white_point"], **options)


def _same_pixels(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 16)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 16)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at pixel {k}: got {g[k].tolist()} want {w[k].tolist()}")


def _frames(r):
    """A fresh colour frame and event frame: (framebuffer, records), both copies."""
    r.render()
    before = r.read_framebuffer().copy()
    return before, r.render_events().copy()


def _pass_against_oracle(r, lib, v, objects, bs, what, passes=1, xg=None, async_=False):
    """Colour frame, event frame, the pass `passes` times with the set the context HOLDS, against the oracle applied as often."""
    before, records = _frames(r)
    for _ in range(passes):
        r.render_ballistics(async_=async_)
    if async_:
        r.sync()
    after = r.read_framebuffer().copy()
    want, counts = before, None
    for _ in range(passes):
        want, counts = bc.oracle_pass(lib, v, objects, bs, want, records, xg)
    _same_pixels(after, want, what)
    assert r.last_ballistics() == counts, f"{what}: rpt_last_ballistics {r.last_ballistics()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


@pytest.mark.parametrize("size", bc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(bc.CAMERAS))
@pytest.mark.parametrize("motion", bc.MOTIONS)
@pytest.mark.parametrize("scene_name", bc.SCENES)
def test_the_pass_equals_the_c_oracle(renderer, lib, scene_name, motion, name, size):
    """Light delay on and off, every Doppler setting, the inverse square on and off, the depth bias 0 and 1e-3 of the largest dist; the
    set is tests/ballistics_cases.py's crafted one, built from the device's own records of the view."""
    W, H = size
    camera = bc.CAMERAS[name]
    for interval in bc.INTERVALS:
        scene = _scene(scene_name, motion, interval)
        objects = pc.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera)
        _, records = _frames(renderer)
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        bs, groups, bias = bc.crafted(records, objects, camera, W, H, interval)
        bc.check_shows_something(lib, records, objects, camera, W, H, interval, bs, groups, bias, what)
        renderer.set_ballistics(bs)
        for flags in bc.FLAGS:
            renderer.set_doppler(bool(flags & 1), bool(flags & 2))
            seen = {}
            for inverse_square in (False, True):
                for depth_bias in (0.0, bias):
                    renderer.set_ballistic_options(inverse_square=inverse_square, depth_bias=depth_bias)
                    v = _view(scene, camera, W, H, flags, inverse_square=inverse_square, depth_bias=depth_bias)
                    case = f"{what} flags {flags} inverse square {inverse_square} bias {depth_bias:g}"
                    before, records_now, after, counts = _pass_against_oracle(renderer, lib, v, objects, bs, case)
                    assert records_now.tobytes() == records.tobytes(), f"{case}: the event frame is not the one the set was built from"
                    assert 0 < counts[0] < len(bs), case
                    seen[(inverse_square, depth_bias)] = counts[0]
                    # the untouched bytes
                    assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]) and np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"])
                    assert np.array_equal(after["unspecified"], before["unspecified"])
                    assert int((after["rgba"] != before["rgba"]).any(axis=1).sum()) == counts[1]
                    if not flags & 1 and not inverse_square:
                        assert counts[1] > 0, case
            assert seen[(False, bias)] >= seen[(False, 0.0)] and seen[(True, 0.0)] == seen[(False, 0.0)], f"{what} flags {flags}: {seen}"


def _case(renderer, W=128, H=72, flags=3, motion="0.9c", name="pinhole", scene_name="cubes"):
    """One parity case set up on the renderer: (scene, camera, objects, set, groups, bias, the particle set it was made from)."""
    scene = _scene(scene_name, motion)
    camera = bc.CAMERAS[name]
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, flags)
    _, records = _frames(renderer)
    ps, groups, bias = pc.crafted(records, objects, camera, W, H, -1)
    return scene, camera, objects, bc.moving(ps, groups, objects, camera, W, H, -1), groups, bias, ps


@pytest.mark.parametrize("motion", bc.MOTIONS)
@pytest.mark.parametrize("name", ["pinhole", "sphere"])
def test_at_rest_and_always_shining_the_pass_is_the_particle_pass(renderer, lib, particles_lib, name, motion):
    """u = 0 and the window open: the bytes and tallies of rpt_render_particles on the same frame, and of both oracles."""
    W, H = 128, 72
    for interval in bc.INTERVALS:
        scene = _scene("cubes", motion, interval)
        camera = bc.CAMERAS[name]
        objects = pc.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera, 3)
        _, records = _frames(renderer)
        ps, _, bias = pc.crafted(records, objects, camera, W, H, interval)
        ps = bc.without_negative_zero(ps)
        bs = bc.from_particles(ps)
        renderer.set_ballistics(bs)
        renderer.set_ballistic_options(inverse_square=True, depth_bias=bias)
        v = _view(scene, camera, W, H, 3, inverse_square=True, depth_bias=bias)
        _, _, ballistic_frame, counts = _pass_against_oracle(renderer, lib, v, objects, bs, f"u = 0, {name} {motion} interval {interval}")
        renderer.set_particles(ps)
        renderer.set_particle_options(inverse_square=True, depth_bias=bias)
        before, records_now = _frames(renderer)
        renderer.render_particles()
        particle_frame = renderer.read_framebuffer().copy()
        assert records_now.tobytes() == records.tobytes()
        _same_pixels(ballistic_frame, particle_frame, f"u = 0 against rpt_render_particles, {name} {motion} interval {interval}")
        assert renderer.last_particles() == counts and counts[0] > 0
        want, want_counts = pc.oracle_pass(particles_lib, v, objects, ps, before, records)
        assert want.tobytes() == particle_frame.tobytes() and want_counts == counts
        renderer.set_particles(None)


def test_thermal_records_equal_the_c_oracle(renderer, lib):
    """Kernel 1152 at 0.9c: temperatures 0 (the record keeps S_f), 3000, 6000 and 3e4 K mixed over the crafted set, every Doppler setting."""
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, 128, 72, 3, "0.9c", "sphere")
    T = np.array([0.0, 3000.0, 6000.0, 3e4], dtype=np.float32)[np.arange(len(bs)) % 4]
    xg = bc.x_green32(lib, T)
    renderer.set_ballistics(bs, T)
    plain = None
    for flags in bc.FLAGS:
        renderer.set_doppler(bool(flags & 1), bool(flags & 2))
        v = _view(scene, camera, 128, 72, flags)
        _, _, after, counts = _pass_against_oracle(renderer, lib, v, objects, bs, f"thermal, flags {flags}", xg=xg)
        assert counts[0] > 0
        if flags == 3:
            plain = after
    renderer.set_ballistic_temperatures(None)           # back on kernel 1150, and another frame than the thermal one
    renderer.set_doppler(True, True)
    _, _, without, _ = _pass_against_oracle(renderer, lib, _view(scene, camera, 128, 72, 3), objects, bs, "the temperatures taken away")
    assert without.tobytes() != plain.tobytes()


def test_a_jet_beyond_the_band_is_black_without_a_temperature_and_lit_with_one(renderer, lib):
    """Blobs that come at the camera at 0.8 c, D = 3 in their objects' frames: S_f has cut the shifted spectrum to zero — for all three
    output samples from D = 1.8 * 546.1 / 435.8 = 2.26 on (between 1.8 and that the blue output still reads the red end of the input) —
    while a blackbody stays in the band."""
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, 128, 72, 1, "rest", "pinhole")
    jet = bs[groups["near"]].copy()
    place = bc.oracle_place(lib, _view(scene, camera, 128, 72, 1), objects, jet)
    jet = jet[place["visible"] & (place["D"] > 2.3)]       # (some ride cubes that move away themselves)
    assert len(jet) >= 20, len(jet)
    renderer.set_ballistics(jet)
    v = _view(scene, camera, 128, 72, 1)
    before, _, after, counts = _pass_against_oracle(renderer, lib, v, objects, jet, "the jet, no temperatures")
    assert counts[0] > 0 and counts[1] == 0 and after.tobytes() == before.tobytes()
    T = np.full(len(jet), 6000.0, dtype=np.float32)
    renderer.set_ballistic_temperatures(T)
    _, _, _, counts = _pass_against_oracle(renderer, lib, v, objects, jet, "the jet at 6000 K", xg=bc.x_green32(lib, T))
    assert counts[1] > 0


def test_the_sums_do_not_depend_on_the_order_and_two_passes_add_twice(renderer, lib):
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, 128, 72, 2, "rest", "pinhole")
    v = _view(scene, camera, 128, 72, 2, inverse_square=True)
    renderer.set_ballistic_options(inverse_square=True)
    renderer.set_ballistics(bs)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, objects, bs, "the set as given")
    shuffled = bs[np.random.default_rng(2).permutation(len(bs))]
    renderer.set_ballistics(shuffled)
    _, _, second, counts_shuffled = _pass_against_oracle(renderer, lib, v, objects, shuffled, "the set shuffled")
    assert forward.tobytes() == second.tobytes() and counts == counts_shuffled
    renderer.set_ballistics(bs[::-1].copy())
    _, _, third, _ = _pass_against_oracle(renderer, lib, v, objects, bs[::-1].copy(), "the set reversed")
    assert third.tobytes() == forward.tobytes()
    renderer.set_ballistics(bs)
    _, _, twice, _ = _pass_against_oracle(renderer, lib, v, objects, bs, "the pass twice on one frame", passes=2)
    assert twice.tobytes() != forward.tobytes()


@pytest.mark.parametrize("count", [1, 256, 257])
def test_a_ragged_last_workgroup(renderer, lib, count):
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, 67, 41, 0, "rest", "pinhole")
    s = groups["surface"]
    some = np.concatenate([bs[groups["near"]], bs[groups["on pixels"]], bs[groups["far"]], bs[s]])[:count]
    assert len(some) == count
    renderer.set_ballistics(some)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, some, f"{count} records")
    assert 0 < counts[0] <= count and counts[1] > 0


def test_the_accumulator_is_clean_afterwards(renderer, lib, stars_lib):
    """A star pass behind a ballistic pass equals its oracle, and so does a ballistic pass behind the stars."""
    scene, camera, objects, bs, groups, bias, _ = _case(renderer)
    renderer.set_ballistics(bs)
    v = _view(scene, camera, 128, 72, 3)
    E = scene.camera_lorentz()[1]
    cat, _ = sc.catalogue(camera, 128, 72, E, -1)
    sv = sc.view(camera, 128, 72, E, -1, 3, scene.params["white_point"])
    renderer.set_stars(cat)
    before, records = _frames(renderer)
    renderer.render_ballistics()
    renderer.render_stars()
    renderer.render_ballistics()
    got = renderer.read_framebuffer().copy()
    want, first = bc.oracle_pass(lib, v, objects, bs, before, records)
    want, star_counts = sc.oracle_pass(stars_lib, sv, cat, want, records)
    want, second = bc.oracle_pass(lib, v, objects, bs, want, records)
    _same_pixels(got, want, "ballistics, stars, ballistics")
    assert renderer.last_stars() == star_counts and renderer.last_ballistics() == second and first[0] == second[0] > 0
    renderer.set_stars(None)


def test_the_objects_own_window_is_not_applied(renderer, lib):
    """Lamps at rest in the frames of a body of three legs, as ballistic records: every leg's show, whatever its window holds."""
    W, H = 128, 72
    wl, scene, ps = pc.turnaround()
    camera = bc.CAMERAS["pinhole"]
    objects = pc.scene_objects(scene, camera)
    assert scene.windows() is not None
    _setup(renderer, scene, W, H, camera, 3)
    bs = bc.from_particles(bc.without_negative_zero(ps))
    renderer.set_ballistics(bs)
    v = _view(scene, camera, W, H, 3)
    _, _, windowed, counts = _pass_against_oracle(renderer, lib, v, objects, bs, "three legs, windows set")
    renderer.set_object_windows(None)
    _, _, free, free_counts = _pass_against_oracle(renderer, lib, v, objects, bs, "three legs, no windows")
    assert counts[0] > 0


def test_off_means_off(renderer, lib):
    fresh = Renderer(0)
    try:
        fresh.render_ballistics()                       # no set: nothing is checked, not even that a scene is there
        assert fresh.last_ballistics() == (0, 0)
    finally:
        fresh.close()
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, 67, 41, 0, "rest")
    renderer.set_ballistics(None)
    before, _ = _frames(renderer)
    variant = renderer.last_variant()
    renderer.render_ballistics()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_variant() == variant and renderer.last_ballistics() == (0, 0)
    renderer.set_ballistics(bs)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, bs, "a set first")
    assert counts[1] > 0
    renderer.set_ballistics(np.zeros(0, dtype=ballistics.BALLISTIC_DTYPE))
    before, _ = _frames(renderer)
    renderer.render_ballistics()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_ballistics() == (0, 0)
    assert renderer._lib.rpt_set_ballistics(renderer._h, None, 5) == 0          # NULL switches off whatever the count
    renderer.render_ballistics()
    assert renderer.read_framebuffer().tobytes() == before.tobytes()


def test_what_the_setters_refuse(renderer, lib):
    scene, camera, objects, good, groups, bias, _ = _case(renderer, 67, 41, 0, "rest")
    renderer.set_ballistics(good)
    renderer.set_ballistic_options(inverse_square=True, depth_bias=bias)
    for field, k, value, words in (("pos", 0, np.nan, "finite"), ("pos", 2, np.inf, "finite"), ("rgb", 1, -np.inf, "finite"), ("u", 2, np.nan, "finite"),
                                   ("u", 0, np.inf, "finite"), ("u", 1, 1000.5, "beyond 1000"), ("u", 1, -1000.5, "beyond 1000"),
                                   ("rgb", 0, -1e-20, "negative"), ("object", None, -1, "object is negative"), ("t0", None, np.nan, "not a number"),
                                   ("t1", None, np.nan, "not a number"), ("t1", None, -np.inf, "empty")):
        bad = good.copy()
        if k is None:
            bad[field][7] = value
        else:
            bad[field][7, k] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_ballistics: entry 7: .*" + words):
            renderer.set_ballistics(bad)
    bad = good.copy()
    bad["t0"][7], bad["t1"][7] = 2.0, 2.0
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_ballistics: entry 7: .*empty"):
        renderer.set_ballistics(bad)
    lib_hip = renderer._lib
    assert lib_hip.rpt_set_ballistics(renderer._h, None, -1) == 1 and lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_ballistics:")
    assert lib_hip.rpt_set_ballistics(renderer._h, None, (1 << 22) + 1) == 1
    for flags, depth_bias in ((2, 0.0), (-1, 0.0), (0, -1e-6), (1, float("nan")), (0, float("inf"))):
        assert lib_hip.rpt_set_ballistic_options(renderer._h, flags, depth_bias) == 1
        assert lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_ballistic_options:")
    # every refusal kept the set and the options that were there
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0, inverse_square=True, depth_bias=bias), objects, good, "after the refusals")


def test_what_the_launch_refuses(renderer, lib):
    W, H = 67, 41
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, W, H, 0, "rest")
    renderer.set_ballistics(bs)
    v = _view(scene, camera, W, H, 0)

    def refused(code, words):
        with pytest.raises(RenderError, match=rf"failed \({code}\): rpt_render_ballistics: .*{words}") as e:
            renderer.render_ballistics()
        assert e.value.code == code

    # a ray map has no inverse
    renderer.set_raymap(raymap("fisheye", W, H))
    renderer.set_projection("raymap")
    _frames(renderer)
    refused(1, "RPT_PROJECTION_RAYMAP")
    renderer.set_projection("pinhole")
    renderer.set_raymap(None)
    _pass_against_oracle(renderer, lib, v, objects, bs, "after the ray map")
    # an interval the cone has no closed form for
    five = eo.load_scene("cubes", "rest", 5)
    renderer.set_scene_params(five, W, H)
    _frames(renderer)
    refused(1, "interval is 5")
    renderer.set_scene_params(scene, W, H)
    _pass_against_oracle(renderer, lib, v, objects, bs, "after interval 5")
    # a set that names object index object_count: refused at the launch
    beyond = bs.copy()
    beyond["object"][5] = len(objects)
    renderer.set_ballistics(beyond)
    _frames(renderer)
    refused(1, f"names object {len(objects)}")
    renderer.set_ballistics(bs)
    _pass_against_oracle(renderer, lib, v, objects, bs, "after the object beyond the Object[]")
    # temperatures whose count is not the set's
    renderer.set_ballistic_temperatures(np.full(len(bs) - 1, 6000.0, dtype=np.float32))
    _frames(renderer)
    refused(1, f"{len(bs) - 1} temperatures are set")
    renderer.set_ballistic_temperatures(None)
    _pass_against_oracle(renderer, lib, v, objects, bs, "after the temperatures")


def test_async_and_sync_give_the_blocking_bytes(renderer, lib):
    scene, camera, objects, bs, groups, bias, _ = _case(renderer, 128, 72, 3, "0.9c", "lens")
    renderer.set_ballistics(bs)
    v = _view(scene, camera, 128, 72, 3)
    _, _, blocking, counts = _pass_against_oracle(renderer, lib, v, objects, bs, "blocking")
    _, _, enqueued, counts_async = _pass_against_oracle(renderer, lib, v, objects, bs, "async, then sync", async_=True)
    assert blocking.tobytes() == enqueued.tobytes() and counts == counts_async
