"""rpt_render_rockets on the MI355X: the device's own pre-pass framebuffer and records go through
tests/native/rockets_oracle.c, the C restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and both
counts of rpt_last_rockets, and leave the record buffer as it was.  Feeding the reference what the device rendered isolates kernels
1160, 1162 and 1131 from every other.  Scenes, cameras, sizes and sets are those of tests/rockets_cases.py — the ballistic cases' crafted
set with accelerations laid over it, fast rockets and rockets beyond the horizon —, built from the device's own records; their
non-vacuity is asserted here on those records and in tests/test_rockets_model.py on CPU frames.  Frames are 128 x 72 at most, sets 4096
records at most."""
import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import rockets_cases as rc
import stars_cases as sc
from relativitypathtracer_amd import rockets
from relativitypathtracer_amd.renderer import RenderError, Renderer, raymap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rc.build_library(tmp_path_factory.mktemp("rockets"))


@pytest.fixture(scope="module")
def stars_lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("rockets_stars"))


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
    r.set_ballistics(None)
    r.set_rocket_options()
    r.set_rocket_temperatures(None)
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
    return rc.view(camera, W, H, scene.params["interval"], flags, scene.params["white_point"], **options)


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


def _pass_against_oracle(r, lib, v, objects, rs, what, passes=1, xg=None, async_=False):
    """Colour frame, event frame, the pass `passes` times with the set the context HOLDS, against the oracle applied as often."""
    before, records = _frames(r)
    for _ in range(passes):
        r.render_rockets(async_=async_)
    if async_:
        r.sync()
    after = r.read_framebuffer().copy()
    want, counts = before, None
    for _ in range(passes):
        want, counts = rc.oracle_pass(lib, v, objects, rs, want, records, xg)
    _same_pixels(after, want, what)
    assert r.last_rockets() == counts, f"{what}: rpt_last_rockets {r.last_rockets()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(rc.CAMERAS))
@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("scene_name", rc.SCENES)
def test_the_pass_equals_the_c_oracle(renderer, lib, scene_name, motion, name, size):
    """Light delay on and off, every Doppler setting, the inverse square on and off, the depth bias 0 and 1e-3 of the largest dist; the
    set is tests/rockets_cases.py's crafted one, built from the device's own records of the view."""
    W, H = size
    camera = rc.CAMERAS[name]
    for interval in rc.INTERVALS:
        scene = _scene(scene_name, motion, interval)
        objects = pc.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera)
        _, records = _frames(renderer)
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        rs, groups, bias = rc.crafted(records, objects, camera, W, H, interval)
        rc.check_shows_something(lib, records, objects, camera, W, H, interval, rs, groups, bias, what)
        renderer.set_rockets(rs)
        for flags in rc.FLAGS:
            renderer.set_doppler(bool(flags & 1), bool(flags & 2))
            seen = {}
            for inverse_square in (False, True):
                for depth_bias in (0.0, bias):
                    renderer.set_rocket_options(inverse_square=inverse_square, depth_bias=depth_bias)
                    v = _view(scene, camera, W, H, flags, inverse_square=inverse_square, depth_bias=depth_bias)
                    case = f"{what} flags {flags} inverse square {inverse_square} bias {depth_bias:g}"
                    before, records_now, after, counts = _pass_against_oracle(renderer, lib, v, objects, rs, case)
                    assert records_now.tobytes() == records.tobytes(), f"{case}: the event frame is not the one the set was built from"
                    assert 0 < counts[0] < len(rs), case
                    seen[(inverse_square, depth_bias)] = counts[0]
                    # the untouched bytes
                    assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]) and np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"])
                    assert np.array_equal(after["unspecified"], before["unspecified"])
                    assert int((after["rgba"] != before["rgba"]).any(axis=1).sum()) == counts[1]
                    if not flags & 1 and not inverse_square:
                        assert counts[1] > 0, case
            assert seen[(False, bias)] >= seen[(False, 0.0)] and seen[(True, 0.0)] == seen[(False, 0.0)], f"{what} flags {flags}: {seen}"


def _case(renderer, W=128, H=72, flags=3, motion="0.9c", name="pinhole", scene_name="cubes"):
    """One parity case set up on the renderer: (scene, camera, objects, set, groups, bias)."""
    scene = _scene(scene_name, motion)
    camera = rc.CAMERAS[name]
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, flags)
    _, records = _frames(renderer)
    rs, groups, bias = rc.crafted(records, objects, camera, W, H, -1)
    return scene, camera, objects, rs, groups, bias


def test_thermal_records_equal_the_c_oracle(renderer, lib):
    """Kernel 1162 at 0.9c: temperatures 0 (the record keeps S_f), 3000, 6000 and 3e4 K mixed over the crafted set, every Doppler setting."""
    scene, camera, objects, rs, groups, bias = _case(renderer, 128, 72, 3, "0.9c", "sphere")
    T = np.array([0.0, 3000.0, 6000.0, 3e4], dtype=np.float32)[np.arange(len(rs)) % 4]
    xg = rc.x_green32(lib, T)
    renderer.set_rockets(rs, T)
    plain = None
    for flags in rc.FLAGS:
        renderer.set_doppler(bool(flags & 1), bool(flags & 2))
        v = _view(scene, camera, 128, 72, flags)
        _, _, after, counts = _pass_against_oracle(renderer, lib, v, objects, rs, f"thermal, flags {flags}", xg=xg)
        assert counts[0] > 0
        if flags == 3:
            plain = after
    renderer.set_rocket_temperatures(None)           # back on kernel 1160, and another frame than the thermal one
    renderer.set_doppler(True, True)
    _, _, without, _ = _pass_against_oracle(renderer, lib, _view(scene, camera, 128, 72, 3), objects, rs, "the temperatures taken away")
    assert without.tobytes() != plain.tobytes()


def test_the_sums_do_not_depend_on_the_order_and_two_passes_add_twice(renderer, lib):
    scene, camera, objects, rs, groups, bias = _case(renderer, 128, 72, 2, "rest", "pinhole")
    v = _view(scene, camera, 128, 72, 2, inverse_square=True)
    renderer.set_rocket_options(inverse_square=True)
    renderer.set_rockets(rs)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, objects, rs, "the set as given")
    shuffled = rs[np.random.default_rng(2).permutation(len(rs))]
    renderer.set_rockets(shuffled)
    _, _, second, counts_shuffled = _pass_against_oracle(renderer, lib, v, objects, shuffled, "the set shuffled")
    assert forward.tobytes() == second.tobytes() and counts == counts_shuffled
    renderer.set_rockets(rs[::-1].copy())
    _, _, third, _ = _pass_against_oracle(renderer, lib, v, objects, rs[::-1].copy(), "the set reversed")
    assert third.tobytes() == forward.tobytes()
    renderer.set_rockets(rs)
    _, _, twice, _ = _pass_against_oracle(renderer, lib, v, objects, rs, "the pass twice on one frame", passes=2)
    assert twice.tobytes() != forward.tobytes()


@pytest.mark.parametrize("count", [1, 256, 257])
def test_a_ragged_last_workgroup(renderer, lib, count):
    scene, camera, objects, rs, groups, bias = _case(renderer, 67, 41, 0, "rest", "pinhole")
    some = np.concatenate([rs[groups["near"]], rs[groups["on pixels"]], rs[groups["far"]], rs[groups["surface"]]])[:count]
    assert len(some) == count
    renderer.set_rockets(some)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, some, f"{count} records")
    assert 0 < counts[0] <= count and counts[1] > 0


def test_the_accumulator_is_clean_afterwards(renderer, lib, stars_lib):
    """A star pass behind a rocket pass equals its oracle, and so does a rocket pass behind the stars."""
    scene, camera, objects, rs, groups, bias = _case(renderer)
    renderer.set_rockets(rs)
    v = _view(scene, camera, 128, 72, 3)
    E = scene.camera_lorentz()[1]
    cat, _ = sc.catalogue(camera, 128, 72, E, -1)
    sv = sc.view(camera, 128, 72, E, -1, 3, scene.params["white_point"])
    renderer.set_stars(cat)
    before, records = _frames(renderer)
    renderer.render_rockets()
    renderer.render_stars()
    renderer.render_rockets()
    got = renderer.read_framebuffer().copy()
    want, first = rc.oracle_pass(lib, v, objects, rs, before, records)
    want, star_counts = sc.oracle_pass(stars_lib, sv, cat, want, records)
    want, second = rc.oracle_pass(lib, v, objects, rs, want, records)
    _same_pixels(got, want, "rockets, stars, rockets")
    assert renderer.last_stars() == star_counts and renderer.last_rockets() == second and first[0] == second[0] > 0
    renderer.set_stars(None)


def test_a_set_wholly_beyond_the_horizon_changes_no_byte(renderer, lib):
    scene, camera, objects, rs, groups, bias = _case(renderer, 128, 72, 3, "rest", "sphere")
    gone = rs[groups["horizon"]].copy()
    assert len(gone) == 2 * rc.HORIZON
    renderer.set_rockets(gone)
    before, _, after, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 128, 72, 3), objects, gone, "beyond the horizon")
    assert counts == (0, 0) and after.tobytes() == before.tobytes()
    # the same rockets without their acceleration are in front of the camera like any other: the horizon alone hid them
    coasting = gone.copy()
    coasting["acc"] = 0.0
    renderer.set_rockets(coasting)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 128, 72, 3), objects, coasting, "the same rockets, coasting")
    assert counts[0] > 0


def test_off_means_off(renderer, lib):
    fresh = Renderer(0)
    try:
        fresh.render_rockets()                       # no set: nothing is checked, not even that a scene is there
        assert fresh.last_rockets() == (0, 0)
    finally:
        fresh.close()
    scene, camera, objects, rs, groups, bias = _case(renderer, 67, 41, 0, "rest")
    renderer.set_rockets(None)
    before, _ = _frames(renderer)
    variant = renderer.last_variant()
    renderer.render_rockets()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_variant() == variant and renderer.last_rockets() == (0, 0)
    renderer.set_rockets(rs)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, rs, "a set first")
    assert counts[1] > 0
    renderer.set_rockets(np.zeros(0, dtype=rockets.ROCKET_DTYPE))
    before, _ = _frames(renderer)
    renderer.render_rockets()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_rockets() == (0, 0)
    assert renderer._lib.rpt_set_rockets(renderer._h, None, 5) == 0          # NULL switches off whatever the count
    renderer.render_rockets()
    assert renderer.read_framebuffer().tobytes() == before.tobytes()


def test_what_the_setters_refuse(renderer, lib):
    scene, camera, objects, good, groups, bias = _case(renderer, 67, 41, 0, "rest")
    renderer.set_rockets(good)
    renderer.set_rocket_options(inverse_square=True, depth_bias=bias)
    for field, k, value, words in (("pos", 0, np.nan, "finite"), ("pos", 2, np.inf, "finite"), ("rgb", 1, -np.inf, "finite"), ("u", 2, np.nan, "finite"),
                                   ("u", 0, np.inf, "finite"), ("u", 1, 1000.5, "u .* beyond 1000"), ("u", 1, -1000.5, "u .* beyond 1000"),
                                   ("acc", 0, np.nan, "finite"), ("acc", 2, -np.inf, "finite"), ("acc", 1, 1000.5, "acc .* beyond 1000"),
                                   ("acc", 0, -1000.5, "acc .* beyond 1000"), ("reserved", None, 1.0, "reserved must be 0"),
                                   ("reserved", None, np.nan, "reserved must be 0"),
                                   ("rgb", 0, -1e-20, "negative"), ("object", None, -1, "object is negative"), ("t0", None, np.nan, "not a number"),
                                   ("t1", None, np.nan, "not a number"), ("t1", None, -np.inf, "empty")):
        bad = good.copy()
        if k is None:
            bad[field][7] = value
        else:
            bad[field][7, k] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_rockets: entry 7: .*" + words):
            renderer.set_rockets(bad)
    bad = good.copy()
    bad["t0"][7], bad["t1"][7] = 2.0, 2.0
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_rockets: entry 7: .*empty"):
        renderer.set_rockets(bad)
    lib_hip = renderer._lib
    assert lib_hip.rpt_set_rockets(renderer._h, None, -1) == 1 and lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_rockets:")
    assert lib_hip.rpt_set_rockets(renderer._h, None, (1 << 22) + 1) == 1
    for flags, depth_bias in ((2, 0.0), (-1, 0.0), (0, -1e-6), (1, float("nan")), (0, float("inf"))):
        assert lib_hip.rpt_set_rocket_options(renderer._h, flags, depth_bias) == 1
        assert lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_rocket_options:")
    # every refusal kept the set and the options that were there
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0, inverse_square=True, depth_bias=bias), objects, good, "after the refusals")


def test_what_the_launch_refuses(renderer, lib):
    W, H = 67, 41
    scene, camera, objects, rs, groups, bias = _case(renderer, W, H, 0, "rest")
    renderer.set_rockets(rs)
    v = _view(scene, camera, W, H, 0)

    def refused(code, words):
        with pytest.raises(RenderError, match=rf"failed \({code}\): rpt_render_rockets: .*{words}") as e:
            renderer.render_rockets()
        assert e.value.code == code

    # no event frame of this view: a colour frame alone is not enough
    renderer.set_scene_params(scene, W + 1, H)
    renderer.render()
    refused(2, "the last colour frame and event frame are not both of the current width x height")
    renderer.set_scene_params(scene, W, H)
    _pass_against_oracle(renderer, lib, v, objects, rs, "after the missing event frame")
    # a ray map has no inverse
    renderer.set_raymap(raymap("fisheye", W, H))
    renderer.set_projection("raymap")
    _frames(renderer)
    refused(1, "RPT_PROJECTION_RAYMAP")
    renderer.set_projection("pinhole")
    renderer.set_raymap(None)
    _pass_against_oracle(renderer, lib, v, objects, rs, "after the ray map")
    # an interval the cone has no closed form for
    five = eo.load_scene("cubes", "rest", 5)
    renderer.set_scene_params(five, W, H)
    _frames(renderer)
    refused(1, "interval is 5")
    renderer.set_scene_params(scene, W, H)
    _pass_against_oracle(renderer, lib, v, objects, rs, "after interval 5")
    # a set that names object index object_count: refused at the launch
    beyond = rs.copy()
    beyond["object"][5] = len(objects)
    renderer.set_rockets(beyond)
    _frames(renderer)
    refused(1, f"names object {len(objects)}")
    renderer.set_rockets(rs)
    _pass_against_oracle(renderer, lib, v, objects, rs, "after the object beyond the Object[]")
    # temperatures whose count is not the set's
    renderer.set_rocket_temperatures(np.full(len(rs) - 1, 6000.0, dtype=np.float32))
    _frames(renderer)
    refused(1, f"{len(rs) - 1} temperatures are set")
    renderer.set_rocket_temperatures(None)
    _pass_against_oracle(renderer, lib, v, objects, rs, "after the temperatures")


def test_async_and_sync_give_the_blocking_bytes(renderer, lib):
    scene, camera, objects, rs, groups, bias = _case(renderer, 128, 72, 3, "0.9c", "lens")
    renderer.set_rockets(rs)
    v = _view(scene, camera, 128, 72, 3)
    _, _, blocking, counts = _pass_against_oracle(renderer, lib, v, objects, rs, "blocking")
    _, _, enqueued, counts_async = _pass_against_oracle(renderer, lib, v, objects, rs, "async, then sync", async_=True)
    assert blocking.tobytes() == enqueued.tobytes() and counts == counts_async
