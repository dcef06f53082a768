"""Thermal stars on the MI355X (kernel 1122 before 1121): the device's own pre-pass framebuffer and records go through
tests/native/thermal_oracle.c, and rpt_render_stars with rpt_set_star_temperatures must give those bytes — all 16 of every pixel — and
both counts of rpt_last_stars.  Scene, cameras, sizes, catalogue and temperatures are tests/thermal_cases.py's (their non-vacuity is
asserted in tests/test_thermal_model.py on CPU frames): `cubes` at 128 x 72 and 67 x 41, the pinhole and the full-circle equirect, at rest
and at 0.9 c, the four Doppler settings, interval -1 and 0; 2000 random stars plus crafted ones, T at 500 and 1e8, x_G = 0 mixed in."""
import ctypes as C

import numpy as np
import pytest

import events_oracle as eo
import stars_cases as sc
import thermal_cases as tc
from relativitypathtracer_amd import stars
from relativitypathtracer_amd.renderer import RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return tc.build_stars_library(tmp_path_factory.mktemp("thermal_stars"))


_SCENES = {}


def _scene(motion, interval=-1):
    key = (motion, interval)
    if key not in _SCENES:
        _SCENES[key] = eo.load_scene(tc.SCENE, motion, interval)
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
    r.set_particles(None)
    sc.setup_camera(r, camera)
    r.upload_scene(scene)
    r.set_object_windows(scene.windows())
    r.set_readouts(None)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _view(scene, camera, W, H, flags):
    return sc.view(camera, W, H, scene.camera_lorentz()[1], scene.params["interval"], flags, scene.params["white_point"])


def _same_pixels(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 16)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 16)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at pixel {k}: got {g[k].tolist()} want {w[k].tolist()}")


def _frames(r):
    r.render()
    before = r.read_framebuffer().copy()
    return before, r.render_events().copy()


def _pass_against_oracle(r, lib, v, cat, T, what):
    """Colour frame, event frame, the pass with the catalogue and the temperatures the context HOLDS (T None: none), against the oracle."""
    before, records = _frames(r)
    r.render_stars()
    after = r.read_framebuffer().copy()
    if T is None:
        want, counts = sc.oracle_pass(lib, v, cat, before, records)
    else:
        want, counts = tc.oracle_stars_pass(lib, v, cat, tc.x_green32(T), before, records)
    _same_pixels(after, want, what)
    assert r.last_stars() == counts, f"{what}: rpt_last_stars {r.last_stars()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


def _case(renderer, W=128, H=72, flags=3, motion="0.9c", name="pinhole"):
    scene = _scene(motion)
    camera = tc.CAMERAS[name]
    _setup(renderer, scene, W, H, camera, flags)
    _, records = _frames(renderer)
    cat, T, groups = tc.star_case(camera, W, H, scene.camera_lorentz()[1], -1, tc.miss_pixel(records, W, H))
    return scene, camera, cat, T, groups


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(tc.CAMERAS))
@pytest.mark.parametrize("motion", tc.MOTIONS)
def test_the_pass_equals_the_c_oracle(renderer, lib, motion, name, size):
    W, H = size
    camera = tc.CAMERAS[name]
    cat = T = groups = None
    for interval in tc.INTERVALS:
        scene = _scene(motion, interval)
        for flags in tc.FLAGS:
            what = f"{motion} {name} {W}x{H} interval {interval} flags {flags}"
            _setup(renderer, scene, W, H, camera, flags)
            if cat is None:
                _, records = _frames(renderer)
                cat, T, groups = tc.star_case(camera, W, H, scene.camera_lorentz()[1], -1, tc.miss_pixel(records, W, H))
                assert len(cat) <= 4096 and (T == 0).sum() > 500 and (T == tc.T_MIN).any() and (T == tc.T_MAX).any()
            v = _view(scene, camera, W, H, flags)
            renderer.set_stars(cat, T)
            _, records, thermal, counts = _pass_against_oracle(renderer, lib, v, cat, T, what)
            assert counts[1] > 0, what
            # an all-zero array, and none at all: the plain pass's frame, byte for byte
            renderer.set_star_temperatures(np.zeros(len(cat), dtype=np.float32))
            _, _, zeros, zero_counts = _pass_against_oracle(renderer, lib, v, cat, np.zeros(len(cat), dtype=np.float32), what + ", all-zero temperatures")
            renderer.set_star_temperatures(None)
            _, _, plain, plain_counts = _pass_against_oracle(renderer, lib, v, cat, None, what + ", no temperatures")
            assert zeros.tobytes() == plain.tobytes() and zero_counts == plain_counts, what
            if motion == "rest" or interval == 0 or not flags & 1:
                # camera at rest (D == 1 exactly for a star at rest in the scene's frame), light delay off, or no shift: nothing to add
                assert thermal.tobytes() == plain.tobytes() and counts == plain_counts, f"{what}: the temperatures changed a frame they have no part in"
            else:
                assert thermal.tobytes() != plain.tobytes(), f"{what}: the temperatures changed nothing"
                colours = tc.oracle_stars_colours(lib, v, cat, tc.x_green32(T))
                dark = tc.oracle_stars_colours(lib, v, cat, np.zeros(len(cat), dtype=np.float32))
                s = groups["out of band"]
                assert not np.any(dark["rgb"][s]) and np.all(colours["rgb"][s] > 0.0), f"{what}: the star S_f blacks out"


def test_a_thousand_thermal_stars_on_one_pixel_forwards_and_shuffled(renderer, lib):
    scene, camera, cat, T, groups = _case(renderer)
    v = _view(scene, camera, 128, 72, 3)
    renderer.set_stars(cat, T)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, cat, T, "the catalogue as given")
    assert groups["pile"].stop - groups["pile"].start == 1000 and np.all(T[groups["pile"]] > 0)
    order = np.random.default_rng(3).permutation(len(cat))
    for what, o in (("reversed", np.arange(len(cat))[::-1]), ("shuffled", order)):
        renderer.set_stars(cat[o].copy(), T[o].copy())
        _, _, other, other_counts = _pass_against_oracle(renderer, lib, v, cat[o].copy(), T[o].copy(), what)
        assert other.tobytes() == forward.tobytes() and other_counts == counts, what


def test_off_means_off_and_the_catalogue_keeps_its_temperatures(renderer, lib):
    scene, camera, cat, T, _ = _case(renderer, 67, 41)
    v = _view(scene, camera, 67, 41, 3)
    renderer.set_stars(cat, T)
    _, _, thermal, _ = _pass_against_oracle(renderer, lib, v, cat, T, "temperatures set")
    renderer.set_stars(cat[::-1].copy())                    # replacing the catalogue keeps the array: entry i now belongs to another star
    _pass_against_oracle(renderer, lib, v, cat[::-1].copy(), T, "the catalogue replaced, the temperatures kept")
    renderer.set_stars(cat)
    renderer.set_star_temperatures(None)
    _, _, plain, _ = _pass_against_oracle(renderer, lib, v, cat, None, "after NULL")
    assert plain.tobytes() != thermal.tobytes()
    renderer.set_star_temperatures(T)
    renderer.set_star_temperatures(np.zeros(0, dtype=np.float32))      # a count of 0 is NULL
    _, _, again, _ = _pass_against_oracle(renderer, lib, v, cat, None, "after a count of 0")
    assert again.tobytes() == plain.tobytes()
    renderer.set_star_temperatures(T)
    renderer.set_stars(None)                                # no catalogue: no pass, whatever the temperatures
    before, _ = _frames(renderer)
    renderer.render_stars()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_stars() == (0, 0)
    renderer.set_star_temperatures(None)


def test_what_the_calls_refuse(renderer, lib):
    scene, camera, cat, T, _ = _case(renderer, 67, 41)
    v = _view(scene, camera, 67, 41, 3)
    renderer.set_stars(cat, T)
    hip, h = renderer._lib, renderer._h
    for value, words in ((np.nan, "finite"), (np.inf, "finite"), (-np.inf, "finite"), (499.99997, "within 500"), (1.0000001e8, "within 500"),
                         (-5000.0, "within 500"), (1e-20, "within 500")):
        bad = T.copy()
        bad[7] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_star_temperatures: entry 7: .*" + words):
            renderer.set_star_temperatures(bad)
    assert hip.rpt_set_star_temperatures(h, T.ctypes.data_as(C.POINTER(C.c_float)), -1) == 1
    assert hip.rpt_last_error(h).decode().startswith("rpt_set_star_temperatures: count")
    assert hip.rpt_set_star_temperatures(h, None, (1 << 22) + 1) == 1 and hip.rpt_last_error(h).decode().startswith("rpt_set_star_temperatures: count")
    ends = T.copy()
    ends[7], ends[8] = tc.T_MIN, tc.T_MAX                   # both ends of the range are inside it
    renderer.set_star_temperatures(ends)
    _pass_against_oracle(renderer, lib, v, cat, ends, "both ends of the range")
    renderer.set_star_temperatures(T)
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_star_temperatures: entry 0: "):
        renderer.set_star_temperatures(np.full(3, 10.0, dtype=np.float32))
    _pass_against_oracle(renderer, lib, v, cat, T, "every refusal kept the array that was there")
    # a count that differs from the catalogue's: refused at the launch, whichever came last, and the context stays usable
    for short in (T[:-1].copy(), np.concatenate([T, T[:1]])):
        renderer.set_star_temperatures(short)
        _frames(renderer)
        with pytest.raises(RenderError, match=rf"failed \(1\): rpt_render_stars: {len(short)} temperatures are set .*the catalogue holds {len(cat)}") as e:
            renderer.render_stars()
        assert e.value.code == 1
        renderer.set_star_temperatures(T)
        _pass_against_oracle(renderer, lib, v, cat, T, "after the count mismatch")
    renderer.set_stars(cat[:100].copy())
    _frames(renderer)
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_stars: .*the catalogue holds 100"):
        renderer.render_stars()
    renderer.set_stars(cat)
    _pass_against_oracle(renderer, lib, v, cat, T, "after a shorter catalogue")
    renderer.set_star_temperatures(None)


def test_async_and_render_scene(renderer, lib):
    from relativitypathtracer_amd.renderer import render_scene
    scene, camera, cat, T, _ = _case(renderer)
    v = _view(scene, camera, 128, 72, 3)
    renderer.set_stars(cat, T)
    _, _, blocking, counts = _pass_against_oracle(renderer, lib, v, cat, T, "blocking")
    renderer.render_async()
    renderer.render_events(async_=True)
    renderer.render_stars(async_=True)
    renderer.sync()
    assert renderer.read_framebuffer().tobytes() == blocking.tobytes() and renderer.last_stars() == counts
    renderer.set_star_temperatures(None)
    W, H = 67, 41
    plain, _, records = render_scene(scene, W, H, events=True)
    small, Ts, _ = tc.star_case(camera, W, H, scene.camera_lorentz()[1], -1, tc.miss_pixel(records, W, H))
    lit, _, _ = render_scene(scene, W, H, stars=small, star_temperatures=Ts)
    want, _ = tc.oracle_stars_pass(lib, _view(scene, camera, W, H, 0), small, tc.x_green32(Ts), plain, records)
    _same_pixels(lit, want, "render_scene(stars=, star_temperatures=)")
    with pytest.raises(RenderError, match="rpt_render_stars: .*temperatures are set"):      # (the keyword reaches the context)
        render_scene(scene, W, H, stars=small, star_temperatures=Ts[:-1])
    cat2, T2 = stars.random_catalogue(100, 1, return_temperatures=True)
    renderer.set_stars(cat2, T2)                            # what random_catalogue returns is what the setter takes
    renderer.set_stars(None)
    renderer.set_star_temperatures(None)
