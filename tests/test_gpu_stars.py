"""rpt_render_stars on the MI355X: the device's own pre-pass framebuffer and records go through
tests/native/stars_oracle.c, the C restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and both counts
of rpt_last_stars.  Feeding the reference what the device rendered isolates kernels 1120 and 1121 from every other.  Scenes, cameras, sizes
and catalogues are those of tests/stars_cases.py, whose non-vacuity tests/test_stars_model.py asserts on the CPU.  Frames are 128 x 72
at most, catalogues 4096 stars at most."""
import numpy as np
import pytest

import events_oracle as eo
import stars_cases as sc
from relativitypathtracer_amd import Scene, stars
from relativitypathtracer_amd.events import overlay
from relativitypathtracer_amd.renderer import RenderError, Renderer, raymap

pytestmark = pytest.mark.gpu

OUTLINES = dict(outlines=True, outline_rgba=(255, 255, 255, 200), clock_step=0.5, clock_rgba=(0, 255, 255, 160))


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("stars"))


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
    sc.setup_camera(r, camera)
    r.upload_scene(scene)
    r.set_object_windows(scene.windows())
    r.set_readouts(None)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _view(scene, camera, W, H, flags, E=None):
    return sc.view(camera, W, H, scene.camera_lorentz()[1] if E is None else E, scene.params["interval"], flags, scene.params["white_point"])


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


def _pass_against_oracle(r, lib, v, cat, what, passes=1):
    """Colour frame, event frame, the pass `passes` times with the catalogue the context HOLDS, against the oracle applied as often."""
    before, records = _frames(r)
    for _ in range(passes):
        r.render_stars()
    after = r.read_framebuffer().copy()
    want, counts = before, None
    for _ in range(passes):
        want, counts = sc.oracle_pass(lib, v, cat, want, records)
    _same_pixels(after, want, what)
    assert r.last_stars() == counts, f"{what}: rpt_last_stars {r.last_stars()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(sc.CAMERAS))
@pytest.mark.parametrize("motion", sc.MOTIONS)
@pytest.mark.parametrize("scene_name", sc.SCENES)
def test_the_pass_equals_the_c_oracle(renderer, lib, scene_name, motion, name, size):
    """Every Doppler setting with light delay on and off; the catalogue is random_catalogue(2000) plus the crafted stars."""
    W, H = size
    camera = sc.CAMERAS[name]
    cat = None
    for interval in sc.INTERVALS:
        scene = _scene(scene_name, motion, interval)
        for flags in sc.FLAGS:
            what = f"{scene_name} {motion} {name} {W}x{H} interval {interval} flags {flags}"
            _setup(renderer, scene, W, H, camera, flags)
            if cat is None:         # the 1000 stars go onto a miss pixel of this view, found in the device's own records
                _, records = _frames(renderer)
                hit = (records["object"] >= 0).reshape(H, W)
                assert hit.any() and (~hit).any(), f"{what}: {int(hit.sum())} hit pixels of {hit.size}"
                miss = np.nonzero(~hit[2:H - 2, 2:W - 2])
                cat, _ = sc.catalogue(camera, W, H, scene.camera_lorentz()[1], -1, (int(miss[1][0]) + 2, int(miss[0][0]) + 2))
                assert len(cat) <= 4096
            renderer.set_stars(cat)
            before, records, after, (inside, changed) = _pass_against_oracle(renderer, lib, _view(scene, camera, W, H, flags), cat, what)
            hit = records["object"].reshape(-1) >= 0
            assert hit.any() and (~hit).any(), what
            assert changed > 0 and (inside == len(cat) if name == "sphere" else 0 < inside < len(cat)), f"{what}: {inside} stars inside, {changed} pixels changed"
            # occlusion and the untouched bytes
            assert np.array_equal(after["rgba"][hit], before["rgba"][hit]), f"{what}: a hit pixel changed"
            assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]) and np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"])
            assert np.array_equal(after["unspecified"], before["unspecified"])
            assert int((after["rgba"] != before["rgba"]).any(axis=1).sum()) == changed


def test_the_accumulator_is_clean_after_every_pass(renderer, lib):
    scene = _scene("cubes", "0.9c")
    camera = sc.CAMERAS["pinhole"]
    cat, _ = sc.catalogue(camera, 128, 72, scene.camera_lorentz()[1], -1)
    _setup(renderer, scene, 128, 72, camera, 3)
    renderer.set_stars(cat)
    v = _view(scene, camera, 128, 72, 3)
    _, _, first, _ = _pass_against_oracle(renderer, lib, v, cat, "first frame")
    _, _, second, _ = _pass_against_oracle(renderer, lib, v, cat, "second frame")
    assert first.tobytes() == second.tobytes()
    _pass_against_oracle(renderer, lib, v, cat, "the pass twice on one frame", passes=2)
    renderer.set_scene_params(scene, 67, 41)            # another size (a smaller frame in the same accumulator), and back
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 3), cat, "67 x 41 in between")
    renderer.set_scene_params(scene, 128, 72)
    _, _, again, _ = _pass_against_oracle(renderer, lib, v, cat, "back at 128 x 72")
    assert again.tobytes() == first.tobytes()
    fresh = Renderer(0)                                 # a larger frame than the context has had: a new accumulator
    try:
        _setup(fresh, scene, 67, 41, camera, 3)
        fresh.set_stars(cat)
        _pass_against_oracle(fresh, lib, _view(scene, camera, 67, 41, 3), cat, "a fresh context at 67 x 41")
        fresh.set_scene_params(scene, 128, 72)
        _, _, grown, _ = _pass_against_oracle(fresh, lib, v, cat, "grown to 128 x 72")
        assert grown.tobytes() == first.tobytes()
    finally:
        fresh.close()


def test_the_sums_do_not_depend_on_the_order(renderer, lib):
    """4096 stars ahead of a camera at gamma = 10 crowd into a few pixels; the reversed catalogue gives the same bytes."""
    W, H = 128, 72
    beta = float(np.sqrt(1.0 - 1.0 / 100.0))
    scene = Scene.from_file("cubes")
    scene.set_interval(-1)
    scene.set_camera((0.0, 0.0, beta), 0.0)
    scene.update_objects()
    camera = sc.CAMERAS["sphere"]
    cat = stars.random_catalogue(4096, 21, faintest=0.5)
    _setup(renderer, scene, W, H, camera, 2)            # beaming alone: at D = 20 the shift would move every colour out of the band
    v = _view(scene, camera, W, H, 2)
    place = sc.oracle_place(lib, v, cat)
    ahead = np.hypot(place["X"] - (W / 2 - 0.5), place["Y"] - (H / 2 - 0.5)) < 4.0
    assert ahead.sum() > 1500, f"only {int(ahead.sum())} of 4096 stars within 4 pixels of the apex"
    renderer.set_stars(cat)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, cat, "gamma 10, the catalogue as given")
    renderer.set_stars(cat[::-1].copy())
    _, _, backward, counts_reversed = _pass_against_oracle(renderer, lib, v, cat[::-1].copy(), "gamma 10, the catalogue reversed")
    assert forward.tobytes() == backward.tobytes() and counts == counts_reversed and counts[1] > 0
    shuffled = cat[np.random.default_rng(2).permutation(len(cat))]
    renderer.set_stars(shuffled)
    _, _, third, _ = _pass_against_oracle(renderer, lib, v, shuffled, "gamma 10, the catalogue shuffled")
    assert third.tobytes() == forward.tobytes()


def test_off_means_off(renderer, lib):
    scene = _scene("cubes", "rest")
    camera = sc.CAMERAS["pinhole"]
    W, H = 67, 41
    _setup(renderer, scene, W, H, camera)
    fresh = Renderer(0)
    try:
        fresh.render_stars()                            # no catalogue: nothing is checked, not even that a scene is there
        assert fresh.last_stars() == (0, 0)
    finally:
        fresh.close()
    renderer.set_stars(None)
    before, _ = _frames(renderer)
    variant = renderer.last_variant()
    renderer.render_stars()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_variant() == variant and renderer.last_stars() == (0, 0)
    cat, _ = sc.catalogue(camera, W, H, scene.camera_lorentz()[1], -1)
    renderer.set_stars(cat)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, W, H, 0), cat, "a catalogue first")
    assert counts[1] > 0
    renderer.set_stars(None)
    before, _ = _frames(renderer)
    renderer.render_stars()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_variant() == variant and renderer.last_stars() == (0, 0)
    renderer.set_stars(np.zeros(0, dtype=stars.STAR_DTYPE))
    renderer.render_stars()
    assert renderer.read_framebuffer().tobytes() == before.tobytes()


def test_what_rpt_set_stars_refuses(renderer, lib):
    scene = _scene("cubes", "rest")
    camera = sc.CAMERAS["pinhole"]
    W, H = 67, 41
    _setup(renderer, scene, W, H, camera)
    good, _ = sc.catalogue(camera, W, H, scene.camera_lorentz()[1], -1)
    renderer.set_stars(good)
    for field, k, value, words in (("dir", 0, np.nan, "finite"), ("dir", 2, np.inf, "finite"), ("rgb", 1, -np.inf, "finite"), ("rgb", 2, np.nan, "finite"),
                                   ("rgb", 0, -1e-20, "negative"), ("dir", None, 0.0, "zero length")):
        bad = good.copy()
        if k is None:
            bad[field][7] = value
        else:
            bad[field][7, k] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_stars: entry 7: .*" + words):
            renderer.set_stars(bad)
    lib_hip = renderer._lib
    assert lib_hip.rpt_set_stars(renderer._h, None, -1) == 1 and lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_stars:")
    assert lib_hip.rpt_set_stars(renderer._h, None, (1 << 22) + 1) == 1
    # every refusal kept the catalogue that was there
    _pass_against_oracle(renderer, lib, _view(scene, camera, W, H, 0), good, "after the refusals")


def test_what_the_launch_refuses(renderer, lib):
    scene = _scene("cubes", "rest")
    camera = sc.CAMERAS["pinhole"]
    W, H = 67, 41
    _setup(renderer, scene, W, H, camera)
    cat, _ = sc.catalogue(camera, W, H, scene.camera_lorentz()[1], -1)
    renderer.set_stars(cat)
    v = _view(scene, camera, W, H, 0)

    def refused(code, words):
        with pytest.raises(RenderError, match=rf"failed \({code}\): rpt_render_stars: .*{words}") as e:
            renderer.render_stars()
        assert e.value.code == code

    # a ray map has no inverse
    renderer.set_raymap(raymap("fisheye", W, H))
    renderer.set_projection("raymap")
    _frames(renderer)
    refused(1, "RPT_PROJECTION_RAYMAP")
    renderer.set_projection("pinhole")
    renderer.set_raymap(None)
    _pass_against_oracle(renderer, lib, v, cat, "after the ray map")
    # a context restricted by rpt_set_rows
    renderer.set_rows(0, 2, False)
    refused(1, "rpt_set_rows")
    renderer.set_rows(0, 1, False)
    _pass_against_oracle(renderer, lib, v, cat, "after rpt_set_rows")
    # no event frame of this view
    renderer.set_orientation(0.1, 0.0, 0.0)
    renderer.render()
    refused(2, "the view has changed")
    renderer.set_orientation(0.0, 0.0, 0.0)
    _pass_against_oracle(renderer, lib, v, cat, "after a stale event frame")
    # a sky matrix that cannot be inverted
    singular = np.eye(4, dtype=np.float32)
    singular[3] = singular[1]
    renderer.set_environment_frame(singular)
    _frames(renderer)
    refused(1, "cannot be inverted")
    renderer.set_environment_frame(scene.camera_lorentz()[1])
    _pass_against_oracle(renderer, lib, v, cat, "after the singular sky matrix")


def test_with_a_sky_image_adaptive_aa_the_overlay_and_async(renderer, lib):
    W, H = 128, 72
    scene = _scene("cubes", "0.9c")
    camera = sc.CAMERAS["pinhole"]
    E = scene.camera_lorentz()[1]
    cat, _ = sc.catalogue(camera, W, H, E, -1)
    v = _view(scene, camera, W, H, 3)
    _setup(renderer, scene, W, H, camera, 3)
    renderer.set_stars(cat)
    _, _, plain, _ = _pass_against_oracle(renderer, lib, v, cat, "the constant background")
    y, x = np.mgrid[0:32, 0:64]
    image = np.ascontiguousarray(np.stack([40 + 3 * x, 30 + 6 * y, 200 - 2 * x], -1).astype(np.uint8))
    renderer.set_environment(image)
    before, _, with_sky, _ = _pass_against_oracle(renderer, lib, v, cat, "over a sky image")
    assert with_sky.tobytes() != plain.tobytes() and renderer.last_variant() != 0
    renderer.set_environment(None)
    renderer.set_adaptive_aa(2, 8)
    _pass_against_oracle(renderer, lib, v, cat, "with adaptive anti-aliasing")
    assert renderer.last_aa_variant() != 0
    renderer.set_adaptive_aa(1, 8)
    # the overlay before and after
    before, records = _frames(renderer)
    renderer.set_overlay(**OUTLINES)
    renderer.render_overlay()
    renderer.render_stars()
    lines_first = renderer.read_framebuffer().copy()
    rgba, n_lines = overlay(before["rgba"], records.reshape(H, W), -1, **OUTLINES)
    want = before.copy()
    want["rgba"] = rgba.reshape(-1, 4)
    want, counts = sc.oracle_pass(lib, v, cat, want, records)
    _same_pixels(lines_first, want, "overlay, then stars")
    assert renderer.last_overlay_pixels() == n_lines > 0 and renderer.last_stars() == counts
    renderer.render()
    renderer.render_stars()
    renderer.render_overlay()
    stars_first = renderer.read_framebuffer().copy()
    want, counts = sc.oracle_pass(lib, v, cat, before, records)
    rgba, n_lines = overlay(want["rgba"], records.reshape(H, W), -1, **OUTLINES)
    want["rgba"] = rgba.reshape(-1, 4)
    _same_pixels(stars_first, want, "stars, then overlay")
    assert renderer.last_stars() == counts
    renderer.set_overlay()
    # async, then rpt_sync
    renderer.render()
    renderer.render_stars()
    blocking = renderer.read_framebuffer().copy()
    renderer.render_async()
    renderer.render_events(async_=True)
    renderer.render_stars(async_=True)
    renderer.sync()
    assert renderer.read_framebuffer().tobytes() == blocking.tobytes() and renderer.last_stars() == counts


def test_render_scene_takes_a_catalogue(lib):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 67, 41
    scene = _scene("cubes", "0.9c")
    cat = stars.random_catalogue(1500, 4, faintest=0.2)
    plain, _ = render_scene(scene, W, H)
    lit, _, records = render_scene(scene, W, H, stars=cat)
    want, counts = sc.oracle_pass(lib, _view(scene, sc.CAMERAS["pinhole"], W, H, 0), cat, plain, records)
    _same_pixels(lit, want, "render_scene(stars=)")
    assert counts[1] > 0
