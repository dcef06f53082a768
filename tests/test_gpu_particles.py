"""rpt_render_particles on the MI355X: the device's own pre-pass framebuffer and records go through
tests/native/particles_oracle.c, the C restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and both
counts of rpt_last_particles, and leave the record buffer as it was.  Feeding the reference what the device rendered isolates kernels
1130 and 1131 from every other.  Scenes, cameras, sizes and particle sets are those of tests/particles_cases.py, built from the device's
own records; their non-vacuity is asserted here on those records and in tests/test_particles_model.py on CPU frames.  Frames are
128 x 72 at most, sets 4096 particles at most."""
import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
from relativitypathtracer_amd import particles
from relativitypathtracer_amd.events import overlay, readout
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
    return pc.build_library(tmp_path_factory.mktemp("particles"))


@pytest.fixture(scope="module")
def stars_lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("particles_stars"))


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
    r.set_particle_options()
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
    return pc.view(camera, W, H, scene.params["interval"], flags, scene.params["white_point"], **options)


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


def _pass_against_oracle(r, lib, v, objects, ps, what, passes=1, windows=None):
    """Colour frame, event frame, the pass `passes` times with the set the context HOLDS, against the oracle applied as often."""
    before, records = _frames(r)
    for _ in range(passes):
        r.render_particles()
    after = r.read_framebuffer().copy()
    want, counts = before, None
    for _ in range(passes):
        want, counts = pc.oracle_pass(lib, v, objects, ps, want, records, windows)
    _same_pixels(after, want, what)
    assert r.last_particles() == counts, f"{what}: rpt_last_particles {r.last_particles()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(pc.CAMERAS))
@pytest.mark.parametrize("motion", pc.MOTIONS)
@pytest.mark.parametrize("scene_name", pc.SCENES)
def test_the_pass_equals_the_c_oracle(renderer, lib, scene_name, motion, name, size):
    """Light delay on and off, every Doppler setting, the inverse square on and off, the depth bias 0 and 1e-3 of the largest dist; the
    set is tests/particles_cases.py's crafted one, built from the device's own records of the view."""
    W, H = size
    camera = pc.CAMERAS[name]
    for interval in pc.INTERVALS:
        scene = _scene(scene_name, motion, interval)
        objects = pc.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera)
        _, records = _frames(renderer)
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        ps, groups, bias = pc.crafted(records, objects, camera, W, H, interval)
        pc.check_shows_something(lib, records, objects, camera, W, H, interval, ps, groups, bias, what)
        renderer.set_particles(ps)
        for flags in pc.FLAGS:
            renderer.set_doppler(bool(flags & 1), bool(flags & 2))
            seen = {}
            for inverse_square in (False, True):
                for depth_bias in (0.0, bias):
                    renderer.set_particle_options(inverse_square=inverse_square, depth_bias=depth_bias)
                    v = _view(scene, camera, W, H, flags, inverse_square=inverse_square, depth_bias=depth_bias)
                    case = f"{what} flags {flags} inverse square {inverse_square} bias {depth_bias:g}"
                    before, records_now, after, counts = _pass_against_oracle(renderer, lib, v, objects, ps, case)
                    assert records_now.tobytes() == records.tobytes(), f"{case}: the event frame is not the one the set was built from"
                    assert 0 < counts[0] < len(ps), case
                    seen[(inverse_square, depth_bias)] = counts[0]
                    # the untouched bytes
                    assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]) and np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"])
                    assert np.array_equal(after["unspecified"], before["unspecified"])
                    assert int((after["rgba"] != before["rgba"]).any(axis=1).sum()) == counts[1]
                    if not flags & 1 and not inverse_square:
                        assert counts[1] > 0, case
            assert seen[(False, bias)] >= seen[(False, 0.0)] and seen[(True, 0.0)] == seen[(False, 0.0)], f"{what} flags {flags}: {seen}"


def test_particles_riding_a_body_of_three_legs_show_on_the_leg_whose_window_holds_them(renderer, lib):
    W, H = 128, 72
    wl, scene, ps = pc.turnaround()
    camera = pc.CAMERAS["pinhole"]
    objects = pc.scene_objects(scene, camera)
    windows = scene.windows()
    _setup(renderer, scene, W, H, camera, 3)
    renderer.set_particles(ps)
    v = _view(scene, camera, W, H, 3)
    _, records, _, windowed = _pass_against_oracle(renderer, lib, v, objects, ps, "three legs, their windows", windows=windows)
    held = pc.oracle_place(lib, v, objects, ps, windows)
    free = pc.oracle_place(lib, v, objects, ps)
    shown = [bool(held["visible"][ps["object"] == j].any()) for j in range(3)]
    assert any(shown) and not all(shown) and (free["visible"] & ~held["visible"]).any(), shown
    # every window at its default: the windowed kernels' frame, and the pass, are the un-windowed ones
    default = np.tile(np.array([-np.inf, np.inf], dtype=np.float32), (len(windows), 1))
    renderer.set_object_windows(default)
    _, _, with_defaults, open_counts = _pass_against_oracle(renderer, lib, v, objects, ps, "every window at its default", windows=default)
    renderer.set_object_windows(None)
    _, _, without, plain_counts = _pass_against_oracle(renderer, lib, v, objects, ps, "no windows")
    assert with_defaults.tobytes() == without.tobytes() and open_counts == plain_counts
    assert 0 < windowed[0] < plain_counts[0]


def test_the_sums_do_not_depend_on_the_order(renderer, lib):
    """4096 lamps of a lattice riding a moving cube crowd into a few hundred pixels; reversed and shuffled sets give the same bytes."""
    W, H = 128, 72
    scene = _scene("cubes", "rest")
    camera = pc.CAMERAS["pinhole"]
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, 2)
    _, records = _frames(renderer)
    hit = records[records["object"] >= 0]
    o = int(hit["object"][0])
    centre = hit["event"][hit["object"] == o][0, 1:4].astype(np.float64)
    ps = particles.lattice(o, centre - 0.5, centre + 0.5, 16, (0.3, 0.2, 0.1))
    assert len(ps) == 4096
    renderer.set_particle_options(inverse_square=True)
    v = _view(scene, camera, W, H, 2, inverse_square=True)
    renderer.set_particles(ps)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, objects, ps, "the set as given")
    assert counts[0] > 1000 and 0 < counts[1] < counts[0], counts
    renderer.set_particles(ps[::-1].copy())
    _, _, backward, counts_reversed = _pass_against_oracle(renderer, lib, v, objects, ps[::-1].copy(), "the set reversed")
    assert forward.tobytes() == backward.tobytes() and counts == counts_reversed
    shuffled = ps[np.random.default_rng(2).permutation(len(ps))]
    renderer.set_particles(shuffled)
    _, _, third, _ = _pass_against_oracle(renderer, lib, v, objects, shuffled, "the set shuffled")
    assert third.tobytes() == forward.tobytes()


def _case(renderer, W=128, H=72, flags=3, motion="0.9c", name="pinhole", scene_name="cubes"):
    """One parity case set up on the renderer: (scene, camera, objects, set, bias)."""
    scene = _scene(scene_name, motion)
    camera = pc.CAMERAS[name]
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, flags)
    _, records = _frames(renderer)
    ps, _, bias = pc.crafted(records, objects, camera, W, H, -1)
    return scene, camera, objects, ps, bias


def test_the_accumulator_is_clean_after_every_pass_and_shared_with_the_stars(renderer, lib, stars_lib):
    scene, camera, objects, ps, _ = _case(renderer)
    renderer.set_particles(ps)
    v = _view(scene, camera, 128, 72, 3)
    _, _, first, _ = _pass_against_oracle(renderer, lib, v, objects, ps, "first frame")
    _, _, second, _ = _pass_against_oracle(renderer, lib, v, objects, ps, "second frame")
    assert first.tobytes() == second.tobytes()
    _pass_against_oracle(renderer, lib, v, objects, ps, "the pass twice on one frame", passes=2)
    renderer.set_scene_params(scene, 67, 41)            # another size (a smaller frame in the same accumulator), and back
    _, records = _frames(renderer)
    small, _, _ = pc.crafted(records, objects, camera, 67, 41, -1)
    renderer.set_particles(small)
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 3), objects, small, "67 x 41 in between")
    renderer.set_scene_params(scene, 128, 72)
    renderer.set_particles(ps)
    _, _, again, _ = _pass_against_oracle(renderer, lib, v, objects, ps, "back at 128 x 72")
    assert again.tobytes() == first.tobytes()
    # a star pass before and after on the same context: each pass finds the accumulator clean and leaves it so
    E = scene.camera_lorentz()[1]
    cat, _ = sc.catalogue(camera, 128, 72, E, -1)
    sv = sc.view(camera, 128, 72, E, -1, 3, scene.params["white_point"])
    renderer.set_stars(cat)
    before, records = _frames(renderer)
    renderer.render_stars()
    renderer.render_particles()
    renderer.render_stars()
    got = renderer.read_framebuffer().copy()
    want, star_counts = sc.oracle_pass(stars_lib, sv, cat, before, records)
    want, particle_counts = pc.oracle_pass(lib, v, objects, ps, want, records)
    want, star_counts_again = sc.oracle_pass(stars_lib, sv, cat, want, records)
    _same_pixels(got, want, "stars, particles, stars")
    assert renderer.last_stars() == star_counts_again and renderer.last_particles() == particle_counts and star_counts[0] == star_counts_again[0]
    renderer.set_stars(None)
    fresh = Renderer(0)                                 # a larger frame than the context has had: a new accumulator, first made by this pass
    try:
        _setup(fresh, scene, 67, 41, camera, 3)
        fresh.set_particles(small)
        _pass_against_oracle(fresh, lib, _view(scene, camera, 67, 41, 3), objects, small, "a fresh context at 67 x 41")
        fresh.set_scene_params(scene, 128, 72)
        fresh.set_particles(ps)
        _, _, grown, _ = _pass_against_oracle(fresh, lib, v, objects, ps, "grown to 128 x 72")
        assert grown.tobytes() == first.tobytes()
    finally:
        fresh.close()


def test_off_means_off(renderer, lib):
    fresh = Renderer(0)
    try:
        fresh.render_particles()                        # no set: nothing is checked, not even that a scene is there
        assert fresh.last_particles() == (0, 0)
    finally:
        fresh.close()
    scene, camera, objects, ps, _ = _case(renderer, 67, 41, 0, "rest")
    renderer.set_particles(None)
    before, _ = _frames(renderer)
    variant = renderer.last_variant()
    renderer.render_particles()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_variant() == variant and renderer.last_particles() == (0, 0)
    renderer.set_particles(ps)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, ps, "a set first")
    assert counts[1] > 0
    renderer.set_particles(None)
    before, _ = _frames(renderer)
    renderer.render_particles()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_particles() == (0, 0)
    renderer.set_particles(np.zeros(0, dtype=particles.PARTICLE_DTYPE))
    renderer.render_particles()
    assert renderer.read_framebuffer().tobytes() == before.tobytes()


def test_what_the_setters_refuse(renderer, lib):
    scene, camera, objects, good, bias = _case(renderer, 67, 41, 0, "rest")
    renderer.set_particles(good)
    renderer.set_particle_options(inverse_square=True, depth_bias=bias)
    for field, k, value, words in (("pos", 0, np.nan, "finite"), ("pos", 2, np.inf, "finite"), ("rgb", 1, -np.inf, "finite"), ("rgb", 2, np.nan, "finite"),
                                   ("rgb", 0, -1e-20, "negative"), ("object", None, -1, "object is negative")):
        bad = good.copy()
        if k is None:
            bad[field][7] = value
        else:
            bad[field][7, k] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_particles: entry 7: .*" + words):
            renderer.set_particles(bad)
    lib_hip = renderer._lib
    assert lib_hip.rpt_set_particles(renderer._h, None, -1) == 1 and lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_particles:")
    assert lib_hip.rpt_set_particles(renderer._h, None, (1 << 22) + 1) == 1
    for flags, depth_bias in ((2, 0.0), (-1, 0.0), (0, -1e-6), (1, float("nan")), (0, float("inf"))):
        assert lib_hip.rpt_set_particle_options(renderer._h, flags, depth_bias) == 1
        assert lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_particle_options:")
    # every refusal kept the set and the options that were there
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0, inverse_square=True, depth_bias=bias), objects, good, "after the refusals")


def test_what_the_launch_refuses(renderer, lib):
    W, H = 67, 41
    scene, camera, objects, ps, _ = _case(renderer, W, H, 0, "rest")
    renderer.set_particles(ps)
    v = _view(scene, camera, W, H, 0)

    def refused(code, words):
        with pytest.raises(RenderError, match=rf"failed \({code}\): rpt_render_particles: .*{words}") as e:
            renderer.render_particles()
        assert e.value.code == code

    # a ray map has no inverse
    renderer.set_raymap(raymap("fisheye", W, H))
    renderer.set_projection("raymap")
    _frames(renderer)
    refused(1, "RPT_PROJECTION_RAYMAP")
    renderer.set_projection("pinhole")
    renderer.set_raymap(None)
    _pass_against_oracle(renderer, lib, v, objects, ps, "after the ray map")
    # an interval the cone has no closed form for
    two = eo.load_scene("cubes", "rest", 2)
    renderer.set_scene_params(two, W, H)
    _frames(renderer)
    refused(1, "interval is 2")
    renderer.set_scene_params(scene, W, H)
    _pass_against_oracle(renderer, lib, v, objects, ps, "after interval 2")
    # a set that names object index object_count: refused at the launch, whatever came last, the set or the objects
    n = len(objects)
    beyond = ps.copy()
    beyond["object"][5] = n
    renderer.set_particles(beyond)
    _frames(renderer)
    refused(1, f"names object {n}, the Object\\[\\] holds {n}")
    renderer.set_particles(ps)
    _pass_against_oracle(renderer, lib, v, objects, ps, "after the index beyond Object[]")
    last = ps.copy()
    last["object"][:] = n - 1
    renderer.set_particles(last)
    _pass_against_oracle(renderer, lib, v, objects, last, "every particle on the last object")
    renderer.set_objects(objects[:n - 1])
    _frames(renderer)
    refused(1, f"names object {n - 1}, the Object\\[\\] holds {n - 1}")
    renderer.upload_scene(scene)
    renderer.set_particles(ps)
    _pass_against_oracle(renderer, lib, v, objects, ps, "after fewer objects")
    # a context restricted by rpt_set_rows
    renderer.set_rows(0, 2, False)
    refused(1, "rpt_set_rows")
    renderer.set_rows(0, 1, False)
    _pass_against_oracle(renderer, lib, v, objects, ps, "after rpt_set_rows")
    # no event frame of this view
    renderer.set_orientation(0.1, 0.0, 0.0)
    renderer.render()
    refused(2, "the view has changed")
    renderer.set_orientation(0.0, 0.0, 0.0)
    _pass_against_oracle(renderer, lib, v, objects, ps, "after a stale event frame")


def test_with_a_sky_image_adaptive_aa_the_overlay_the_readouts_and_async(renderer, lib):
    W, H = 128, 72
    scene, camera, objects, ps, bias = _case(renderer, W, H, 3)
    renderer.set_particles(ps)
    renderer.set_particle_options(depth_bias=bias)
    v = _view(scene, camera, W, H, 3, depth_bias=bias)
    _, _, plain, _ = _pass_against_oracle(renderer, lib, v, objects, ps, "the constant background")
    y, x = np.mgrid[0:32, 0:64]
    image = np.ascontiguousarray(np.stack([40 + 3 * x, 30 + 6 * y, 200 - 2 * x], -1).astype(np.uint8))
    renderer.set_environment(image)
    _, _, with_sky, _ = _pass_against_oracle(renderer, lib, v, objects, ps, "over a sky image")
    assert with_sky.tobytes() != plain.tobytes() and renderer.last_variant() != 0
    renderer.set_environment(None)
    renderer.set_adaptive_aa(2, 8)
    _pass_against_oracle(renderer, lib, v, objects, ps, "with adaptive anti-aliasing")
    assert renderer.last_aa_variant() != 0
    renderer.set_adaptive_aa(1, 8)
    # the overlay and the readouts before and after
    displays = [dict(rate=1.0, offset=0.0, digits=3, decimals=1)] * len(objects)
    before, records = _frames(renderer)
    renderer.set_overlay(**OUTLINES)
    renderer.set_readouts(displays)
    renderer.render_overlay()
    renderer.render_readouts()
    renderer.render_particles()
    layers_first = renderer.read_framebuffer().copy()
    rgba, n_lines = overlay(before["rgba"], records.reshape(H, W), -1, **OUTLINES)
    rgba, n_digits = readout(rgba.reshape(-1, 4), records.reshape(H, W), displays)
    want = before.copy()
    want["rgba"] = rgba.reshape(-1, 4)
    want, counts = pc.oracle_pass(lib, v, objects, ps, want, records)
    _same_pixels(layers_first, want, "overlay, readouts, then particles")
    assert renderer.last_overlay_pixels() == n_lines > 0 and renderer.last_readout_pixels() == n_digits and renderer.last_particles() == counts
    renderer.render()
    renderer.render_particles()
    renderer.render_overlay()
    renderer.render_readouts()
    particles_first = renderer.read_framebuffer().copy()
    want, counts = pc.oracle_pass(lib, v, objects, ps, before, records)
    rgba, _ = overlay(want["rgba"], records.reshape(H, W), -1, **OUTLINES)
    rgba, _ = readout(rgba.reshape(-1, 4), records.reshape(H, W), displays)
    want["rgba"] = rgba.reshape(-1, 4)
    _same_pixels(particles_first, want, "particles, then overlay and readouts")
    assert renderer.last_particles() == counts
    renderer.set_overlay()
    renderer.set_readouts(None)
    # async, then rpt_sync
    renderer.render()
    renderer.render_particles()
    blocking = renderer.read_framebuffer().copy()
    renderer.render_async()
    renderer.render_events(async_=True)
    renderer.render_particles(async_=True)
    renderer.sync()
    assert renderer.read_framebuffer().tobytes() == blocking.tobytes() and renderer.last_particles() == counts


def test_render_scene_takes_particles(lib):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 67, 41
    scene = _scene("cubes", "0.9c")
    camera = pc.CAMERAS["pinhole"]
    objects = pc.scene_objects(scene, camera)
    plain, _, records = render_scene(scene, W, H, events=True)
    ps, _, bias = pc.crafted(records.reshape(-1), objects, camera, W, H, -1)
    lit, _, records_again = render_scene(scene, W, H, particles=ps, particle_options=dict(inverse_square=True, depth_bias=bias))
    assert records_again.tobytes() == records.tobytes()
    want, counts = pc.oracle_pass(lib, _view(scene, camera, W, H, 0, inverse_square=True, depth_bias=bias), objects, ps, plain, records)
    _same_pixels(lit, want, "render_scene(particles=)")
    assert counts[1] > 0
