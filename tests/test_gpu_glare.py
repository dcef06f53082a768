"""Glare on the MI355X (rpt_set_glare): with a layer set on, each of the five splat passes — and the thermal twin of one,
and lit dust with shadows — must give the bytes of tests/native/glare_oracle.c: the pass's own C restatement up to its accumulator, then
rules G2-G6.  All 16 bytes of every pixel and both counts, on the device's own pre-pass framebuffer and records, as the per-pass files
do it.  Then what only glare has: the star pass's mask and the spill onto hit pixels, the clamp of rule G2, the accumulator and the
planes handed over clean, and glare off being the pass as it always was.  Frames are 300 x 70 (two row segments of kernel 1170, the
second partial; 19 x 5 tiles of kernel 1171, the last of each ragged) and 40 x 24 (smaller than the widest layer's support)."""
import math

import numpy as np
import pytest

import ballistics_cases as bc
import dust_cases as dc
import events_oracle as eo
import glare_cases as gl
import particles_cases as pc
import rockets_cases as rc
import segments_cases as gc
import stars_cases as sc
import thermal_cases as tc
from relativitypathtracer_amd import particles, stars
from relativitypathtracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

PASSES = ("stars", "particles", "segments", "ballistics", "rockets")
KIND_OF = {"stars": "stars", "particles": "segments", "segments": "segments", "ballistics": "ballistics", "rockets": "rockets", "dust": "dust"}
CAMERAS = {k: sc.CAMERAS[k] for k in ("pinhole", "sphere")}       # the pinhole and the full-circle panorama (the stage wraps)
MOTIONS = ("rest", "0.9c")
SCENE = "cubes"
FLAGS = 3                                                # shift and beaming: at 0.9c the colours span many more decades yet
PIECES = 16
SOURCES = 300


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.set_glare(None)
    r.close()


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    built = {}

    def get(kind):
        if kind not in built:
            built[kind] = gl.build_library(tmp_path_factory.mktemp("glare_" + kind), kind)
        return built[kind]
    return get


_SCENES = {}


def _scene(name, motion):
    if (name, motion) not in _SCENES:
        _SCENES[(name, motion)] = eo.load_scene(name, motion, -1)
    return _SCENES[(name, motion)]


def _setup(r, scene, W, H, camera, flags=FLAGS, windows="scene"):
    r.set_variant(0)
    r.set_msaa(1)
    r.set_adaptive_aa(1, 8)
    r.set_doppler(bool(flags & 1), bool(flags & 2))
    r.set_environment(None)
    r.set_environment_frame(scene.camera_lorentz()[1])
    r.set_debug_rgb(False)
    r.set_overlay()
    r.set_stars(None)
    r.set_particles(None, [])
    r.set_particle_options()
    r.set_particle_lighting()
    r.set_segments(None)
    r.set_segment_options()
    r.set_ballistics(None)
    r.set_ballistic_options()
    r.set_rockets(None)
    r.set_rocket_options()
    for name in PASSES:
        getattr(r, f"set_{name}_measurement")(False)
    sc.setup_camera(r, camera)
    r.upload_scene(scene)
    r.set_object_windows(scene.windows() if isinstance(windows, str) else windows)
    r.set_readouts(None)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


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


def _thin(records, n=SOURCES):
    """At most n records, evenly taken."""
    if len(records) <= n:
        return np.ascontiguousarray(records)
    return np.ascontiguousarray(records[np.unique(np.linspace(0, len(records) - 1, n).astype(np.int64))])


def _sources(name, scene, camera, objects, records, W, H, rng):
    """A few hundred sources of one pass for one view, colours spread over 1e-2 .. 1e6: the pass's crafted set (in front of surfaces,
    behind them, on the frame's edges, ...) thinned, or 300 random stars."""
    E = scene.camera_lorentz()[1]
    if name == "stars":
        cat, groups = sc.crafted(camera, W, H, E, -1)
        crafted = np.concatenate([cat[groups[k]] for k in ("on pixels", "edges and corners", "seam", "poles")])
        srcs = np.concatenate([stars.random_catalogue(SOURCES - len(crafted), 7), crafted])
    elif name in ("particles", "dust"):
        srcs = _thin(pc.crafted(records, objects, camera, W, H, -1)[0])
    elif name == "segments":
        srcs = _thin(gc.crafted(records, objects, camera, W, H, -1)[0], 40)
    elif name == "ballistics":
        srcs = _thin(bc.crafted(records, objects, camera, W, H, -1)[0])
    else:
        srcs = _thin(rc.crafted(records, objects, camera, W, H, -1)[0])
    srcs = srcs.copy()
    srcs["rgb"] = gl.spread_colours(len(srcs), rng)
    return srcs


def _pass(name, r, lib, scene, camera, objects, srcs, W, H, flags=FLAGS, kelvin=None, lighting=0):
    """(set the sources on the context, render the pass, read its two counts, the plain C pass as gl.glared takes it)"""
    wp, interval, windows = scene.params["white_point"], scene.params["interval"], scene.windows()
    if name == "stars":
        v = sc.view(camera, W, H, scene.camera_lorentz()[1], interval, flags, wp)
        if kelvin is None:
            return (lambda: r.set_stars(srcs)), r.render_stars, r.last_stars, (lambda px, rec: sc.oracle_pass(lib, v, srcs, px, rec))
        xg = tc.x_green32(kelvin)
        return (lambda: r.set_stars(srcs, kelvin)), r.render_stars, r.last_stars, (lambda px, rec: tc.oracle_stars_pass(lib, v, srcs, xg, px, rec))
    v = pc.view(camera, W, H, interval, flags, wp)
    if name == "particles":
        return (lambda: r.set_particles(srcs)), r.render_particles, r.last_particles, (lambda px, rec: pc.oracle_pass(lib, v, objects, srcs, px, rec, windows))
    if name == "dust":
        def on():
            r.set_particles(srcs)
            r.set_particle_lighting(lit=bool(lighting & dc.LIT), shadows=bool(lighting & dc.SHADOWED), ambient=bool(lighting & dc.AMBIENT))
        return on, r.render_particles, r.last_particles, (lambda px, rec: dc.oracle_pass(lib, scene, v, objects, lighting, srcs, px, rec, windows))
    if name == "segments":
        def on():
            r.set_segment_options(pieces=PIECES)
            r.set_segments(srcs)
        return on, r.render_segments, r.last_segments, (lambda px, rec: gc.oracle_pass(lib, v, objects, srcs, PIECES, px, rec, windows))
    if name == "ballistics":
        return (lambda: r.set_ballistics(srcs)), r.render_ballistics, r.last_ballistics, (lambda px, rec: bc.oracle_pass(lib, v, objects, srcs, px, rec))
    return (lambda: r.set_rockets(srcs)), r.render_rockets, r.last_rockets, (lambda px, rec: rc.oracle_pass(lib, v, objects, srcs, px, rec))


def _glared_against_oracle(r, lib, how, layers, W, H, scene, camera, what, star_pass):
    """Fresh frames, the pass the context holds with `layers` on, against the oracle: bytes, counts, the records untouched.
    (before, records, after, counts, S, acc)"""
    _, render, last, plain = how
    r.set_glare(layers)
    before, records = _frames(r)
    render()
    after = r.read_framebuffer().copy()
    want, counts, S, acc = gl.glared(lib, plain, W, H, layers, before, records, scene.params["white_point"], gl.wraps(camera), star_pass)
    _same_pixels(after, want, what)
    assert last()[:2] == counts, f"{what}: the pass counted {last()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts, S, acc


@pytest.mark.parametrize("camera_name", list(CAMERAS))
@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("name", PASSES)
def test_every_pass_with_glare_on_equals_the_c_oracle(renderer, libs, name, motion, camera_name):
    """Both sizes, the three layer sets: one narrow layer, three with the widest there is, and two that leave the core nothing."""
    lib = libs(KIND_OF[name])
    camera, scene = CAMERAS[camera_name], _scene(SCENE, motion)
    objects = pc.scene_objects(scene, camera)
    rng = np.random.default_rng(31)
    srcs = None
    for W, H in gl.SIZES:
        _setup(renderer, scene, W, H, camera)
        _, records = _frames(renderer)
        if srcs is None:                                 # (from the larger frame's records; the smaller frame sees the same set)
            srcs = _sources(name, scene, camera, objects, records, W, H, rng)
        assert 20 <= len(srcs) <= 400
        how = _pass(name, renderer, lib, scene, camera, objects, srcs, W, H)
        how[0]()
        for label, layers in gl.LAYER_SETS.items():
            what = f"{name} {motion} {camera_name} {W}x{H} {label}"
            before, _, after, counts, S, acc = _glared_against_oracle(renderer, lib, how, layers, W, H, scene, camera, what, name == "stars")
            print(what, counts, int((acc != 0).any(axis=2).sum()), int((S != 0).any(axis=2).sum()))
            assert counts[0] > 0, what
            if (W, H) == gl.SIZES[0]:                    # (at 0.9c the smaller frame of a pass can be left with sums that are all zero)
                assert counts[1] > 0 and acc.any(), what
            if acc.any():
                assert (S != 0).any(axis=2).sum() > (acc != 0).any(axis=2).sum(), f"{what}: the stage lit no pixel the splat had not"
            assert np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"]) and np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3])
    renderer.set_glare(None)


def test_the_thermal_twin_and_dust_with_shadows(renderer, libs):
    W, H = gl.SIZES[0]
    rng = np.random.default_rng(32)
    camera, scene = CAMERAS["sphere"], _scene(SCENE, "0.9c")
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera)
    _, records = _frames(renderer)
    cat = _sources("stars", scene, camera, objects, records, W, H, rng)
    kelvin = tc.temperatures(len(cat), rng)
    how = _pass("stars", renderer, libs("stars"), scene, camera, objects, cat, W, H, kelvin=kelvin)
    how[0]()
    _, _, _, counts, _, _ = _glared_against_oracle(renderer, libs("stars"), how, gl.LAYER_SETS["three"], W, H, scene, camera, "thermal stars", True)
    assert counts[0] > 0 and counts[1] > 0
    renderer.set_star_temperatures(None)

    camera, scene = CAMERAS["pinhole"], dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, flags=0, windows=None)
    ps = dc.cloud("shadows", scene, 400).copy()
    ps["rgb"] = np.clip(gl.spread_colours(len(ps), rng), None, 1e3)      # (albedos: the lamp's colour multiplies them)
    lighting = dc.LIT | dc.SHADOWED
    how = _pass("dust", renderer, libs("dust"), scene, camera, objects, ps, W, H, flags=0, lighting=lighting)
    how[0]()
    renderer.set_glare(gl.LAYER_SETS["three"])
    before, records = _frames(renderer)
    renderer.render_particles()
    after = renderer.read_framebuffer().copy()
    v = pc.view(camera, W, H, -1, 0, scene.params["white_point"])
    plain = lambda px, rec: dc.oracle_pass(libs("dust"), scene, v, objects, lighting, ps, px, rec, None)      # noqa: E731
    want, counts, _, _ = gl.glared(libs("dust"), plain, W, H, gl.LAYER_SETS["three"], before, records, scene.params["white_point"], False)
    _same_pixels(after, want, "dust with shadows")
    assert renderer.last_particles() == counts and counts[0] > 0 and counts[1] > 0
    pairs = renderer.last_particle_lighting()
    assert pairs[0] > 0 and pairs[1] > 0, pairs            # (some pairs lit, some shadowed: the shadowed kernel ran)
    renderer.set_particle_lighting()
    renderer.set_glare(None)


def _one_star(scene, camera, W, H, x, y, rgb, copies=1):
    cat = np.zeros(copies, dtype=stars.STAR_DTYPE)
    cat["dir"] = sc.sky_direction(camera, scene.camera_lorentz()[1], -1, sc.pixel_direction(camera, W, H, float(x), float(y)))
    cat["rgb"] = rgb
    return cat


def test_the_star_mask_and_the_spill(renderer, libs):
    """A star at the clamp on a pixel whose neighbours are all hits is behind the object: no source, no glare, no byte.  The same star
    two pixels outside the silhouette glares over it: hit pixels change."""
    lib = libs("stars")
    W, H = gl.SIZES[0]
    camera, scene = CAMERAS["pinhole"], _scene(SCENE, "rest")
    _setup(renderer, scene, W, H, camera, flags=0)
    _, records = _frames(renderer)
    hit = records["object"].reshape(H, W) >= 0
    inner = hit.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= np.roll(np.roll(hit, dy, 0), dx, 1)
    inner[[0, -1], :] = False
    inner[:, [0, -1]] = False
    ys, xs = np.nonzero(inner)
    assert len(ys) > 0
    layers = [(0.5, 2.5)]
    objects = pc.scene_objects(scene, camera)
    cat = _one_star(scene, camera, W, H, xs[0], ys[0], 65536.0)
    how = _pass("stars", renderer, lib, scene, camera, objects, cat, W, H, flags=0)
    how[0]()
    before, _, after, counts, S, acc = _glared_against_oracle(renderer, lib, how, layers, W, H, scene, camera, "behind", True)
    assert counts == (1, 0) and acc.any() and not S.any()
    assert after.tobytes() == before.tobytes()
    # a miss pixel with a miss to its right and a hit two to its right, clear of the frame's edge
    spot = ~hit[:, :-2] & ~hit[:, 1:-1] & hit[:, 2:]
    spot[:8, :] = False
    spot[-8:, :] = False
    spot[:, :8] = False
    ys, xs = np.nonzero(spot)
    assert len(ys) > 0
    cat = _one_star(scene, camera, W, H, xs[0], ys[0], 65536.0)
    how = _pass("stars", renderer, lib, scene, camera, objects, cat, W, H, flags=0)
    how[0]()
    before, _, after, counts, S, _ = _glared_against_oracle(renderer, lib, how, layers, W, H, scene, camera, "spill", True)
    moved = (after["rgba"] != before["rgba"]).any(axis=1).reshape(H, W)
    print(counts, int(moved.sum()), int((moved & hit).sum()))
    assert counts[0] == 1 and counts[1] == moved.sum() and (moved & hit).any() and (moved & ~hit).any()
    renderer.set_glare(None)


def test_the_clamp_of_the_source(renderer, libs):
    """Twenty stars at the per-tap clamp on one pixel sum to 20 x 2^40 > 2^44: the stage takes 2^44."""
    lib = libs("stars")
    W, H = gl.SIZES[1]
    camera, scene = CAMERAS["pinhole"], _scene(SCENE, "rest")
    _setup(renderer, scene, W, H, camera, flags=0)
    _, records = _frames(renderer)
    miss = records["object"].reshape(H, W) < 0
    ys, xs = np.nonzero(miss)
    assert len(ys) > 0
    k = len(ys) // 2
    cat = _one_star(scene, camera, W, H, xs[k], ys[k], 1e30, copies=20)
    how = _pass("stars", renderer, lib, scene, camera, pc.scene_objects(scene, camera), cat, W, H, flags=0)
    how[0]()
    for label, layers in gl.LAYER_SETS.items():
        _, _, _, counts, S, acc = _glared_against_oracle(renderer, lib, how, layers, W, H, scene, camera, "clamp " + label, True)
        assert int(acc.max()) == 20 << 40 and counts == (20, counts[1]) and counts[1] > 0
        assert int(S.sum(axis=(0, 1)).max()) <= 1 << 44
    renderer.set_glare(None)


def test_a_clean_hand_over(renderer, libs):
    """A glared pass, then the same pass with glare unset on a fresh colour frame: the plain oracle's bytes — the accumulator was left
    all zero and the off path is the pass's own.  Then a smaller frame, the larger one again and the smaller one, glared: the planes follow."""
    camera, scene = CAMERAS["sphere"], _scene(SCENE, "0.9c")
    objects = pc.scene_objects(scene, camera)
    rng = np.random.default_rng(33)
    for name in ("stars", "rockets"):
        lib = libs(KIND_OF[name])
        srcs = None
        for W, H in (gl.SIZES[0], gl.SIZES[1], gl.SIZES[0], gl.SIZES[1]):
            _setup(renderer, scene, W, H, camera)
            _, records = _frames(renderer)
            if srcs is None:
                srcs = _sources(name, scene, camera, objects, records, W, H, rng)
            how = _pass(name, renderer, lib, scene, camera, objects, srcs, W, H)
            how[0]()
            _glared_against_oracle(renderer, lib, how, gl.LAYER_SETS["three"], W, H, scene, camera, f"{name} {W}x{H} glared", name == "stars")
            renderer.set_glare(None)
            before, records = _frames(renderer)
            how[1]()
            want, counts = how[3](before, records)[:2]
            _same_pixels(renderer.read_framebuffer(), want, f"{name} {W}x{H} plain after glared")
            assert how[2]()[:2] == counts


def test_off_is_the_pass_as_it_was(libs):
    """A context that never heard of glare and one that set it and unset it give the plain oracle's frame; and a timed glared pass
    reports two finite, non-negative times."""
    W, H = gl.SIZES[0]
    camera, scene = CAMERAS["pinhole"], _scene(SCENE, "0.9c")
    objects = pc.scene_objects(scene, camera)
    rng = np.random.default_rng(34)
    frames = []
    for unset in (False, True):
        r = Renderer(0)
        try:
            _setup(r, scene, W, H, camera)
            _, records = _frames(r)
            if not frames:
                srcs = {name: _sources(name, scene, camera, objects, records, W, H, rng) for name in ("stars", "particles")}
            if unset:
                r.set_glare(gl.LAYER_SETS["narrow"])
                r.set_glare([])
            want, _ = _frames(r)
            for name in ("stars", "particles"):
                lib = libs(KIND_OF[name])
                how = _pass(name, r, lib, scene, camera, objects, srcs[name], W, H)
                how[0]()
                how[1]()
                want, counts = how[3](want, records)[:2]
                assert how[2]()[:2] == counts
            _same_pixels(r.read_framebuffer(), want, f"glare {'set and unset' if unset else 'never set'}")
            frames.append(r.read_framebuffer().tobytes())
            if unset:
                r.set_stars_measurement(True)
                r.set_glare(gl.LAYER_SETS["three"])
                _frames(r)
                r.render_stars()
                ms = r.last_stars_ms()
                print(ms)
                assert len(ms) == 2 and all(math.isfinite(m) and m >= 0.0 for m in ms), ms
        finally:
            r.close()
    assert frames[0] == frames[1]
