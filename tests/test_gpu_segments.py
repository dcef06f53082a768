"""rpt_render_segments on the MI355X: the device's own pre-pass framebuffer and records go through
tests/native/segments_oracle.c, the C restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and both
counts of rpt_last_segments, and leave the record buffer as it was.  Feeding the reference what the device rendered isolates kernels
1140 and 1131 from every other.  Scenes, cameras, sizes and rod sets are those of tests/segments_cases.py, built from the device's own
records; their non-vacuity is asserted here on those records and in tests/test_segments_model.py on CPU frames.  Frames are 128 x 72 at
most, sets 512 rods at most."""
import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import segments_cases as sg
import stars_cases as sc
from relativitypathtracer_amd import _ffi, segments
from relativitypathtracer_amd.events import overlay, readout
from relativitypathtracer_amd.renderer import RenderError, Renderer, raymap

pytestmark = pytest.mark.gpu

OUTLINES = dict(outlines=True, outline_rgba=(255, 255, 255, 200), clock_step=0.5, clock_rgba=(0, 255, 255, 160))
LOOP_ARM = 1141         # rpt_set_variant in librpt_hip_diag.so: the segment splat as a loop per lane


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sg.build_library(tmp_path_factory.mktemp("segments"))


@pytest.fixture(scope="module")
def stars_lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("segments_stars"))


@pytest.fixture(scope="module")
def particles_lib(tmp_path_factory):
    return pc.build_library(tmp_path_factory.mktemp("segments_particles"))


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
    r.set_segments(None)
    r.set_segment_options()
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
    return sg.view(camera, W, H, scene.params["interval"], flags, scene.params["white_point"], **options)


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


def _pass_against_oracle(r, lib, v, objects, segs, pieces, what, passes=1, windows=None, frames=None):
    """Colour frame, event frame, the pass `passes` times with the set and the pieces the context HOLDS, against the oracle applied as
    often.  frames: (framebuffer, records) of the view as it stands, where the caller has read them already (the colour frame is then
    rendered anew, and must give the same bytes: nothing between two frames of one view is random)."""
    if frames is None:
        before, records = _frames(r)
    else:
        before, records = frames
        r.render()
    for _ in range(passes):
        r.render_segments()
    after = r.read_framebuffer().copy()
    want, counts = before, None
    for _ in range(passes):
        want, counts = sg.oracle_pass(lib, v, objects, segs, pieces, want, records, windows)
    _same_pixels(after, want, what)
    assert r.last_segments() == counts, f"{what}: rpt_last_segments {r.last_segments()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


@pytest.mark.parametrize("size", sg.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(sg.CAMERAS))
@pytest.mark.parametrize("motion", sg.MOTIONS)
@pytest.mark.parametrize("scene_name", sg.SCENES)
def test_the_pass_equals_the_c_oracle(renderer, lib, scene_name, motion, name, size):
    """Light delay on and off, every Doppler setting, the inverse square on and off, the depth bias 0 and 1e-3 of the largest dist,
    pieces 1, 16 and 64; the set is tests/segments_cases.py's crafted one, built from the device's own records of the view: rods on
    surfaces and the same 1 % nearer and farther, across a silhouette, through the pinhole's plane, one that ends next to it, across
    the seam, over a pole, of no length, seen end-on, of colour 1e30, 64 on one pixel, leaving the frame, and a rod_lattice."""
    W, H = size
    camera = sg.CAMERAS[name]
    for interval in sg.INTERVALS:
        scene = _scene(scene_name, motion, interval)
        objects = sg.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera)
        frames = _frames(renderer)
        records = frames[1]
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        segs, groups, bias = sg.crafted(records, objects, camera, W, H, interval)
        renderer.set_segments(segs)
        for pieces in sg.PIECES:
            sg.check_shows_something(lib, records, objects, camera, W, H, interval, segs, groups, bias, pieces, f"{what} pieces {pieces}")
            for flags in sg.FLAGS:
                renderer.set_doppler(bool(flags & 1), bool(flags & 2))
                frames = _frames(renderer)
                assert frames[1].tobytes() == records.tobytes(), f"{what}: the event frame is not the one the set was built from"
                drawn = {}
                for inverse_square in (False, True):
                    for depth_bias in (0.0, bias):
                        renderer.set_segment_options(inverse_square=inverse_square, depth_bias=depth_bias, pieces=pieces)
                        v = _view(scene, camera, W, H, flags, inverse_square=inverse_square, depth_bias=depth_bias)
                        case = f"{what} pieces {pieces} flags {flags} inverse square {inverse_square} bias {depth_bias:g}"
                        before, _, after, counts = _pass_against_oracle(renderer, lib, v, objects, segs, pieces, case, frames=frames)
                        assert 0 < counts[0] < len(segs) * pieces, case
                        drawn[(inverse_square, depth_bias)] = counts[0]
                        # the untouched bytes
                        assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]) and np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"])
                        assert np.array_equal(after["unspecified"], before["unspecified"])
                        assert int((after["rgba"] != before["rgba"]).any(axis=1).sum()) == counts[1]
                        if not flags & 1 and not inverse_square:
                            assert counts[1] > 0, case
                assert drawn[(False, bias)] >= drawn[(False, 0.0)] and drawn[(True, 0.0)] == drawn[(False, 0.0)], f"{what} flags {flags}: {drawn}"
            renderer.set_doppler(False, False)


def test_box_edges_riding_a_body_of_three_legs_show_on_the_leg_whose_window_holds_them(renderer, lib):
    W, H = 128, 72
    wl, scene, segs = sg.turnaround()
    camera = sg.CAMERAS["pinhole"]
    objects = sg.scene_objects(scene, camera)
    windows = scene.windows()
    _setup(renderer, scene, W, H, camera, 3)
    renderer.set_segments(segs)
    v = _view(scene, camera, W, H, 3)
    for pieces in sg.PIECES:
        renderer.set_segment_options(pieces=pieces)
        renderer.set_object_windows(windows)
        _, _, _, windowed = _pass_against_oracle(renderer, lib, v, objects, segs, pieces, f"three legs, their windows, pieces {pieces}", windows=windows)
        held = sg.oracle_pieces(lib, v, objects, segs, pieces, windows)["placed"]
        free = sg.oracle_pieces(lib, v, objects, segs, pieces)["placed"]
        assert held.any() and (free & ~held).any()
        # every window at its default: the windowed kernels' frame, and the pass, are the un-windowed ones
        default = np.tile(np.array([-np.inf, np.inf], dtype=np.float32), (len(windows), 1))
        renderer.set_object_windows(default)
        _, _, with_defaults, open_counts = _pass_against_oracle(renderer, lib, v, objects, segs, pieces, "every window at its default", windows=default)
        renderer.set_object_windows(None)
        _, _, without, plain_counts = _pass_against_oracle(renderer, lib, v, objects, segs, pieces, "no windows")
        assert with_defaults.tobytes() == without.tobytes() and open_counts == plain_counts
        assert 0 < windowed[0] < plain_counts[0]


def _case(renderer, W=128, H=72, flags=3, motion="0.9c", name="pinhole", scene_name="cubes"):
    """One parity case set up on the renderer: (scene, camera, objects, set, bias)."""
    scene = _scene(scene_name, motion)
    camera = sg.CAMERAS[name]
    objects = sg.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, flags)
    _, records = _frames(renderer)
    segs, _, bias = sg.crafted(records, objects, camera, W, H, -1)
    return scene, camera, objects, segs, bias


def test_the_sums_do_not_depend_on_the_order(renderer, lib):
    scene, camera, objects, segs, _ = _case(renderer, flags=2, motion="rest")
    renderer.set_segment_options(inverse_square=True, pieces=16)
    v = _view(scene, camera, 128, 72, 2, inverse_square=True)
    renderer.set_segments(segs)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, objects, segs, 16, "the set as given")
    assert counts[0] > 500 and counts[1] > 0, counts
    renderer.set_segments(segs[::-1].copy())
    _, _, backward, counts_reversed = _pass_against_oracle(renderer, lib, v, objects, segs[::-1].copy(), 16, "the set reversed")
    assert forward.tobytes() == backward.tobytes() and counts == counts_reversed
    shuffled = segs[np.random.default_rng(2).permutation(len(segs))]
    renderer.set_segments(shuffled)
    _, _, third, counts_shuffled = _pass_against_oracle(renderer, lib, v, objects, shuffled, 16, "the set shuffled")
    assert third.tobytes() == forward.tobytes() and counts_shuffled == counts


def test_the_loop_arm_of_the_diag_library_gives_the_same_bytes(lib):
    """rpt_segments_splat_loop_kernel (librpt_hip_diag.so, rpt_set_variant 1141), the lane-per-piece loop the cost tool measures the
    pooled kernel against, on the crafted set: the frame, both counts and the oracle's bytes, for every number of pieces."""
    import os
    if not os.path.exists(_ffi._path("librpt_hip_diag.so")):
        pytest.skip("librpt_hip_diag.so is not built (make -C relativitypathtracer_amd/csrc diag)")
    r = Renderer(0, diag=True)
    try:
        for name, motion in (("pinhole", "0.9c"), ("sphere", "rest")):
            scene, camera, objects, segs, bias = _case(r, 128, 72, 3, motion, name)
            r.set_segments(segs)
            for pieces in sg.PIECES:
                r.set_segment_options(inverse_square=True, depth_bias=bias, pieces=pieces)
                v = _view(scene, camera, 128, 72, 3, inverse_square=True, depth_bias=bias)
                _, _, pooled, pooled_counts = _pass_against_oracle(r, lib, v, objects, segs, pieces, f"{name} pieces {pieces}: the pooled kernel of the diag library")
                r.render()
                r.set_variant(LOOP_ARM)
                try:
                    r.render_segments()
                finally:
                    r.set_variant(0)
                assert r.read_framebuffer().tobytes() == pooled.tobytes(), f"{name} pieces {pieces}: the loop arm's frame differs from the pooled kernel's"
                assert r.last_segments() == pooled_counts
    finally:
        r.close()


def test_the_product_library_does_not_know_the_loop_arm(renderer):
    with pytest.raises(RenderError):
        renderer.set_variant(LOOP_ARM)
    renderer.set_variant(0)


def test_the_accumulator_is_clean_after_every_pass_and_shared_with_the_stars_and_the_particles(renderer, lib, stars_lib, particles_lib):
    scene, camera, objects, segs, _ = _case(renderer)
    renderer.set_segments(segs)
    v = _view(scene, camera, 128, 72, 3)
    P = 16
    _, _, first, _ = _pass_against_oracle(renderer, lib, v, objects, segs, P, "first frame")
    _, _, second, _ = _pass_against_oracle(renderer, lib, v, objects, segs, P, "second frame")
    assert first.tobytes() == second.tobytes()
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "the pass twice on one frame", passes=2)
    renderer.set_scene_params(scene, 67, 41)            # another size (a smaller frame in the same accumulator), and back
    _, records = _frames(renderer)
    small, _, _ = sg.crafted(records, objects, camera, 67, 41, -1)
    renderer.set_segments(small)
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 3), objects, small, P, "67 x 41 in between")
    renderer.set_scene_params(scene, 128, 72)
    renderer.set_segments(segs)
    _, _, again, _ = _pass_against_oracle(renderer, lib, v, objects, segs, P, "back at 128 x 72")
    assert again.tobytes() == first.tobytes()
    # a star pass and a particle pass before and after on the same context: each pass finds the accumulator clean and leaves it so
    E = scene.camera_lorentz()[1]
    cat, _ = sc.catalogue(camera, 128, 72, E, -1)
    sv = sc.view(camera, 128, 72, E, -1, 3, scene.params["white_point"])
    renderer.set_stars(cat)
    before, records = _frames(renderer)
    ps, _, _ = pc.crafted(records, objects, camera, 128, 72, -1)
    renderer.set_particles(ps)
    renderer.set_particle_options()
    renderer.render_stars()
    renderer.render_particles()
    renderer.render_segments()
    renderer.render_particles()
    renderer.render_stars()
    got = renderer.read_framebuffer().copy()
    pv = pc.view(camera, 128, 72, -1, 3, scene.params["white_point"])
    want, _ = sc.oracle_pass(stars_lib, sv, cat, before, records)
    want, _ = pc.oracle_pass(particles_lib, pv, objects, ps, want, records)
    want, segment_counts = sg.oracle_pass(lib, v, objects, segs, P, want, records)
    want, particle_counts = pc.oracle_pass(particles_lib, pv, objects, ps, want, records)
    want, star_counts = sc.oracle_pass(stars_lib, sv, cat, want, records)
    _same_pixels(got, want, "stars, particles, segments, particles, stars")
    assert renderer.last_stars() == star_counts and renderer.last_particles() == particle_counts and renderer.last_segments() == segment_counts
    renderer.set_stars(None)
    renderer.set_particles(None)
    fresh = Renderer(0)                                 # a larger frame than the context has had: a new accumulator, first made by this pass
    try:
        _setup(fresh, scene, 67, 41, camera, 3)
        fresh.set_segments(small)
        _pass_against_oracle(fresh, lib, _view(scene, camera, 67, 41, 3), objects, small, P, "a fresh context at 67 x 41")
        fresh.set_scene_params(scene, 128, 72)
        fresh.set_segments(segs)
        _, _, grown, _ = _pass_against_oracle(fresh, lib, v, objects, segs, P, "grown to 128 x 72")
        assert grown.tobytes() == first.tobytes()
    finally:
        fresh.close()


def test_off_means_off(renderer, lib):
    fresh = Renderer(0)
    try:
        fresh.render_segments()                         # no set: nothing is checked, not even that a scene is there
        assert fresh.last_segments() == (0, 0)
    finally:
        fresh.close()
    scene, camera, objects, segs, _ = _case(renderer, 67, 41, 0, "rest")
    renderer.set_segments(None)
    before, _ = _frames(renderer)
    variant = renderer.last_variant()
    renderer.render_segments()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_variant() == variant and renderer.last_segments() == (0, 0)
    renderer.set_segments(segs)
    _, _, _, counts = _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, segs, 16, "a set first")
    assert counts[1] > 0
    renderer.set_segments(None)
    before, _ = _frames(renderer)
    renderer.render_segments()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_segments() == (0, 0)
    renderer.set_segments(np.zeros(0, dtype=segments.SEGMENT_DTYPE))
    renderer.render_segments()
    assert renderer.read_framebuffer().tobytes() == before.tobytes()


def test_what_the_setters_refuse(renderer, lib):
    scene, camera, objects, good, bias = _case(renderer, 67, 41, 0, "rest")
    renderer.set_segment_options(inverse_square=True, depth_bias=bias, pieces=4)
    renderer.set_segments(good)
    for field, k, value, words in (("a", 0, np.nan, "finite"), ("a", 2, np.inf, "finite"), ("b", 1, -np.inf, "finite"), ("b", 0, np.nan, "finite"),
                                   ("rgb", 1, -np.inf, "finite"), ("rgb", 2, np.nan, "finite"), ("rgb", 0, -1e-20, "negative"),
                                   ("object", None, -1, "object is negative")):
        bad = good.copy()
        if k is None:
            bad[field][7] = value
        else:
            bad[field][7, k] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_segments: entry 7: .*" + words):
            renderer.set_segments(bad)
    lib_hip = renderer._lib
    assert lib_hip.rpt_set_segments(renderer._h, None, -1) == 1 and lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_segments:")
    # count x pieces > 2^21 with the pieces in force (4): refused before anything of the set is read
    assert lib_hip.rpt_set_segments(renderer._h, None, (1 << 19) + 1) == 1 and "count * pieces" in lib_hip.rpt_last_error(renderer._h).decode()
    for flags, depth_bias, pieces in ((2, 0.0, 4), (-1, 0.0, 4), (0, -1e-6, 4), (1, float("nan"), 4), (0, float("inf"), 4), (0, 0.0, 0), (0, 0.0, 3),
                                      (0, 0.0, 128), (0, 0.0, -16), (0, 0.0, 48)):
        assert lib_hip.rpt_set_segment_options(renderer._h, flags, depth_bias, pieces) == 1
        assert lib_hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_segment_options:")
    # every refusal kept the set and the options that were there
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0, inverse_square=True, depth_bias=bias), objects, good, 4, "after the refusals")
    # the pieces are held against the set that is there: 2^15 + 1 rods take pieces up to 32, not 64
    many = np.repeat(good[:1], (1 << 15) + 1)
    renderer.set_segment_options(pieces=32)
    renderer.set_segments(many)
    assert lib_hip.rpt_set_segment_options(renderer._h, 0, 0.0, 64) == 1 and "count * pieces" in lib_hip.rpt_last_error(renderer._h).decode()
    renderer.set_segments(good)
    renderer.set_segment_options(pieces=64)
    with pytest.raises(RenderError, match=r"rpt_set_segments: count \* pieces"):
        renderer.set_segments(many)
    _pass_against_oracle(renderer, lib, _view(scene, camera, 67, 41, 0), objects, good, 64, "after the load refusals")


def test_what_the_launch_refuses(renderer, lib):
    W, H = 67, 41
    scene, camera, objects, segs, _ = _case(renderer, W, H, 0, "rest")
    renderer.set_segments(segs)
    v = _view(scene, camera, W, H, 0)
    P = 16

    def refused(code, words):
        with pytest.raises(RenderError, match=rf"failed \({code}\): rpt_render_segments: .*{words}") as e:
            renderer.render_segments()
        assert e.value.code == code

    # a ray map has no inverse
    renderer.set_raymap(raymap("fisheye", W, H))
    renderer.set_projection("raymap")
    _frames(renderer)
    refused(1, "RPT_PROJECTION_RAYMAP")
    renderer.set_projection("pinhole")
    renderer.set_raymap(None)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "after the ray map")
    # an interval the cone has no closed form for
    two = eo.load_scene("cubes", "rest", 2)
    renderer.set_scene_params(two, W, H)
    _frames(renderer)
    refused(1, "interval is 2")
    renderer.set_scene_params(scene, W, H)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "after interval 2")
    # a set that names object index object_count: refused at the launch, whatever came last, the set or the objects
    n = len(objects)
    beyond = segs.copy()
    beyond["object"][5] = n
    renderer.set_segments(beyond)
    _frames(renderer)
    refused(1, f"names object {n}, the Object\\[\\] holds {n}")
    renderer.set_segments(segs)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "after the index beyond Object[]")
    last = segs.copy()
    last["object"][:] = n - 1
    renderer.set_segments(last)
    _pass_against_oracle(renderer, lib, v, objects, last, P, "every rod on the last object")
    renderer.set_objects(objects[:n - 1])
    _frames(renderer)
    refused(1, f"names object {n - 1}, the Object\\[\\] holds {n - 1}")
    renderer.upload_scene(scene)
    renderer.set_segments(segs)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "after fewer objects")
    # a context restricted by rpt_set_rows
    renderer.set_rows(0, 2, False)
    refused(1, "rpt_set_rows")
    renderer.set_rows(0, 1, False)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "after rpt_set_rows")
    # no event frame of this view
    renderer.set_orientation(0.1, 0.0, 0.0)
    renderer.render()
    refused(2, "the view has changed")
    renderer.set_orientation(0.0, 0.0, 0.0)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "after a stale event frame")


def test_with_a_sky_image_adaptive_aa_the_overlay_the_readouts_and_async(renderer, lib):
    W, H = 128, 72
    P = 16
    scene, camera, objects, segs, bias = _case(renderer, W, H, 3)
    renderer.set_segments(segs)
    renderer.set_segment_options(depth_bias=bias)
    v = _view(scene, camera, W, H, 3, depth_bias=bias)
    _, _, plain, _ = _pass_against_oracle(renderer, lib, v, objects, segs, P, "the constant background")
    y, x = np.mgrid[0:32, 0:64]
    image = np.ascontiguousarray(np.stack([40 + 3 * x, 30 + 6 * y, 200 - 2 * x], -1).astype(np.uint8))
    renderer.set_environment(image)
    _, _, with_sky, _ = _pass_against_oracle(renderer, lib, v, objects, segs, P, "over a sky image")
    assert with_sky.tobytes() != plain.tobytes() and renderer.last_variant() != 0
    renderer.set_environment(None)
    renderer.set_adaptive_aa(2, 8)
    _pass_against_oracle(renderer, lib, v, objects, segs, P, "with adaptive anti-aliasing")
    assert renderer.last_aa_variant() != 0
    renderer.set_adaptive_aa(1, 8)
    # the overlay and the readouts before and after
    displays = [dict(rate=1.0, offset=0.0, digits=3, decimals=1)] * len(objects)
    before, records = _frames(renderer)
    renderer.set_overlay(**OUTLINES)
    renderer.set_readouts(displays)
    renderer.render_overlay()
    renderer.render_readouts()
    renderer.render_segments()
    layers_first = renderer.read_framebuffer().copy()
    rgba, n_lines = overlay(before["rgba"], records.reshape(H, W), -1, **OUTLINES)
    rgba, n_digits = readout(rgba.reshape(-1, 4), records.reshape(H, W), displays)
    want = before.copy()
    want["rgba"] = rgba.reshape(-1, 4)
    want, counts = sg.oracle_pass(lib, v, objects, segs, P, want, records)
    _same_pixels(layers_first, want, "overlay, readouts, then segments")
    assert renderer.last_overlay_pixels() == n_lines > 0 and renderer.last_readout_pixels() == n_digits and renderer.last_segments() == counts
    renderer.render()
    renderer.render_segments()
    renderer.render_overlay()
    renderer.render_readouts()
    segments_first = renderer.read_framebuffer().copy()
    want, counts = sg.oracle_pass(lib, v, objects, segs, P, before, records)
    rgba, _ = overlay(want["rgba"], records.reshape(H, W), -1, **OUTLINES)
    rgba, _ = readout(rgba.reshape(-1, 4), records.reshape(H, W), displays)
    want["rgba"] = rgba.reshape(-1, 4)
    _same_pixels(segments_first, want, "segments, then overlay and readouts")
    assert renderer.last_segments() == counts
    renderer.set_overlay()
    renderer.set_readouts(None)
    # async, then rpt_sync
    renderer.render()
    renderer.render_segments()
    blocking = renderer.read_framebuffer().copy()
    renderer.render_async()
    renderer.render_events(async_=True)
    renderer.render_segments(async_=True)
    renderer.sync()
    assert renderer.read_framebuffer().tobytes() == blocking.tobytes() and renderer.last_segments() == counts


def test_render_scene_takes_segments(lib):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 67, 41
    scene = _scene("cubes", "0.9c")
    camera = sg.CAMERAS["pinhole"]
    objects = sg.scene_objects(scene, camera)
    plain, _, records = render_scene(scene, W, H, events=True)
    segs, _, bias = sg.crafted(records.reshape(-1), objects, camera, W, H, -1)
    lit, _, records_again = render_scene(scene, W, H, segments=segs, segment_options=dict(inverse_square=True, depth_bias=bias, pieces=8))
    assert records_again.tobytes() == records.tobytes()
    want, counts = sg.oracle_pass(lib, _view(scene, camera, W, H, 0, inverse_square=True, depth_bias=bias), objects, segs, 8, plain, records)
    _same_pixels(lit, want, "render_scene(segments=)")
    assert counts[1] > 0
