"""Thermal particles on the MI355X (kernel 1132 before 1131): the device's own pre-pass framebuffer and records go through
tests/native/thermal_oracle.c, and rpt_render_particles with rpt_set_particle_temperatures must give those bytes — all 16 of every pixel
— and both counts of rpt_last_particles.  Scene, cameras, sizes, sets and temperatures are tests/thermal_cases.py's, built from the
device's own records (their non-vacuity is asserted in tests/test_thermal_model.py on CPU frames): `cubes` at 128 x 72 and 67 x 41, the
pinhole and the full-circle equirect, camera at rest and at 0.9 c, the four Doppler settings, interval -1 and 0, the inverse square and a
depth bias; 2000 random particles plus crafted ones, T at 500 and 1e8, x_G = 0 mixed in; and the windowed three-leg body.

`cubes` has moving cubes: a particle riding one has D != 1 for a camera at rest too, so there the frame without temperatures is held
against the frame of the particles whose D is exactly 1 (those riding a body at rest), not of the whole set."""
import ctypes as C

import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
import thermal_cases as tc
from relativitypathtracer_amd.renderer import RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return tc.build_particles_library(tmp_path_factory.mktemp("thermal_particles"))


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
    r.render()
    before = r.read_framebuffer().copy()
    return before, r.render_events().copy()


def _pass_against_oracle(r, lib, v, objects, ps, T, what, windows=None):
    """Colour frame, event frame, the pass with the set and the temperatures the context HOLDS (T None: none), against the oracle."""
    before, records = _frames(r)
    r.render_particles()
    after = r.read_framebuffer().copy()
    if T is None:
        want, counts = pc.oracle_pass(lib, v, objects, ps, before, records, windows)
    else:
        want, counts = tc.oracle_particles_pass(lib, v, objects, ps, tc.x_green32(T), before, records, windows)
    _same_pixels(after, want, what)
    assert r.last_particles() == counts, f"{what}: rpt_last_particles {r.last_particles()}, the oracle {counts}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts


def _case(renderer, W=128, H=72, flags=3, motion="0.9c", name="pinhole"):
    scene = _scene(motion)
    camera = tc.CAMERAS[name]
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, flags)
    _, records = _frames(renderer)
    ps, T, groups, bias = tc.particle_case(records, objects, camera, W, H, -1)
    return scene, camera, objects, ps, T, groups, bias


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(tc.CAMERAS))
@pytest.mark.parametrize("motion", tc.MOTIONS)
def test_the_pass_equals_the_c_oracle(renderer, lib, motion, name, size):
    W, H = size
    camera = tc.CAMERAS[name]
    for interval in tc.INTERVALS:
        scene = _scene(motion, interval)
        objects = pc.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera)
        _, records = _frames(renderer)
        ps, T, groups, bias = tc.particle_case(records, objects, camera, W, H, interval)
        assert len(ps) <= 8192 and (T == 0).sum() > 500 and (T == tc.T_MIN).any() and (T == tc.T_MAX).any()
        xg = tc.x_green32(T)
        for flags in tc.FLAGS:
            renderer.set_doppler(bool(flags & 1), bool(flags & 2))
            for inverse_square, depth_bias in ((False, 0.0), (True, bias)):
                what = f"{motion} {name} {W}x{H} interval {interval} flags {flags} inverse square {inverse_square} bias {depth_bias:g}"
                renderer.set_particle_options(inverse_square=inverse_square, depth_bias=depth_bias)
                v = _view(scene, camera, W, H, flags, inverse_square=inverse_square, depth_bias=depth_bias)
                renderer.set_particles(ps, T)
                _, _, thermal, counts = _pass_against_oracle(renderer, lib, v, objects, ps, T, what)
                assert 0 < counts[0] < len(ps), what
                # none at all, and (once per Doppler setting) an all-zero array: the plain pass's frame, byte for byte
                renderer.set_particle_temperatures(None)
                _, _, plain, plain_counts = _pass_against_oracle(renderer, lib, v, objects, ps, None, what + ", no temperatures")
                if not inverse_square:
                    renderer.set_particle_temperatures(np.zeros(len(ps), dtype=np.float32))
                    _, _, zeros, zero_counts = _pass_against_oracle(renderer, lib, v, objects, ps, np.zeros(len(ps), dtype=np.float32), what + ", all-zero temperatures")
                    assert zeros.tobytes() == plain.tobytes() and zero_counts == plain_counts, what
                if interval == 0 or not flags & 1:
                    assert thermal.tobytes() == plain.tobytes() and counts == plain_counts, f"{what}: the temperatures changed a frame they have no part in"
                    continue
                colours = tc.oracle_particles_colours(lib, v, objects, ps, xg)
                if motion == "rest":        # the particles riding a body at rest, D == 1 exactly: with or without temperatures, one frame
                    still = colours["visible"] & (colours["D"] == 1.0)
                    assert still.sum() > 1000, f"{what}: {int(still.sum())} particles at rest"
                    renderer.set_particles(ps[still].copy(), T[still].copy())
                    _, _, a, ca = _pass_against_oracle(renderer, lib, v, objects, ps[still].copy(), T[still].copy(), what + ", at rest, temperatures")
                    renderer.set_particle_temperatures(None)
                    _, _, b, cb = _pass_against_oracle(renderer, lib, v, objects, ps[still].copy(), None, what + ", at rest, none")
                    assert a.tobytes() == b.tobytes() and ca == cb, f"{what}: the temperatures changed the frame of particles at rest"
                else:
                    assert thermal.tobytes() != plain.tobytes(), f"{what}: the temperatures changed nothing"
    renderer.set_particle_temperatures(None)


def test_a_thousand_thermal_particles_on_one_pixel_forwards_and_shuffled(renderer, lib):
    scene, camera, objects, ps, T, groups, _ = _case(renderer)
    v = _view(scene, camera, 128, 72, 3)
    renderer.set_particles(ps, T)
    _, _, forward, counts = _pass_against_oracle(renderer, lib, v, objects, ps, T, "the set as given")
    assert groups["pile"].stop - groups["pile"].start == 1000 and np.all(T[groups["pile"]] > 0)
    order = np.random.default_rng(3).permutation(len(ps))
    for what, o in (("reversed", np.arange(len(ps))[::-1]), ("shuffled", order)):
        renderer.set_particles(ps[o].copy(), T[o].copy())
        _, _, other, other_counts = _pass_against_oracle(renderer, lib, v, objects, ps[o].copy(), T[o].copy(), what)
        assert other.tobytes() == forward.tobytes() and other_counts == counts, what
    renderer.set_particle_temperatures(None)


def test_thermal_lamps_on_a_body_of_three_legs_keep_their_windows(renderer, lib):
    W, H = 128, 72
    _, scene, ps = pc.turnaround()
    camera = tc.CAMERAS["pinhole"]
    objects = pc.scene_objects(scene, camera)
    windows = scene.windows()
    T = np.where(np.arange(len(ps)) % 2 == 0, 4000.0, 0.0).astype(np.float32)
    _setup(renderer, scene, W, H, camera, 3)
    renderer.set_particles(ps, T)
    v = _view(scene, camera, W, H, 3)
    _, _, windowed, counts = _pass_against_oracle(renderer, lib, v, objects, ps, T, "three legs, their windows", windows=windows)
    renderer.set_particle_temperatures(None)
    _, _, plain, plain_counts = _pass_against_oracle(renderer, lib, v, objects, ps, None, "three legs, no temperatures", windows=windows)
    assert counts[0] == plain_counts[0] > 0 and windowed.tobytes() != plain.tobytes()
    renderer.set_object_windows(None)


def test_off_means_off_and_the_set_keeps_its_temperatures(renderer, lib):
    scene, camera, objects, ps, T, _, _ = _case(renderer, 67, 41)
    v = _view(scene, camera, 67, 41, 3)
    renderer.set_particles(ps, T)
    _, _, thermal, _ = _pass_against_oracle(renderer, lib, v, objects, ps, T, "temperatures set")
    renderer.set_particles(ps[::-1].copy())                 # replacing the set keeps the array: entry i now belongs to another particle
    _pass_against_oracle(renderer, lib, v, objects, ps[::-1].copy(), T, "the set replaced, the temperatures kept")
    renderer.set_particles(ps)
    renderer.set_particle_temperatures(None)
    _, _, plain, _ = _pass_against_oracle(renderer, lib, v, objects, ps, None, "after NULL")
    assert plain.tobytes() != thermal.tobytes()
    renderer.set_particle_temperatures(T)
    renderer.set_particle_temperatures(np.zeros(0, dtype=np.float32))      # a count of 0 is NULL
    _, _, again, _ = _pass_against_oracle(renderer, lib, v, objects, ps, None, "after a count of 0")
    assert again.tobytes() == plain.tobytes()
    renderer.set_particle_temperatures(T)
    renderer.set_particles(None)                            # no set: no pass, whatever the temperatures
    before, _ = _frames(renderer)
    renderer.render_particles()
    assert renderer.read_framebuffer().tobytes() == before.tobytes() and renderer.last_particles() == (0, 0)
    renderer.set_particle_temperatures(None)


def test_what_the_calls_refuse(renderer, lib):
    scene, camera, objects, ps, T, _, _ = _case(renderer, 67, 41)
    v = _view(scene, camera, 67, 41, 3)
    renderer.set_particles(ps, T)
    hip, h = renderer._lib, renderer._h
    for value, words in ((np.nan, "finite"), (np.inf, "finite"), (-np.inf, "finite"), (499.99997, "within 500"), (1.0000001e8, "within 500"),
                         (-5000.0, "within 500"), (1e-20, "within 500")):
        bad = T.copy()
        bad[7] = value
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_set_particle_temperatures: entry 7: .*" + words):
            renderer.set_particle_temperatures(bad)
    assert hip.rpt_set_particle_temperatures(h, T.ctypes.data_as(C.POINTER(C.c_float)), -1) == 1
    assert hip.rpt_last_error(h).decode().startswith("rpt_set_particle_temperatures: count")
    assert hip.rpt_set_particle_temperatures(h, None, (1 << 22) + 1) == 1 and hip.rpt_last_error(h).decode().startswith("rpt_set_particle_temperatures: count")
    assert hip.rpt_set_particle_options(h, 2, 0.0) == 1     # (flag bit 2 stays refused)
    _pass_against_oracle(renderer, lib, v, objects, ps, T, "every refusal kept the array that was there")
    for other in (T[:-1].copy(), np.concatenate([T, T[:1]])):
        renderer.set_particle_temperatures(other)
        _frames(renderer)
        with pytest.raises(RenderError, match=rf"failed \(1\): rpt_render_particles: {len(other)} temperatures are set .*the set holds {len(ps)}") as e:
            renderer.render_particles()
        assert e.value.code == 1
        renderer.set_particle_temperatures(T)
        _pass_against_oracle(renderer, lib, v, objects, ps, T, "after the count mismatch")
    renderer.set_particles(ps[:100].copy())
    _frames(renderer)
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_particles: .*the set holds 100"):
        renderer.render_particles()
    renderer.set_particles(ps)
    _pass_against_oracle(renderer, lib, v, objects, ps, T, "after a shorter set")
    renderer.set_particle_temperatures(None)


def test_async_and_render_scene(renderer, lib):
    from relativitypathtracer_amd.renderer import render_scene
    scene, camera, objects, ps, T, _, bias = _case(renderer)
    v = _view(scene, camera, 128, 72, 3, depth_bias=bias)
    renderer.set_particle_options(depth_bias=bias)
    renderer.set_particles(ps, T)
    _, _, blocking, counts = _pass_against_oracle(renderer, lib, v, objects, ps, T, "blocking")
    renderer.render_async()
    renderer.render_events(async_=True)
    renderer.render_particles(async_=True)
    renderer.sync()
    assert renderer.read_framebuffer().tobytes() == blocking.tobytes() and renderer.last_particles() == counts
    renderer.set_particle_temperatures(None)
    renderer.set_particle_options()
    W, H = 67, 41
    plain, _, records = render_scene(scene, W, H, events=True)
    small, Ts, _, _ = tc.particle_case(records.reshape(-1), objects, camera, W, H, -1)
    lit, _, _ = render_scene(scene, W, H, particles=small, particle_temperatures=Ts)
    want, _ = tc.oracle_particles_pass(lib, _view(scene, camera, W, H, 0), objects, small, tc.x_green32(Ts), plain, records)
    _same_pixels(lit, want, "render_scene(particles=, particle_temperatures=)")
    with pytest.raises(RenderError, match="rpt_render_particles: .*temperatures are set"):      # (the keyword reaches the context)
        render_scene(scene, W, H, particles=small, particle_temperatures=Ts[:-1])
