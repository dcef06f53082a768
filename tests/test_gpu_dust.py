"""Lit particles on the MI355X (rpt_set_particle_lighting): the device's own pre-pass framebuffer and records go through
tests/native/dust_oracle.c, the C restatement of rules D0-D7, and the pass must give those bytes — all 16 of every pixel —, all four counts
(rpt_last_particles and rpt_last_particle_lighting), and leave the record buffer as it was.  Feeding the reference what the device
rendered isolates kernels 1134, 1135 and 1136 (and 1131) from every other.  Scenes, clouds and windows are those of tests/dust_cases.py;
their non-vacuity is asserted in tests/test_dust_model.py with the oracle, and where a count is at hand, here.  Frames are 128 x 72 at
most, sets 4096 grains at most."""
import numpy as np
import pytest

import dust_cases as dc
import events_oracle as eo
import particles_cases as pc
import segments_cases as gc
import stars_cases as sc
from relativitypathtracer_amd import particles, segments
from relativitypathtracer_amd.renderer import RenderError, Renderer

pytestmark = pytest.mark.gpu

LIT, SHADOWED, AMBIENT = dc.LIT, dc.SHADOWED, dc.AMBIENT


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return dc.build_library(tmp_path_factory.mktemp("dust"))


def _setup(r, scene, W, H, camera, flags=0, windows=None):
    r.set_variant(0)
    r.set_msaa(1)
    r.set_adaptive_aa(1, 8)
    r.set_doppler(bool(flags & 1), bool(flags & 2))
    r.set_environment(None)
    r.set_environment_frame(scene.camera_lorentz()[1])
    r.set_debug_rgb(False)
    r.set_overlay()
    r.set_stars(None)
    r.set_segments(None)
    r.set_particle_options()
    r.set_particle_lighting()
    r.set_particles(None, [])
    sc.setup_camera(r, camera)
    r.upload_scene(scene)
    r.set_object_windows(windows)
    r.set_readouts(None)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _lighting(r, lighting):
    r.set_particle_lighting(lit=bool(lighting & LIT), shadows=bool(lighting & SHADOWED), ambient=bool(lighting & AMBIENT))


def _view(scene, camera, W, H, flags, **options):
    return pc.view(camera, W, H, scene.params["interval"], flags, scene.params["white_point"], **options)


def _same_pixels(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 16)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 16)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at pixel {k}: got {g[k].tolist()} want {w[k].tolist()}")


def _pass_against_oracle(r, lib, scene, v, objects, lighting, ps, what, records=None, windows=None, async_=False):
    """A fresh colour frame (and event frame, unless the view's records are handed in), the pass with the set and the lighting the context
    HOLDS, against the oracle: bytes, four counts, the records untouched."""
    if async_:
        r.render_async()
        r.render_events(async_=True)
        r.render_particles(async_=True)
        r.sync()
        r.render()
        before = r.read_framebuffer().copy()
        records = r.render_events().copy()
        r.render_async()
        r.render_events(async_=True)
        r.render_particles(async_=True)
        r.sync()
    else:
        r.render()
        before = r.read_framebuffer().copy()
        if records is None:
            records = r.render_events().copy()
        r.render_particles()
    after = r.read_framebuffer().copy()
    want, counts, pairs = dc.oracle_pass(lib, scene, v, objects, lighting, ps, before, records, windows)
    _same_pixels(after, want, what)
    assert r.last_particles() == counts, f"{what}: rpt_last_particles {r.last_particles()}, the oracle {counts}"
    assert r.last_particle_lighting() == pairs, f"{what}: rpt_last_particle_lighting {r.last_particle_lighting()}, the oracle {pairs}"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after, counts, pairs


@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(pc.CAMERAS))
@pytest.mark.parametrize("motion", ["rest", "0.9c"])
@pytest.mark.parametrize("scene_name", ["shadows", "cubes"])
def test_the_lit_pass_equals_the_c_oracle(renderer, lib, scene_name, motion, name, size):
    """Every Doppler setting x {LIT, LIT|SHADOWED, LIT|AMBIENT, LIT|SHADOWED|AMBIENT}, the inverse square on for every other one."""
    W, H = size
    camera = pc.CAMERAS[name]
    scene = dc.scene(scene_name, motion)
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera)
    ps = dc.cloud(scene_name, scene, 4096)
    renderer.set_particles(ps)
    renderer.render()
    records = renderer.render_events().copy()
    totals = np.zeros(4, dtype=np.int64)
    for flags in (0, 1, 2, 3):
        renderer.set_doppler(bool(flags & 1), bool(flags & 2))
        for n, lighting in enumerate(dc.LIGHTINGS):
            inverse_square = bool((flags + n) & 1)
            renderer.set_particle_options(inverse_square=inverse_square)
            _lighting(renderer, lighting)
            v = _view(scene, camera, W, H, flags, inverse_square=inverse_square)
            case = f"{scene_name} {motion} {name} {W}x{H} flags {flags} lighting {lighting} inverse square {inverse_square}"
            before, _, after, counts, pairs = _pass_against_oracle(renderer, lib, scene, v, objects, lighting, ps, case, records)
            assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]) and np.array_equal(after["x"], before["x"]) and np.array_equal(after["y"], before["y"])
            assert int((after["rgba"] != before["rgba"]).any(axis=1).sum()) == counts[1]
            assert 0 < counts[0] <= len(ps) and pairs[0] > 0, case
            assert (pairs[1] > 0) == bool(lighting & SHADOWED), f"{case}: pairs shadowed {pairs[1]}"
            totals += (counts[0], counts[1], pairs[0], pairs[1])
    assert (totals > 0).all(), totals


def test_a_lamp_switched_on_and_an_occluder_that_ends(renderer, lib):
    """Time windows: kernel 1134's pointer path (the lamp's window) and kernel 1136 (the lamp's, and the red sphere's on the shadow ray)."""
    W, H = 128, 72
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    ps = dc.cloud("shadows", scene, 4096)
    windows = dc.shadows_windows(lib, scene, objects, ps)
    got = {}
    for held in (None, windows):
        _setup(renderer, scene, W, H, camera, 3, held)
        renderer.set_particles(ps)
        for lighting in (LIT, LIT | SHADOWED):
            _lighting(renderer, lighting)
            v = _view(scene, camera, W, H, 3)
            what = f"windows {'set' if held is not None else 'not set'}, lighting {lighting}"
            got[(held is not None, lighting)] = _pass_against_oracle(renderer, lib, scene, v, objects, lighting, ps, what, windows=held)[3:]
    # the front: with the lamp's window fewer pairs light, but some do
    assert 0 < got[(True, LIT)][1][0] < got[(False, LIT)][1][0], got
    assert 0 < got[(True, LIT | SHADOWED)][1][1], got
    # every window at its default: the windowed kernels give the un-windowed bytes
    default = np.tile(np.array([-np.inf, np.inf], dtype=np.float32), (len(windows), 1))
    _setup(renderer, scene, W, H, camera, 3, default)
    renderer.set_particles(ps)
    _lighting(renderer, LIT | SHADOWED)
    _, _, with_defaults, counts, pairs = _pass_against_oracle(renderer, lib, scene, _view(scene, camera, W, H, 3), objects, LIT | SHADOWED, ps, "default windows", windows=default)
    assert (counts, pairs) == got[(False, LIT | SHADOWED)]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 4096])
def test_every_count_of_grains(renderer, lib, count):
    W, H = 67, 41
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, 2)
    cloud = dc.cloud("shadows", scene, 4096)
    ps = cloud[np.random.default_rng(count).permutation(len(cloud))[:count]] if count < 4096 else np.concatenate([cloud, cloud[:4096 - len(cloud)]])
    assert len(ps) == count
    renderer.set_particles(ps)
    _lighting(renderer, LIT | SHADOWED | AMBIENT)
    _pass_against_oracle(renderer, lib, scene, _view(scene, camera, W, H, 2), objects, LIT | SHADOWED | AMBIENT, ps, f"{count} grains")


@pytest.mark.parametrize("lights", [0, 1, 3])
def test_zero_one_and_three_lights(renderer, lib, lights):
    W, H = 128, 72
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("cubes", "rest", lights=lights)
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, 3)
    ps = dc.cloud("cubes", scene, 2048)
    renderer.set_particles(ps)
    for lighting in dc.LIGHTINGS:
        _lighting(renderer, lighting)
        before, _, after, counts, pairs = _pass_against_oracle(renderer, lib, scene, _view(scene, camera, W, H, 3), objects, lighting, ps, f"{lights} lights, lighting {lighting}")
        assert counts[0] > 0
        if lights == 0:         # all dark, or the ambient term only: a seen grain in the dark is still seen
            assert pairs == (0, 0) and (counts[1] > 0) == bool(lighting & AMBIENT), (counts, pairs)
        else:
            # no windows and no grain at a lamp's centre: every seen grain makes one pair with every lamp, lit or shadowed
            assert pairs[0] + pairs[1] == lights * counts[0] and pairs[0] > 0, (counts, pairs)


def test_a_grain_riding_the_lamp_and_a_grain_at_its_centre(renderer, lib):
    """i == object is allowed: a grain riding a lamp is lit by it (the lamp of `shadows`, at 0.95c).  A grain AT a lamp's centre has
    len == 0 and that pair is skipped: a lamp at rest before a camera at rest, whose Lorentz matrices are the identity, so that the
    centre comes back exactly (through a boost it comes back within rounding, and len is some 1e-7).  The grain sits inside the lamp's
    sphere, so the depth bias is what lets the frame see it."""
    W, H = 128, 72
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, 3)
    centre = np.array([-5.0, -3.0, 10.0])
    ps = particles.from_arrays(np.stack([centre + (0.0, 0.9, 0.0), centre + (0.0, 0.0, -1.2), centre + (1.5, 0.5, 0.0)]), dc.LAMP, (0.7, 0.7, 0.7))
    detail = dc.oracle_pairs(lib, scene, objects, 3, LIT, ps)
    assert detail["state"][:, dc.LAMP].tolist() == [1, 1, 1]
    renderer.set_particles(ps)
    _lighting(renderer, LIT)
    _, _, _, counts, pairs = _pass_against_oracle(renderer, lib, scene, _view(scene, camera, W, H, 3), objects, LIT, ps, "riding the lamp")
    assert counts[0] > 0 and pairs[0] == counts[0], (counts, pairs)
    scene = dc.scene("cubes", "rest", lights=3)
    objects = pc.scene_objects(scene, camera)
    lamp, centre = 35, np.array([3.0, -2.0, 9.0])           # LIGHT_TEXT[1]: at rest, radius 0.2
    _setup(renderer, scene, W, H, camera, 0)
    ps = particles.from_arrays(np.stack([centre, centre + (0.0, 0.5, 0.0)]), lamp, (0.7, 0.7, 0.7))
    detail = dc.oracle_pairs(lib, scene, objects, 0, LIT, ps)
    assert detail["state"][:, lamp].tolist() == [2, 1] and detail["len"][0, lamp] == 0.0
    assert (detail["state"][:, [34, 36]] == 1).all()
    renderer.set_particles(ps)
    renderer.set_particle_options(depth_bias=1.0)
    _lighting(renderer, LIT)
    _, _, _, counts, pairs = _pass_against_oracle(renderer, lib, scene, _view(scene, camera, W, H, 0, depth_bias=1.0), objects, LIT, ps, "at the lamp's centre")
    assert counts[0] == 2 and pairs == (5, 0), (counts, pairs)


def test_the_sums_do_not_depend_on_the_order(renderer, lib):
    W, H = 128, 72
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "0.9c")
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, 2)
    ps = dc.cloud("shadows", scene, 4096)
    _lighting(renderer, LIT | SHADOWED)
    v = _view(scene, camera, W, H, 2)
    frames = []
    for what, order in (("as given", np.arange(len(ps))), ("reversed", np.arange(len(ps))[::-1]), ("shuffled", np.random.default_rng(2).permutation(len(ps)))):
        renderer.set_particles(ps[order].copy())
        frames.append(_pass_against_oracle(renderer, lib, scene, v, objects, LIT | SHADOWED, ps[order].copy(), f"the set {what}")[2:])
    assert frames[0][0].tobytes() == frames[1][0].tobytes() == frames[2][0].tobytes()
    assert frames[0][1:] == frames[1][1:] == frames[2][1:]


def test_interval_0_and_flags_0_are_the_plain_pass(renderer, lib):
    """D0: with light propagation off a lit pass equals the plain one byte for byte.  Off means off: flags 0 launches kernel 1130 and gives
    the bytes of the particle oracle, which knows nothing of lights."""
    W, H = 67, 41
    camera = pc.CAMERAS["pinhole"]
    for interval in (0, -1):
        scene = dc.scene("shadows", "rest", interval)
        objects = pc.scene_objects(scene, camera)
        _setup(renderer, scene, W, H, camera, 3)
        ps = dc.cloud("shadows", scene, 1024)
        renderer.set_particles(ps)
        v = _view(scene, camera, W, H, 3)
        renderer.render()
        before = renderer.read_framebuffer().copy()
        records = renderer.render_events().copy()
        renderer.render_particles()
        plain = renderer.read_framebuffer().copy()
        plain_counts = renderer.last_particles()
        want, counts = pc.oracle_pass(lib, v, objects, ps, before, records)
        _same_pixels(plain, want, f"interval {interval}: lighting 0 against the particle oracle")
        assert plain_counts == counts and counts[1] > 0 and renderer.last_particle_lighting() == (0, 0)
        if interval == 0:
            for lighting in dc.LIGHTINGS:
                _lighting(renderer, lighting)
                _, _, lit, lit_counts, pairs = _pass_against_oracle(renderer, lib, scene, v, objects, lighting, ps, f"interval 0, lighting {lighting}", records)
                assert lit.tobytes() == plain.tobytes() and lit_counts == plain_counts and pairs == (0, 0)
        else:
            _lighting(renderer, LIT)
            _, _, lit, _, pairs = _pass_against_oracle(renderer, lib, scene, v, objects, LIT, ps, "interval -1, lit", records)
            assert lit.tobytes() != plain.tobytes() and pairs[0] > 0
            renderer.set_particle_lighting()
            renderer.render()
            renderer.render_particles()
            assert renderer.read_framebuffer().tobytes() == plain.tobytes() and renderer.last_particle_lighting() == (0, 0)


def test_the_accumulator_stays_clean_among_the_other_passes_and_async(renderer, lib, tmp_path_factory):
    """A star pass, a plain particle pass and a segment pass before and after a lit pass on one context; then the lit pass enqueued only."""
    W, H = 128, 72
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    stars_lib = sc.build_library(tmp_path_factory.mktemp("dust_stars"))
    seg_lib = gc.build_library(tmp_path_factory.mktemp("dust_segments"))
    _setup(renderer, scene, W, H, camera, 3)
    ps = dc.cloud("shadows", scene, 2048)
    E = scene.camera_lorentz()[1]
    cat, _ = sc.catalogue(camera, W, H, E, -1)
    sv = sc.view(camera, W, H, E, -1, 3, scene.params["white_point"])
    rods = segments.box_edges(dc.FLOOR, dc.BOX[0], dc.BOX[1], (0.5, 0.5, 0.9))
    v = _view(scene, camera, W, H, 3)
    renderer.set_stars(cat)
    renderer.set_segment_options()
    renderer.set_segments(rods)
    renderer.set_particles(ps)
    renderer.render()
    before = renderer.read_framebuffer().copy()
    records = renderer.render_events().copy()
    want = before
    tallies = []
    for lighting in (0, LIT | SHADOWED, 0):
        renderer.render_stars()
        want, _ = sc.oracle_pass(stars_lib, sv, cat, want, records)
        renderer.set_particle_lighting(lit=bool(lighting & LIT), shadows=bool(lighting & SHADOWED))
        renderer.render_particles()
        want, counts, pairs = dc.oracle_pass(lib, scene, v, objects, lighting, ps, want, records)
        tallies.append((renderer.last_particles(), renderer.last_particle_lighting(), counts, pairs))
        renderer.render_segments()
        want, _ = gc.oracle_pass(seg_lib, v, objects, rods, 16, want, records)
    _same_pixels(renderer.read_framebuffer(), want, "stars, particles, segments; stars, lit particles, segments; and again plain")
    for got_counts, got_pairs, counts, pairs in tallies:
        assert got_counts == counts and got_pairs == pairs
    assert tallies[1][3][0] > 0 and tallies[0][3] == tallies[2][3] == (0, 0)
    renderer.set_stars(None)
    renderer.set_segments(None)
    _lighting(renderer, LIT | SHADOWED | AMBIENT)
    _pass_against_oracle(renderer, lib, scene, v, objects, LIT | SHADOWED | AMBIENT, ps, "async", async_=True)


def test_render_scene_takes_particle_lighting(lib):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 67, 41
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    ps = dc.cloud("shadows", scene, 1024)
    plain, _, records = render_scene(scene, W, H, events=True)
    lit, _, _ = render_scene(scene, W, H, particles=ps, particle_lighting=dict(lit=True, shadows=True))
    want, counts, pairs = dc.oracle_pass(lib, scene, _view(scene, camera, W, H, 0), objects, LIT | SHADOWED, ps, plain, records.reshape(-1))
    _same_pixels(lit, want, "render_scene(particle_lighting=)")
    assert counts[1] > 0 and pairs[0] > 0 and pairs[1] > 0


def test_what_the_setter_and_the_launch_refuse(renderer, lib):
    W, H = 67, 41
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    objects = pc.scene_objects(scene, camera)
    _setup(renderer, scene, W, H, camera, 0)
    ps = dc.cloud("shadows", scene, 512)
    renderer.set_particles(ps)
    _lighting(renderer, LIT | AMBIENT)
    v = _view(scene, camera, W, H, 0)
    hip = renderer._lib
    for flags in (8, -1, SHADOWED, AMBIENT, SHADOWED | AMBIENT, LIT | 16):
        assert hip.rpt_set_particle_lighting(renderer._h, flags) == 1
        assert hip.rpt_last_error(renderer._h).decode().startswith("rpt_set_particle_lighting:")
        # the previous value is kept
        _pass_against_oracle(renderer, lib, scene, v, objects, LIT | AMBIENT, ps, f"after the refused flags {flags}")
    # rpt_set_particle_options still refuses bit 2: the lighting is no bit of it
    assert hip.rpt_set_particle_options(renderer._h, 2, 0.0) == 1
    # LIT with temperatures
    renderer.set_particle_temperatures(np.full(len(ps), 5000.0, dtype=np.float32))
    renderer.render()
    renderer.render_events()
    with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_particles: RPT_PARTICLES_LIT with particle temperatures") as e:
        renderer.render_particles()
    assert e.value.code == 1                            # RPT_ERR_ARG
    renderer.set_particle_temperatures(None)
    _pass_against_oracle(renderer, lib, scene, v, objects, LIT | AMBIENT, ps, "after the temperatures")
    # what the plain pass refuses is still refused: an interval with no closed form
    two = eo.load_scene("shadows", "rest", 2)
    renderer.set_scene_params(two, W, H)
    renderer.render()
    renderer.render_events()
    with pytest.raises(RenderError, match=r"rpt_render_particles: .*interval is 2"):
        renderer.render_particles()
    renderer.set_scene_params(scene, W, H)
    _lighting(renderer, LIT | SHADOWED)
    _pass_against_oracle(renderer, lib, scene, v, objects, LIT | SHADOWED, ps, "after interval 2")


def test_shadows_are_refused_on_an_octree_without_the_derived_layout(lib):
    """An octree whose children are not stored consecutively (tests/test_gpu_events.py's construction: a copy of the root's first child
    appended at the end, the root pointed at it) has no derived layout.  With the pear's entry of Object[] turned into a sphere the frames
    need no octree — the analytic kernels render them — and the particle launch is reached: LIT | SHADOWED is refused with RPT_ERR_STATE,
    LIT alone runs on the same context, and SHADOWED runs again once the scene as shipped is uploaded."""
    from relativitypathtracer_amd import _ffi
    from relativitypathtracer_amd.scene import OBJECT_DTYPE
    W, H = 67, 41
    camera = pc.CAMERAS["pinhole"]
    scene = dc.scene("shadows", "rest")
    oc = scene.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
    root = scene.mesh_roots()[0]
    new = np.vstack([oc, oc[oc[root, 10]][None]])
    new[root, 10] = len(oc)
    d2 = _ffi.SceneDesc.from_buffer_copy(scene.desc())
    raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
    d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
    objects = pc.scene_objects(scene, camera)
    no_mesh = objects.copy()
    typed = no_mesh.reshape(-1).view(OBJECT_DTYPE)
    assert typed["type"][dc.PEAR] == 2
    typed["type"][dc.PEAR] = 0                          # RPT_SPHERE
    ps = dc.cloud("shadows", scene, 512)
    v = _view(scene, camera, W, H, 0)
    r = Renderer(0)
    try:
        _setup(r, scene, W, H, camera, 0)
        r.upload_desc(d2)
        r.set_objects(no_mesh)
        r.set_particles(ps)
        _lighting(r, LIT | SHADOWED)
        r.render()
        r.render_events()
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_particles: RPT_PARTICLES_SHADOWED .*no derived layout") as e:
            r.render_particles()
        assert e.value.code == 2                        # RPT_ERR_STATE
        _lighting(r, LIT | AMBIENT)                     # the context is usable: a lit pass without the shadow ray, on the same scene
        _, _, _, counts, pairs = _pass_against_oracle(r, lib, scene, v, no_mesh, LIT | AMBIENT, ps, "LIT on the octree without the layout")
        assert counts[0] > 0 and pairs[0] > 0 and pairs[1] == 0
        r.upload_scene(scene)                           # the scene as shipped: the layout is there, the pear is a mesh again
        _lighting(r, LIT | SHADOWED)
        _, _, _, counts, pairs = _pass_against_oracle(r, lib, scene, v, objects, LIT | SHADOWED, ps, "SHADOWED after the real scene")
        assert pairs[0] > 0 and pairs[1] > 0
    finally:
        r.close()
