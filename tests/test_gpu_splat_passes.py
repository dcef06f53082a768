"""The three splat passes on the MI355X, all on one context: the stars, the particles and the segments scatter into one fixed-point
accumulator and share one host skeleton (csrc/rpt_api.hip), so what is checked here is what only shows with all three together — the
frame and the tallies are the same whether each call blocks or all are in flight behind one sync; the measurement switches and
rpt_last_*_ms are each pass's own; a refused launch leaves the accumulator clean and the other passes' tallies alone; lit particles
change the particle pass and nothing else; the options (inverse square, depth bias) of the particles, the segments, the ballistic
records and the rockets are each pass's own.  The per-pass files hold each pass's bytes to its C oracle; nothing here restates a rule.
The case is tests/pass_tallies_case.py — the cube of tests/readout_cases.py, pinhole, 67 x 41, which is no multiple of any tile, and
its 4096 stars — with the particles just in front of surfaces and the lattice of tests/particles_cases.py's crafted set and the rods
just in front of surfaces, in the frame and in the lattice of tests/segments_cases.py's, built from the device's own records; star and particle temperatures set."""
import math

import numpy as np
import pytest

import ballistics_cases as bc
import particles_cases as pc
import pass_tallies_case as case
import segments_cases as gc
import stars_cases as sc
from relativitypathtracer_amd import rockets
from relativitypathtracer_amd.renderer import RenderError, Renderer

pytestmark = pytest.mark.gpu

W, H = case.SIZE
PASSES = ("stars", "particles", "segments")
BIAS = {}                                                # the crafted sets' depth biases, by pass: the fixture fills it
NOT_TIMED = r"failed \(2\): rpt_last_{0}_ms: the last .* pass was not timed \(rpt_set_{0}_measurement\)"      # RPT_ERR_STATE


def _kelvin(n):
    """One temperature per source, every fifth 0: that source keeps the piecewise-linear spectrum."""
    t = np.linspace(2000.0, 30000.0, n).astype(np.float32)
    t[::5] = 0.0
    return t


def _switch_on(r, sets, particle_temperatures=True):
    """Everything this file changes, as the reference run had it."""
    stars, ps, rods = sets
    r.set_scene_params(case.scene_and_readouts()[0], W, H)
    r.set_stars(stars, _kelvin(len(stars)))
    r.set_particles(ps)
    r.set_particle_temperatures(_kelvin(len(ps)) if particle_temperatures else None)
    r.set_particle_lighting()
    r.set_segments(rods)
    for name in PASSES:
        getattr(r, f"set_{name}_measurement")(False)


def _tallies(r):
    return {"stars": r.last_stars(), "particles": r.last_particles() + r.last_particle_lighting(), "segments": r.last_segments()}


def _frames(r, in_flight=False):
    if in_flight:
        r.render_async()
    else:
        r.render()
    r.render_events(async_=in_flight)


def _run(r, in_flight=False, passes=PASSES):
    """Colour, events, then `passes`: each blocking, or all enqueued and one sync.  (the framebuffer's bytes, the tallies)"""
    _frames(r, in_flight)
    for name in passes:
        getattr(r, f"render_{name}")(async_=in_flight)
    if in_flight:
        r.sync()
    return r.read_framebuffer().tobytes(), _tallies(r)


@pytest.fixture(scope="module")
def blocking():
    """(the context, (catalogue, particles, rods), the bare frame's bytes, (bytes, tallies) of the blocking run: the reference of every
    test here, computed once)"""
    scene, _ = case.scene_and_readouts()
    r = Renderer(0)
    r.set_environment_frame(scene.camera_lorentz()[1])
    sc.setup_camera(r, case.CAMERA)
    r.upload_scene(scene)
    r.set_object_windows(scene.windows())
    r.set_scene_params(scene, W, H)
    r.render()
    bare = r.read_framebuffer().tobytes()
    records = r.render_events().copy()
    objects = pc.scene_objects(scene, case.CAMERA)
    ps, groups, BIAS["particles"] = pc.crafted(records, objects, case.CAMERA, W, H, -1)
    ps = np.concatenate([ps[groups["near"]], ps[groups["lattice"]]])
    rods, groups, BIAS["segments"] = gc.crafted(records, objects, case.CAMERA, W, H, -1)
    rods = np.concatenate([rods[groups["near"]][::2], rods[groups["in frame"]], rods[groups["lattice"]]])
    print(f"{len(ps)} particles, {len(rods)} rods")
    assert 200 <= len(ps) <= 1000 and 20 <= len(rods) <= 100
    sets = (case.catalogue(), ps, rods)
    _switch_on(r, sets)
    yield r, sets, bare, _run(r)
    r.close()


def test_blocking_equals_in_flight_and_all_three_off_is_the_bare_frame(blocking):
    r, sets, bare, (frame, tallies) = blocking
    print(tallies)
    assert all(count > 0 for name in PASSES for count in tallies[name][:2])
    assert tallies["particles"][2:] == (0, 0)            # (the pairs of a lit pass: a plain one has none)
    assert frame != bare
    _switch_on(r, sets)
    got_frame, got = _run(r, True)
    assert got == tallies
    assert got_frame == frame
    for name in PASSES:
        getattr(r, f"set_{name}")(None)
    for in_flight in (False, True):
        off_frame, off = _run(r, in_flight)
        assert off_frame == bare
        assert off == {"stars": (0, 0), "particles": (0, 0, 0, 0), "segments": (0, 0)}
    _switch_on(r, sets)
    assert _run(r) == (frame, tallies)


def _last_ms(r, name):
    ms = getattr(r, f"last_{name}_ms")()
    assert len(ms) == 2 and all(math.isfinite(m) and m >= 0.0 for m in ms), (name, ms)
    return ms


def test_measurement_is_each_passes_own_and_changes_no_byte(blocking):
    r, sets, _, (frame, tallies) = blocking
    _switch_on(r, sets)
    for name in PASSES:                                  # nothing timed yet (or no longer): every call refuses
        _run(r)
        with pytest.raises(RenderError, match=NOT_TIMED.format(name)) as e:
            getattr(r, f"last_{name}_ms")()
        assert e.value.code == 2
    for name in PASSES:
        getattr(r, f"set_{name}_measurement")(True)
    for in_flight in (False, True):
        assert _run(r, in_flight) == (frame, tallies)    # a timed run and an untimed run: equal bytes, equal counts
        print({name: _last_ms(r, name) for name in PASSES})
    for only in PASSES:
        for name in PASSES:
            getattr(r, f"set_{name}_measurement")(name == only)
        assert _run(r, True) == (frame, tallies)
        for name in PASSES:
            if name == only:
                _last_ms(r, name)
            else:
                with pytest.raises(RenderError, match=NOT_TIMED.format(name)) as e:
                    getattr(r, f"last_{name}_ms")()
                assert e.value.code == 2
    # a timed pass, then the same pass switched off and rendered: no pass, so no marks of one
    for name in PASSES:
        getattr(r, f"set_{name}_measurement")(True)
    _run(r)
    for name in PASSES:
        _last_ms(r, name)
        getattr(r, f"set_{name}")(None)
        getattr(r, f"render_{name}")()
        with pytest.raises(RenderError, match=NOT_TIMED.format(name)):
            getattr(r, f"last_{name}_ms")()
        for other in PASSES[PASSES.index(name) + 1:]:    # (the passes still on keep theirs)
            _last_ms(r, other)
    _switch_on(r, sets)
    assert _run(r) == (frame, tallies)


def test_no_refused_launch_leaves_a_mark_behind(blocking):
    r, sets, _, (frame, tallies) = blocking
    stars, ps, rods = sets
    scene, _ = case.scene_and_readouts()
    n = len(pc.scene_objects(scene, case.CAMERA))

    def refused(name, words, in_flight=False):
        """A fresh pair of frames, the two other passes, then the refused one: RPT_ERR_ARG, and the other two tallies as they were.  (Not
        as the reference has them: what a pass changes depends on the passes before it, and one is missing here.)"""
        others = tuple(p for p in PASSES if p != name)
        _, before = _run(r, in_flight, others)
        assert all(count > 0 for p in others for count in before[p][:2])
        with pytest.raises(RenderError, match=rf"failed \(1\): rpt_render_{name}: .*{words}") as e:
            getattr(r, f"render_{name}")(async_=in_flight)
        assert e.value.code == 1
        r.sync()
        after = _tallies(r)
        assert all(after[p] == before[p] for p in others)

    def accepted():
        """The next accepted passes give the reference's bytes: the refused one left nothing in the accumulator, blocking or in flight."""
        _switch_on(r, sets)
        assert _run(r) == (frame, tallies)
        assert _run(r, True) == (frame, tallies)

    _switch_on(r, sets)
    # an interval the light cone has no closed form for: the particles and the segments refuse (the stars do not ask)
    for name in ("particles", "segments"):
        for in_flight in (False, True):
            r.set_params(scene.params["white_point"], scene.params["ambient"], W, H, 2)
            _frames(r, in_flight)
            with pytest.raises(RenderError, match=rf"failed \(1\): rpt_render_{name}: interval is 2"):
                getattr(r, f"render_{name}")(async_=in_flight)
            r.sync()
            accepted()
    # a set that names an object beyond Object[]
    beyond = ps.copy()
    beyond["object"][5] = n
    r.set_particles(beyond)
    refused("particles", rf"names object {n}, the Object\[\] holds {n}")
    accepted()
    beyond = rods.copy()
    beyond["object"][3] = n + 1
    r.set_segments(beyond)
    refused("segments", rf"names object {n + 1}, the Object\[\] holds {n}", in_flight=True)
    accepted()
    # temperatures whose count is not the set's
    r.set_star_temperatures(_kelvin(len(stars) - 1))
    refused("stars", rf"{len(stars) - 1} temperatures are set \(rpt_set_star_temperatures\), the catalogue holds {len(stars)}")
    accepted()
    r.set_particle_temperatures(_kelvin(len(ps) + 1))
    refused("particles", rf"{len(ps) + 1} temperatures are set \(rpt_set_particle_temperatures\), the set holds {len(ps)}", in_flight=True)
    accepted()
    # lit particles with temperatures set: the lit pass's own refusal
    r.set_particle_lighting(lit=True)
    refused("particles", "RPT_PARTICLES_LIT with particle temperatures set")
    accepted()


def test_lighting_changes_the_particle_words_only(blocking):
    r, sets, _, _ = blocking
    _switch_on(r, sets, particle_temperatures=False)     # (a lit pass refuses temperatures)
    def alone(name, in_flight=False):
        """(bytes, its tally) of one pass on a fresh pair of frames: its share of the frame"""
        got_frame, got = _run(r, in_flight, (name,))
        return got_frame, got[name]

    shares = {name: alone(name) for name in ("stars", "segments")}
    plain_frame, plain = _run(r)
    assert plain["particles"][0] > 0 and plain["particles"][1] > 0
    r.set_particle_lighting(lit=True)
    for in_flight in (False, True):
        lit_frame, lit = _run(r, in_flight)
        print(plain, lit)
        # the scene has no light: a grain that is seen is still seen, and scatters nothing
        assert lit["particles"] != plain["particles"] and lit["particles"][0] == plain["particles"][0]
        assert lit["stars"] == plain["stars"] and lit_frame != plain_frame
        # (the rods are drawn over what the particles left, so their changed pixels are compared alone, as the stars' are)
        for name in ("stars", "segments"):
            assert alone(name, in_flight) == shares[name]
    r.set_particle_lighting()
    assert _run(r) == (plain_frame, plain)


OPTION_SETTERS = {"particles": "set_particle_options", "segments": "set_segment_options", "ballistics": "set_ballistic_options", "rockets": "set_rocket_options"}


def test_the_options_are_each_passes_own(blocking):
    """The four passes with options (inverse square, depth bias) keep them in one array of the context: a pass's pair moves its own
    frame and no other's.  The ballistic records are the fixture's particles at rest in their objects' frames, the rockets those without
    an acceleration; every pass is rendered alone on a fresh pair of frames, so its bytes and its tally are its share."""
    r, sets, _, (frame, tallies) = blocking
    _switch_on(r, sets)
    records = bc.from_particles(sets[1])
    r.set_ballistics(records)
    r.set_rockets(rockets.from_ballistics(records))
    names = tuple(OPTION_SETTERS)
    default = (False, 0.0)
    crafted = {name: (True, BIAS["segments" if name == "segments" else "particles"]) for name in names}
    assert all(bias > 0.0 for _, bias in crafted.values())

    def set_options(pairs):
        for name in names:
            getattr(r, OPTION_SETTERS[name])(*pairs[name])

    def alone(name):
        _frames(r)
        getattr(r, f"render_{name}")()
        return r.read_framebuffer().tobytes(), getattr(r, f"last_{name}")()

    set_options(dict.fromkeys(names, default))
    plain = {name: alone(name) for name in names}
    kept = {}
    for name in names:                                   # one pass with the crafted pair, the other three at their defaults
        set_options({**dict.fromkeys(names, default), name: crafted[name]})
        kept[name] = alone(name)
        print(name, crafted[name], plain[name][1], kept[name][1])
        assert plain[name][1][0] > 0 and kept[name][0] != plain[name][0]      # (not a dead option)
    for turn, name in enumerate(names):                  # four different pairs at once, this pass's the crafted one
        bias = crafted[name][1]
        others = [(False, 2.0 * bias), (True, 0.0), (False, 0.5 * bias)]
        rest = [n for n in names if n != name]
        set_options({name: crafted[name], **{n: others[(k + turn) % 3] for k, n in enumerate(rest)}})
        assert alone(name) == kept[name]
    set_options(crafted)                                 # every pass its crafted pair: each as it was with the others at their defaults
    for name in names:
        assert alone(name) == kept[name]
    for name in names:                                   # one pass back to its default: its default frame, the other three unmoved
        set_options({**crafted, name: default})
        for other in names:
            assert alone(other) == (plain if other == name else kept)[other], (name, other)
    set_options(dict.fromkeys(names, default))
    r.set_ballistics(None)
    r.set_rockets(None)
    assert _run(r) == (frame, tallies)
