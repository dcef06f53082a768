"""The passes' counters on the MI355X, all at once on one context: the refined pixels of an adaptive frame, the overlay's and the
readouts' changed pixels and the stars' two counts come home through one mechanism (csrc/rpt_api.hip, Tally), so what is checked here is
that no pass reads another's: every number above zero and the same whether each call blocks or all are in flight behind one sync; one
pass switched off reads zero and leaves the other three; a second context leaves the first's alone.  The case is
tests/pass_tallies_case.py — the cube of tests/readout_cases.py, pinhole, 67 x 41, which is no multiple of the 64 x 8 tile either way —,
whose five numbers tests/test_pass_tallies_model.py shows to be above zero by the CPU models.  The frame passes do not refuse a context
with adaptive anti-aliasing on, so the refined count shares the frame with the other three."""
import pytest

import pass_tallies_case as case
import stars_cases as sc
from relativitypathtracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

NAMES = ("refined", "overlay", "readouts", "stars")


def _context(scene):
    W, H = case.SIZE
    r = Renderer(0)
    r.set_environment_frame(scene.camera_lorentz()[1])
    sc.setup_camera(r, case.CAMERA)
    r.upload_scene(scene)
    r.set_object_windows(scene.windows())
    r.set_scene_params(scene, W, H)
    return r


def _switch_on(r, readouts, overlay=case.OVERLAY):
    r.set_adaptive_aa(*case.AA)
    r.set_overlay(**overlay)
    r.set_readouts(readouts)
    r.set_stars(case.catalogue())


def _tallies(r):
    return {"refined": r.last_aa_refined(), "overlay": r.last_overlay_pixels(), "readouts": r.last_readout_pixels(), "stars": r.last_stars()}


def _run(r, in_flight):
    """Colour, events, overlay, readouts, stars: each blocking, or all enqueued and one sync.  (the framebuffer's bytes, the tallies)"""
    if in_flight:
        r.render_async()
    else:
        r.render()
    for call in (r.render_events, r.render_overlay, r.render_readouts, r.render_stars):
        call(async_=in_flight)
    if in_flight:
        r.sync()
    return r.read_framebuffer().tobytes(), _tallies(r)


@pytest.fixture(scope="module")
def blocking():
    """(the context, its readouts, (bytes, tallies) of the blocking run: the reference of every test here, computed once)"""
    scene, readouts = case.scene_and_readouts()
    r = _context(scene)
    _switch_on(r, readouts)
    yield r, readouts, _run(r, False)
    r.close()


def test_every_tally_counts_something(blocking):
    _, _, (_, tallies) = blocking
    print(tallies)
    assert tallies["refined"] > 0 and tallies["overlay"] > 0 and tallies["readouts"] > 0 and tallies["stars"][0] > 0 and tallies["stars"][1] > 0


def test_in_flight_reads_what_blocking_read(blocking):
    r, readouts, (frame, tallies) = blocking
    _switch_on(r, readouts)
    got_frame, got = _run(r, True)
    assert got == tallies
    assert got_frame == frame


@pytest.mark.parametrize("off", NAMES)
def test_one_pass_switched_off_reads_zero_and_leaves_the_others(blocking, off):
    r, readouts, (_, tallies) = blocking
    _switch_on(r, readouts)
    assert _run(r, False)[1] == tallies
    if off == "refined":
        r.set_adaptive_aa(1)
        r.render()
    elif off == "overlay":
        r.set_overlay()
        r.render_overlay()
    elif off == "readouts":
        r.set_readouts(None)
        r.render_readouts()
    else:
        r.set_stars(None)
        r.render_stars()
    assert _tallies(r) == dict(tallies, **{off: (0, 0) if off == "stars" else 0})


def test_a_second_context_leaves_the_firsts_tallies(blocking):
    r, readouts, (_, tallies) = blocking
    _switch_on(r, readouts)
    assert _run(r, False)[1] == tallies
    scene, _ = case.scene_and_readouts()
    other = _context(scene)
    try:
        _switch_on(other, readouts, case.OTHER_OVERLAY)
        theirs = _run(other, False)[1]
    finally:
        other.close()
    assert theirs["overlay"] not in (0, tallies["overlay"])      # (a tint colours every hit pixel: another count than the lines')
    assert _tallies(r) == tallies
