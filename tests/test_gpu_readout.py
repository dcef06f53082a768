"""rpt_render_readouts on the MI355X (DESIGN.md "Readout pass"): the device's own pre-pass framebuffer and records go through
events.readout, the numpy restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and that count.  Feeding
the reference what the device rendered isolates kernel 1110 from every other.  Scenes, cameras, sizes and displays are those of
tests/readout_cases.py, whose non-vacuity tests/test_readout_model.py asserts on the CPU.  Frames are 128 x 72 at most."""

import numpy as np
import pytest

import readout_cases as rc
from relativitypathtracer_amd import _ffi
from relativitypathtracer_amd.events import overlay, readout, readout_coverage
from relativitypathtracer_amd.renderer import RenderError, Renderer

pytestmark = pytest.mark.gpu

OUTLINES = dict(outlines=True, outline_rgba=(255, 255, 255, 200), clock_step=0.5, clock_rgba=(0, 255, 255, 160))


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    return rc.scenes()


def _setup(r, scene, W, H, camera="pinhole", ypr=None, upload=True):
    r.set_variant(0)
    r.set_msaa(1)
    r.set_adaptive_aa(1, 8)
    r.set_doppler(False, False)
    r.set_environment(None)
    r.set_debug_rgb(False)
    r.set_overlay()
    r.set_orientation(*(ypr if ypr is not None else rc.YPR if camera == "lens" else (0.0, 0.0, 0.0)))
    r.set_field_of_view(rc.LENS_V_FOV if camera == "lens" else 0.0)
    if camera == "panorama":
        r.set_projection("equirect", **rc.PANO)
    else:
        r.set_projection("pinhole")
    if upload:
        r.upload_scene(scene)
    else:
        r.set_objects(scene)
    r.set_object_windows(scene.windows())
    r.set_readouts(None)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _expected(before, records, readouts):
    """The framebuffer the pass must leave, as bytes, and the count: `before` with its RGBA replaced by the reference's."""
    rgba, count = readout(before["rgba"], records, readouts)
    want = before.copy()
    want["rgba"] = rgba.reshape(-1, 4)
    return want, count


def _same_pixels(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 16)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 16)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at pixel {k}: got {g[k].tolist()} want {w[k].tolist()}")


def _three_passes(r, readouts, what, draws=True):
    """Colour frame, event frame, readouts — each read back — against the reference.  Returns (before, records, after)."""
    r.render()
    before = r.read_framebuffer().copy()
    records = r.render_events().copy()
    r.set_readouts(readouts)
    r.render_readouts()
    after = r.read_framebuffer().copy()
    want, count = _expected(before, records, readouts)
    _same_pixels(after, want, what)
    assert r.last_readout_pixels() == count, what
    assert (count > 0) == draws, f"{what}: {count} pixels changed"
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    return before, records, after


def _correct_frame(r, readouts, what):
    """A fresh colour frame and event frame, then the pass with the setting the context HOLDS (it is not set again), against the reference."""
    r.render()
    before = r.read_framebuffer().copy()
    records = r.render_events().copy()
    r.render_readouts()
    want, count = _expected(before, records, readouts)
    _same_pixels(r.read_framebuffer(), want, what)
    assert r.last_readout_pixels() == count > 0, what


@pytest.mark.parametrize("name, camera, size", rc.CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_the_pass_equals_the_numpy_reference(renderer, scenes, name, camera, size):
    W, H = size
    scene, readouts = scenes[name]
    _setup(renderer, scene, W, H, camera)
    _, records, _ = _three_passes(renderer, readouts, f"{name} {camera} {W}x{H}")
    shown, n_in, n_on, _ = readout_coverage(records, readouts)
    assert (shown & (n_on > 0)).any() and (shown & (n_in == 0)).any() and (~shown).any()
    if name == "many":
        assert set(np.unique(records["object"][shown]).tolist()) == {66}


def test_a_turnaround_shows_one_clock_and_needs_its_windows(renderer, scenes):
    """worldline.to_dsl(readout=...): both legs carry a display of the body's proper time.  With the scene's windows each leg is there
    only for its own part of the journey; with the windows cleared both are there at once, and the frame with its displays differs."""
    W, H = 128, 72
    scene, readouts = scenes["turnaround"]
    assert scene.windows() is not None and [bool(d) for d in readouts] == [True, True, False]
    _setup(renderer, scene, W, H)
    _, records, windowed = _three_passes(renderer, readouts, "turnaround with windows")
    assert renderer.last_events_variant() >= 2000
    renderer.set_object_windows(None)
    with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_readouts: the view has changed"):
        renderer.render_readouts()                              # clearing the windows makes both frames stale
    _, records_all, unwindowed = _three_passes(renderer, readouts, "turnaround, windows cleared")
    assert renderer.last_events_variant() < 2000
    assert records.tobytes() != records_all.tobytes() and windowed.tobytes() != unwindowed.tobytes()


def test_with_the_overlay_in_both_orders(renderer, scenes):
    W, H = 67, 41
    scene, readouts = scenes["cube"]
    _setup(renderer, scene, W, H)
    renderer.render()
    before = renderer.read_framebuffer().copy()
    records = renderer.render_events().copy()
    renderer.set_overlay(**OUTLINES)
    renderer.set_readouts(readouts)
    renderer.render_overlay()
    renderer.render_readouts()
    lines_first = renderer.read_framebuffer().copy()
    rgba, n_lines = overlay(before["rgba"], records, -1, **OUTLINES)
    rgba, n_digits = readout(rgba, records, readouts)
    want = before.copy()
    want["rgba"] = rgba.reshape(-1, 4)
    _same_pixels(lines_first, want, "overlay, then readouts")
    assert renderer.last_overlay_pixels() == n_lines > 0 and renderer.last_readout_pixels() == n_digits > 0
    renderer.render()
    renderer.render_readouts()
    renderer.render_overlay()
    digits_first = renderer.read_framebuffer().copy()
    rgba, n_digits = readout(before["rgba"], records, readouts)
    rgba, n_lines = overlay(rgba, records, -1, **OUTLINES)
    want["rgba"] = rgba.reshape(-1, 4)
    _same_pixels(digits_first, want, "readouts, then overlay")
    assert renderer.last_overlay_pixels() == n_lines and renderer.last_readout_pixels() == n_digits
    assert lines_first.tobytes() != digits_first.tobytes()
    renderer.set_overlay()


def test_with_doppler_and_with_adaptive_aa(renderer, scenes):
    W, H = 128, 72
    scene, readouts = scenes["cube"]
    _setup(renderer, scene, W, H)
    renderer.render()
    plain = renderer.read_framebuffer()["rgba"].copy()
    renderer.set_doppler(True, True)
    before, _, _ = _three_passes(renderer, readouts, "cube with Doppler")
    assert not np.array_equal(before["rgba"], plain), "Doppler changed nothing: the case shows nothing"
    renderer.set_doppler(False, False)
    renderer.set_adaptive_aa(2, 8)
    _three_passes(renderer, readouts, "cube with adaptive anti-aliasing")
    assert renderer.last_aa_variant() != 0 and renderer.last_aa_refined() > 0
    renderer.set_adaptive_aa(1, 8)


def test_nothing_set_changes_no_byte_and_none_clears(renderer, scenes):
    W, H = 67, 41
    scene, readouts = scenes["cube"]
    _setup(renderer, scene, W, H)
    _three_passes(renderer, readouts, "a display first")
    assert renderer.last_readout_pixels() > 0
    before, _, after = _three_passes(renderer, None, "set_readouts(None) after a set", draws=False)
    assert after.tobytes() == before.tobytes() and renderer.last_readout_pixels() == 0
    before, _, after = _three_passes(renderer, [None, None], "no object has a display", draws=False)
    assert after.tobytes() == before.tobytes() and renderer.last_readout_pixels() == 0
    fresh = Renderer(0)
    try:
        fresh.render_readouts()                                 # nothing set: nothing is checked, not even that a scene is there
        assert fresh.last_readout_pixels() == 0
    finally:
        fresh.close()


def test_calling_it_twice_blends_twice(renderer, scenes):
    W, H = 67, 41
    scene, readouts = scenes["cube"]
    _setup(renderer, scene, W, H)
    _, records, once = _three_passes(renderer, readouts, "first pass")
    renderer.render_readouts()
    twice = renderer.read_framebuffer()
    want, count = _expected(once, records, readouts)
    _same_pixels(twice, want, "second pass over the first")
    assert renderer.last_readout_pixels() == count and not np.array_equal(twice["rgba"], once["rgba"])


def test_caller_owned_output_and_record_buffers(renderer, scenes):
    import torch
    W, H = 67, 41
    scene, readouts = scenes["cube"]
    _setup(renderer, scene, W, H)
    _, _, owned = _three_passes(renderer, readouts, "library-owned buffers")
    out = torch.zeros(W * H * 4, dtype=torch.int32, device="cuda:0")
    rec = torch.zeros(W * H * 8, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    try:
        renderer.set_output(out.data_ptr())
        renderer.set_events_output(rec.data_ptr())
        _, records, mine = _three_passes(renderer, readouts, "caller-owned buffers")
        assert mine.tobytes() == owned.tobytes()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == mine.tobytes() and rec.cpu().numpy().tobytes() == records.tobytes()
    finally:
        renderer.set_output(None)
        renderer.set_events_output(None)


def test_two_contexts_sharing_a_scene_async_equal_blocking(scenes):
    W, H = 128, 72
    scene, readouts = scenes["cube"]
    views = [(0.0, 0.0, 0.0), (0.2, 0.1, -0.2)]
    pair = [Renderer(0), Renderer(0)]
    try:
        pair[0].upload_scene(scene)
        pair[1].share_scene(pair[0])
        for r, ypr in zip(pair, views):
            _setup(r, scene, W, H, ypr=ypr, upload=False)
        pair[0].set_readouts(readouts)
        pair[0].render()
        pair[0].render_events()
        pair[1].render()
        pair[1].render_events()
        plain = pair[1].read_framebuffer().copy()
        pair[1].render_readouts()                               # the setting is per context: sharing the scene does not share it
        assert pair[1].read_framebuffer().tobytes() == plain.tobytes() and pair[1].last_readout_pixels() == 0
        blocking = [_three_passes(r, readouts, f"blocking, view {k}")[2] for k, r in enumerate(pair)]
        counts = [r.last_readout_pixels() for r in pair]
        assert blocking[0].tobytes() != blocking[1].tobytes()
        for r in pair:                                          # the three passes of both contexts enqueued before anything is waited for
            r.render_async()
            r.render_events(async_=True)
            r.render_readouts(async_=True)
        for r in pair:
            r.sync()
        for k, r in enumerate(pair):
            _same_pixels(r.read_framebuffer(), blocking[k], f"async, view {k}")
            assert r.last_readout_pixels() == counts[k]
    finally:
        for r in pair:
            r.close()


def test_refusals_leave_the_context_usable(scenes):
    W, H = 67, 41
    scene, readouts = scenes["cube"]
    r = Renderer(0)
    try:
        _setup(r, scene, W, H)
        r.set_readouts(readouts)
        assert r.last_readout_pixels() == 0
        r.render()
        for async_ in (False, True):                            # no event pass yet
            with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_readouts: no event frame"):
                r.render_readouts(async_)
        r.render_events()
        r.render_readouts()
        _correct_frame(r, readouts, "after the missing event frame")
        # the objects are handed over again: both frames are stale, then only the event frame, then none
        r.set_objects(scene)
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_readouts: the view has changed"):
            r.render_readouts()
        r.render()
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_readouts: the view has changed"):
            r.render_readouts()
        r.render_events()
        r.render_readouts()
        _correct_frame(r, readouts, "after the objects were handed over again")
        default_windows = np.array([[-np.inf, np.inf]] * len(readouts), dtype=np.float32)
        for k, change in enumerate((lambda: r.set_field_of_view(1.0), lambda: r.set_orientation(0.1, 0.0, 0.0), lambda: r.set_field_of_view(0.0), lambda: r.set_projection("equirect"),
                       lambda: r.set_scene_params(scene, W, H), lambda: r.set_object_windows(default_windows), lambda: r.set_object_windows(None))):
            change()
            with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_readouts: the view has changed"):
                r.render_readouts()
            with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_overlay: the view has changed"):
                r.set_overlay(outlines=True)
                r.render_overlay()                              # the overlay's bookkeeping is the same, time windows included
            r.set_overlay()
            _correct_frame(r, readouts, f"after view change {k}")
        _setup(r, scene, W, H)
        r.set_readouts(readouts)
        r.render()
        r.render_events()
        r.set_scene_params(scene, W + 1, H)                     # frames of another size
        r.render()
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_readouts:"):
            r.render_readouts()
        _correct_frame(r, readouts, "after frames of another size")
        # a context restricted to some rows
        _setup(r, scene, W, H)
        r.set_readouts(readouts)
        r.set_rows(0, 2, False)
        r.render()
        r.render_events()
        for async_ in (False, True):
            with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_readouts: .*rpt_set_rows"):
                r.render_readouts(async_)
        r.set_rows(0, 1, True)
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_readouts:"):
            r.render_readouts()
        r.set_rows(0, 1, False)
        _correct_frame(r, readouts, "after the restricted context")
        # a count that is not the Object[]'s
        r.set_readouts(readouts + [None])
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_readouts: 3 readouts are set, the Object\[\] holds 2"):
            r.render_readouts()
        r.set_readouts(readouts)
        _correct_frame(r, readouts, "after the wrong count")
        # bad descriptions: the call refuses and the setting made before stays, each followed by a correct frame of that setting
        good = readouts[0]
        for bad in (dict(digits=10), dict(decimals=7, digits=9), dict(decimals=3), dict(rect=(0.5, 0.2, 0.5, 0.8)), dict(rect=(0.1, 0.3, 0.9, 0.3)),
                    dict(rate=float("nan")), dict(offset=float("inf")), dict(rect=(0.1, 0.2, float("-inf"), 0.8))):
            with pytest.raises(RenderError, match=r"rpt_set_readouts failed \(1\): rpt_set_readouts:"):
                r.set_readouts([dict(good, **bad), None])
            with pytest.raises(RenderError, match=r"rpt_set_readouts failed \(1\): rpt_set_readouts: entry 1"):
                r.set_readouts([good, dict(good, **bad)])
            _correct_frame(r, readouts, f"after the refused {bad}")
        with pytest.raises(TypeError, match="digit"):           # a misspelt keyword is not silently "no display"
            r.set_readouts([dict(good, digit=4), None])
        _correct_frame(r, readouts, "after the unknown keyword")
        d = (_ffi.Readout * 2)()
        assert r._lib.rpt_set_readouts(r._h, d, -1) == 1 and r._lib.rpt_set_readouts(None, d, 2) == 1
        assert r._lib.rpt_last_readout_pixels(r._h, None) == 1 and r._lib.rpt_render_readouts(None) == 1 and r._lib.rpt_render_readouts_async(None) == 1
        # a correct frame afterwards
        _three_passes(r, readouts, "at the end")
        assert r.last_readout_pixels() > 0
    finally:
        r.close()


def test_set_objects_passes_the_scenes_readouts_on(renderer, scenes):
    W, H = 67, 41
    scene, readouts = scenes["turnaround"]
    cube, _ = scenes["cube"]
    _setup(renderer, scene, W, H)
    renderer.set_objects(scene)                                 # the scene's own `d` (and `w`) commands
    renderer.render()
    before = renderer.read_framebuffer().copy()
    records = renderer.render_events().copy()
    renderer.render_readouts()
    want, count = _expected(before, records, readouts)
    _same_pixels(renderer.read_framebuffer(), want, "the scene's displays")
    assert renderer.last_readout_pixels() == count > 0
    renderer.upload_scene(cube)                                 # a scene without `d` after one with: the displays it passed on are cleared
    renderer.set_objects(cube)
    renderer.set_scene_params(cube, W, H)
    renderer.render()
    renderer.render_events()
    renderer.render_readouts()
    assert renderer.last_readout_pixels() == 0
    renderer.set_object_windows(None)


def test_render_scene_runs_the_passes(scenes):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 67, 41
    scene, readouts = scenes["cube"]
    plain, _, records = render_scene(scene, W, H, events=True)
    drawn, _, records2 = render_scene(scene, W, H, readouts=readouts)
    assert records2.tobytes() == records.tobytes()
    want, count = _expected(plain, records, readouts)
    _same_pixels(drawn, want, "render_scene(readouts=...)")
    assert count > 0
    both, _, _ = render_scene(scene, W, H, overlay=OUTLINES, readouts=readouts)
    rgba, _ = overlay(plain["rgba"], records, -1, **OUTLINES)
    rgba, _ = readout(rgba, records, readouts)
    want["rgba"] = rgba.reshape(-1, 4)
    _same_pixels(both, want, "render_scene(overlay=..., readouts=...)")
    turn, own = scenes["turnaround"]
    plain, _, records = render_scene(turn, W, H, events=True)
    drawn, _, _ = render_scene(turn, W, H, readouts=True)      # the scene's own displays
    want, count = _expected(plain, records, own)
    _same_pixels(drawn, want, "render_scene(readouts=True)")
    assert count > 0
