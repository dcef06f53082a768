"""rpt_render_overlay on the MI355X (DESIGN.md "Overlay pass"): the device's own pre-overlay framebuffer and records go through
events.overlay, the numpy restatement of the rules, and the pass must give those bytes — all 16 of every pixel — and that count.  Feeding
the reference what the device rendered isolates the overlay kernels from every other.  Scenes, cameras, sizes and layer settings are those
of tests/overlay_cases.py, whose non-vacuity tests/test_overlay_model.py asserts on the CPU.  Frames are 128 x 72 at most."""
import ctypes as C

import numpy as np
import pytest

import events_oracle as eo
import overlay_cases as oc
from relativitypathtracer_amd import _ffi
from relativitypathtracer_amd.events import overlay
from relativitypathtracer_amd.renderer import RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def _setup(r, scene, W, H, camera="pinhole", ypr=None, upload=True):
    r.set_variant(0)
    r.set_msaa(1)
    r.set_adaptive_aa(1, 8)
    r.set_doppler(False, False)
    r.set_environment(None)
    r.set_debug_rgb(False)
    r.set_orientation(*(ypr if ypr is not None else oc.YPR if camera == "lens" else (0.0, 0.0, 0.0)))
    r.set_field_of_view(oc.LENS_V_FOV if camera == "lens" else 0.0)
    if camera == "panorama":
        r.set_projection("equirect", **oc.PANO)
    else:
        r.set_projection("pinhole")
    if upload:
        r.upload_scene(scene)
    else:
        r.set_objects(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)


def _expected(before, records, interval, kw):
    """The framebuffer the pass must leave, as bytes, and the count: `before` with its RGBA replaced by the reference's."""
    rgba, count = overlay(before["rgba"], records, interval, **kw)
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


def _three_passes(r, interval, kw, what):
    """Colour frame, event frame, overlay — each read back — against the reference.  Returns (before, records, after)."""
    r.render()
    before = r.read_framebuffer().copy()
    records = r.render_events().copy()
    r.set_overlay(**kw)
    r.render_overlay()
    after = r.read_framebuffer().copy()
    want, count = _expected(before, records, interval, kw)
    _same_pixels(after, want, what)
    assert r.last_overlay_pixels() == count, what
    assert r.read_events().tobytes() == records.tobytes(), f"{what}: the pass wrote the record buffer"
    for untouched in ("x", "y", "unspecified"):
        assert np.array_equal(after[untouched].view(np.uint32), before[untouched].view(np.uint32)), f"{what}: bytes outside RGBA changed"
    assert np.array_equal(after["rgba"][:, 3], before["rgba"][:, 3]), f"{what}: alpha changed"
    return before, records, after


@pytest.mark.parametrize("size", oc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", oc.CAMERAS)
@pytest.mark.parametrize("name", oc.SCENES)
def test_the_pass_equals_the_numpy_reference(renderer, name, camera, size):
    W, H = size
    scene = eo.load_scene(name, "rest", -1)
    _setup(renderer, scene, W, H, camera)
    for layer, kw in oc.layer_settings(name).items():           # each layer alone, then all five together
        before, records, after = _three_passes(renderer, -1, kw, f"{name} {camera} {W}x{H} {layer}")
        hit = records["object"] >= 0
        assert hit.any() and (~hit).any()
        assert oc.marked(before["rgba"], after["rgba"]).any(), f"{layer} drew nothing"


def test_the_frames_own_largest_delay_equals_passing_it(renderer):
    W, H = 67, 41
    scene = eo.load_scene("ladder_paradox", "rest", -1)
    _setup(renderer, scene, W, H)
    _, records, auto = _three_passes(renderer, -1, dict(tint=True, tint_t_max=0.0, tint_alpha=200), "tint, the frame's range")
    hit = records["object"] >= 0
    top = float(np.abs(np.float32(-1) * records["dist"][hit]).max())
    _, _, explicit = _three_passes(renderer, -1, dict(tint=True, tint_t_max=top, tint_alpha=200), "tint, the same range passed")
    assert auto.tobytes() == explicit.tobytes()
    # light delay off: every delay is 0, so is the largest, and every hit pixel gets the ramp's first knot
    scene0 = eo.load_scene("ladder_paradox", "rest", 0)
    _setup(renderer, scene0, W, H)
    _, records, after = _three_passes(renderer, 0, dict(tint=True, tint_alpha=255), "tint with light delay off")
    assert (after["rgba"].reshape(H, W, 4)[records["object"] >= 0][:, :3] == (255, 64, 64)).all()


def test_with_doppler_and_with_adaptive_aa(renderer):
    W, H = 128, 72
    scene = eo.load_scene("arch", "0.9c", -1)
    _setup(renderer, scene, W, H)
    renderer.render()
    plain = renderer.read_framebuffer()["rgba"].copy()
    renderer.set_doppler(True, True)
    before, _, _ = _three_passes(renderer, -1, oc.layer_settings("arch")["all"], "arch 0.9c with Doppler")
    assert not np.array_equal(before["rgba"], plain), "Doppler changed nothing: the case shows nothing"
    assert renderer.last_variant() in (241, 243, 244)
    renderer.set_doppler(False, False)
    scene = eo.load_scene("rulers", "rest", -1)
    _setup(renderer, scene, W, H)
    renderer.set_adaptive_aa(2, 8)
    _three_passes(renderer, -1, oc.layer_settings("rulers")["all"], "rulers with adaptive anti-aliasing")
    assert renderer.last_aa_variant() != 0 and renderer.last_aa_refined() > 0
    renderer.set_adaptive_aa(1, 8)


def test_no_layer_changes_no_byte(renderer):
    W, H = 67, 41
    scene = eo.load_scene("shadows", "rest", -1)
    _setup(renderer, scene, W, H)
    _three_passes(renderer, -1, oc.layer_settings("shadows")["all"], "all layers first")
    assert renderer.last_overlay_pixels() > 0
    before, _, after = _three_passes(renderer, -1, {}, "no layer")
    assert after.tobytes() == before.tobytes() and renderer.last_overlay_pixels() == 0


def test_calling_it_twice_blends_twice(renderer):
    W, H = 67, 41
    scene = eo.load_scene("rulers", "rest", -1)
    _setup(renderer, scene, W, H)
    kw = dict(outlines=True, outline_rgba=(255, 255, 255, 128))
    _, records, once = _three_passes(renderer, -1, kw, "first pass")
    renderer.render_overlay()
    twice = renderer.read_framebuffer()
    want, count = _expected(once, records, -1, kw)
    _same_pixels(twice, want, "second pass over the first")
    assert renderer.last_overlay_pixels() == count and not np.array_equal(twice["rgba"], once["rgba"])


def test_caller_owned_output_and_record_buffers(renderer):
    import torch
    W, H = 67, 41
    scene = eo.load_scene("arch", "rest", -1)
    _setup(renderer, scene, W, H)
    kw = oc.layer_settings("arch")["all"]
    _, _, owned = _three_passes(renderer, -1, kw, "library-owned buffers")
    out = torch.zeros(W * H * 4, dtype=torch.int32, device="cuda:0")
    rec = torch.zeros(W * H * 8, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    try:
        renderer.set_output(out.data_ptr())
        renderer.set_events_output(rec.data_ptr())
        _, records, mine = _three_passes(renderer, -1, kw, "caller-owned buffers")
        assert mine.tobytes() == owned.tobytes()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == mine.tobytes() and rec.cpu().numpy().tobytes() == records.tobytes()
    finally:
        renderer.set_output(None)
        renderer.set_events_output(None)


def test_two_contexts_sharing_a_scene_async_equal_blocking():
    W, H = 128, 72
    scene = eo.load_scene("shadows", "rest", -1)
    kw = oc.layer_settings("shadows")["all"]
    views = [(0.0, 0.0, 0.0), (0.3, 0.1, -0.2)]
    pair = [Renderer(0), Renderer(0)]
    try:
        pair[0].upload_scene(scene)
        pair[1].share_scene(pair[0])
        for r, ypr in zip(pair, views):
            _setup(r, scene, W, H, ypr=ypr, upload=False)
        blocking = [_three_passes(r, -1, kw, f"blocking, view {k}")[2] for k, r in enumerate(pair)]
        counts = [r.last_overlay_pixels() for r in pair]
        assert blocking[0].tobytes() != blocking[1].tobytes()
        for r in pair:                                  # the three passes of both contexts enqueued before anything is waited for
            r.render_async()
            r.render_events(async_=True)
            r.render_overlay(async_=True)
        for r in pair:
            r.sync()
        for k, r in enumerate(pair):
            _same_pixels(r.read_framebuffer(), blocking[k], f"async, view {k}")
            assert r.last_overlay_pixels() == counts[k]
    finally:
        for r in pair:
            r.close()


def test_refusals_leave_the_context_usable():
    W, H = 67, 41
    scene = eo.load_scene("rulers", "rest", -1)
    kw = oc.layer_settings("rulers")["all"]
    r = Renderer(0)
    try:
        _setup(r, scene, W, H)
        r.set_overlay(**kw)
        assert r.last_overlay_pixels() == 0
        r.render()
        for async_ in (False, True):                    # no event pass yet
            with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_overlay: no event frame"):
                r.render_overlay(async_)
        r.render_events()
        r.render_overlay()
        # the objects are handed over again: both frames are stale, then only the event frame, then none
        r.set_objects(scene)
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_overlay: the view has changed"):
            r.render_overlay()
        r.render()
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_overlay: the view has changed"):
            r.render_overlay()
        r.render_events()
        r.render_overlay()
        for change in (lambda: r.set_field_of_view(1.0), lambda: r.set_orientation(0.1, 0.0, 0.0), lambda: r.set_projection("equirect"),
                       lambda: r.set_scene_params(scene, W, H)):
            change()
            with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_overlay: the view has changed"):
                r.render_overlay()
        _setup(r, scene, W, H)
        r.render()
        r.render_events()
        r.set_scene_params(scene, W + 1, H)             # frames of another size
        r.render()
        with pytest.raises(RenderError, match=r"failed \(2\): rpt_render_overlay:"):
            r.render_overlay()
        # a context restricted to some rows
        _setup(r, scene, W, H)
        r.set_rows(0, 2, False)
        r.render()
        r.render_events()
        for async_ in (False, True):
            with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_overlay: .*rpt_set_rows"):
                r.render_overlay(async_)
        r.set_rows(0, 1, True)
        with pytest.raises(RenderError, match=r"failed \(1\): rpt_render_overlay:"):
            r.render_overlay()
        r.set_rows(0, 1, False)
        # bad descriptions: the call refuses and the description set before stays
        for bad in (dict(delay_step=-1.0), dict(clock_step=0.0), dict(clock_step=float("nan")), dict(lattice_step=(0.0, 0.0, 0.0)),
                    dict(lattice_step=(1.0, float("inf"), 0.0)), dict(tint=True, tint_t_max=-2.0)):
            with pytest.raises(RenderError, match=r"rpt_set_overlay failed \(1\): rpt_set_overlay:"):
                r.set_overlay(**bad)
        d = _ffi.OverlayDesc()
        d.layers = 32
        assert r._lib.rpt_set_overlay(r._h, C.byref(d)) == 1 and r._lib.rpt_last_error(r._h).decode().startswith("rpt_set_overlay: unknown layer bits")
        assert r._lib.rpt_last_overlay_pixels(r._h, None) == 1 and r._lib.rpt_render_overlay(None) == 1
        # a correct frame afterwards
        _three_passes(r, -1, kw, "after the refusals")
        assert r.last_overlay_pixels() > 0
    finally:
        r.close()


def test_render_scene_runs_the_three_passes():
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 67, 41
    scene = eo.load_scene("rulers", "rest", -1)
    kw = oc.layer_settings("rulers")["all"]
    plain, _, records = render_scene(scene, W, H, events=True)
    drawn, _, records2 = render_scene(scene, W, H, overlay=kw)
    assert records2.tobytes() == records.tobytes()
    want, count = _expected(plain, records, -1, kw)
    _same_pixels(drawn, want, "render_scene(overlay=...)")
    assert count > 0
