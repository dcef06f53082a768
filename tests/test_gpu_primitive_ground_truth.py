"""The device's own event records (rpt_render_events) and its debug RGB plane against the float64 model of tests/primitive_truth.py
 — directly, not through the oracle: the same assertions, constants and caps as
tests/test_primitive_ground_truth.py, imported from it and not re-measured.  Every kernel form reads the model's verdict: the pinhole in
every variant tests/test_gpu_parity.py runs (culled and un-culled), a lens below and above 90 degrees, an orientation, the panorama, a
fisheye ray map, the blocking and the in-flight form, the windowed kernels (colour and events).  Textured and mesh hits carry a colour
too: the `textured` cases, a textured scene with a textured mesh through every camera form, and the texture fetch at each of its three
places in the kernels' source.  Doppler, the sky, MSAA and adaptive anti-aliasing stay off.  The model's frames are computed once per
case and shared with nothing re-derived here."""
import math

import numpy as np
import pytest

import events_oracle as eo
import primitive_cases as pc
import primitive_truth as pt
import raymap_cases as rc
import test_primitive_ground_truth as truth
import window_oracle as wo
from relativitypathtracer_amd.renderer import Renderer, orient_objects, raymap

pytestmark = pytest.mark.gpu

PARITY_VARIANTS = (0, 1, 3, 41, 43, 44)          # tests/test_gpu_parity.py's VARIANTS
YPR = (0.4, -0.25, 0.15)
PANO = dict(h_fov=2.0, v_fov=1.2, yaw=0.3)
LENS60, LENS100 = 60.0 * math.pi / 180.0, 100.0 * math.pi / 180.0


@pytest.fixture(scope="module")
def wlib(tmp_path_factory):
    return wo.build_library(tmp_path_factory.mktemp("gpu_primitive_truth"))


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.set_object_windows(None)
    r.close()


def _setup(r, scene, W, H, v_fov=0.0, pano=None, ray_map=None, ypr=(0.0, 0.0, 0.0), windows=None):
    r.set_variant(0)
    r.set_msaa(1)
    r.set_adaptive_aa(1)
    r.set_debug_doppler(False)
    r.set_doppler(False, False)
    r.set_environment(None)
    r.set_environment_frame(None)
    r.set_orientation(*ypr)
    r.set_field_of_view(v_fov)
    if pano is not None:
        r.set_projection("equirect", **pano)
    elif ray_map is not None:
        r.set_raymap(ray_map)
        r.set_projection("raymap")
    else:
        r.set_projection("pinhole")
    r.set_object_windows(windows)
    r.upload_scene(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_events_output(None)
    r.set_debug_rgb(True)


def _reset(r):
    r.set_variant(0)
    r.set_object_windows(None)
    r.set_orientation(0.0, 0.0, 0.0)
    r.set_field_of_view(0.0)
    r.set_projection("pinhole")


def _check_forms(r, label, model, objs, colour_variants, mask=None):
    """Every form of the context's current state against the model: the colour frame through `colour_variants`, blocking, and the
    default choice in flight; the records through the default choice and the un-culled form, blocking and in flight.  A form whose
    output equals, bit for bit, one that was already checked is not compared a second time."""
    if mask is not None:
        model = pt.subset(model, mask)
    seen_rgb, seen_rec = [], []

    def take(rgb, rec, what):
        rgb = None if rgb is None else np.ascontiguousarray(rgb).reshape(-1, 3)
        rec = np.ascontiguousarray(rec).reshape(-1)
        if mask is not None:
            rgb, rec = (None if rgb is None else rgb[mask]), rec[mask]
        new_rgb = rgb is not None and not any(np.array_equal(rgb.view(np.uint32), s.view(np.uint32)) for s in seen_rgb)
        new_rec = not any(rec.tobytes() == s.tobytes() for s in seen_rec)
        if new_rgb or new_rec:
            truth.check_frame(f"{label} {what}", model, objs, rec, rgb if new_rgb else None, caps=mask is None)
            if new_rgb:
                seen_rgb.append(rgb)
            if new_rec:
                seen_rec.append(rec)

    r.set_variant(0)
    rec0 = r.render_events().copy()
    kernels = set()
    for variant in colour_variants:
        r.set_variant(variant)
        r.render()
        kernels.add(r.last_variant())
        take(r.read_debug_rgb().copy(), rec0, f"colour variant {variant} kernel {r.last_variant()} blocking")
    r.set_variant(0)
    r.render_async()
    r.sync()
    take(r.read_debug_rgb().copy(), rec0, f"colour kernel {r.last_variant()} in flight")
    for variant in (0, 3):
        r.set_variant(variant)
        take(None, r.render_events().copy(), f"events variant {variant} kernel {r.last_events_variant()} blocking")
        assert r.render_events(async_=True) is None
        r.sync()
        take(None, r.read_events().copy(), f"events variant {variant} kernel {r.last_events_variant()} in flight")
    r.set_variant(0)
    assert len(seen_rgb) >= 1 and len(seen_rec) >= 1
    return kernels


# ---- 1. every committed case: the pinhole (or its lens), culled and un-culled, blocking and in flight, windowed where the case has windows
@pytest.mark.parametrize("name", pc.case_ids())
def test_device_agrees_with_the_model_on_every_case(renderer, wlib, name):
    scene, W, H, dirs, windows, model = truth.case_model(name, wlib)
    v_fov = truth._CASES[name][6]
    _setup(renderer, scene, W, H, v_fov=0.0 if v_fov is None else v_fov, windows=windows)
    plain = v_fov is None and windows is None
    kernels = _check_forms(renderer, name, model, scene.objects(), PARITY_VARIANTS if plain else (0, 3))
    if windows is not None:
        assert all(k >= 2000 for k in kernels), (name, "the windowed kernels did not run", kernels)
        renderer.render_events()
        assert renderer.last_events_variant() >= 2000
    _reset(renderer)


# ---- 2. the other cameras -------------------------------------------------------------------------------------------------------------------
def _five(camera="rest", interval=-1):
    return pc._text(pc.FIVE, camera, interval, t=2.0)


CAMERA_FORMS = ("lens60", "lens100", "turned", "panorama", "fisheye")


def _through_a_camera(renderer, wlib, scene, W, H, label, form, camera, windowed, flip=False):
    objs, mask, view = scene.objects(), None, {}
    if form in ("lens60", "lens100"):
        v = LENS60 if form == "lens60" else LENS100
        view, dirs = dict(v_fov=v), eo.pinhole_dirs(W, H, eo.lens_scale(v))
    elif form == "turned":
        view, dirs = dict(ypr=YPR), eo.pinhole_dirs(W, H)
        objs = np.ascontiguousarray(orient_objects(scene, *YPR)).view(np.uint8).reshape(-1).view(objs.dtype)
    elif form == "panorama":
        view, dirs = dict(pano=PANO), eo.pano_dirs(W, H, **PANO)
    else:
        m = raymap("fisheye", W, H, fov=math.pi, fit=0)
        view, dirs, mask = dict(ray_map=m), rc.oracle_dirs(m), rc.has_ray(m)
    windows = None
    if windowed:
        windows = wo.choose_windows(wlib, scene, W, H, dirs=dirs, objects=None if form != "turned" else objs, flip=flip)
        assert np.isfinite(windows).any()
    model = truth.model_frame(scene, objs, dirs, windows)
    assert int((model["object"][mask if mask is not None else slice(None)] >= 0).sum()) >= pc.MIN_HIT_PIXELS
    _setup(renderer, scene, W, H, windows=windows, **view)
    kernels = _check_forms(renderer, f"{label} {camera} {form}{' windowed' if windowed else ''}", model, objs, (0, 3), mask=mask)
    assert all((k >= 2000) == windowed for k in kernels), kernels
    _reset(renderer)


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("camera", ["rest", "oblique"])
@pytest.mark.parametrize("form", CAMERA_FORMS)
def test_device_agrees_with_the_model_through_every_camera(renderer, wlib, form, camera, windowed):
    _through_a_camera(renderer, wlib, _five(camera), 128, 72, "five", form, camera, windowed)


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("camera", ["rest", "oblique"])
@pytest.mark.parametrize("form", CAMERA_FORMS)
def test_device_agrees_with_the_model_on_a_textured_scene_through_every_camera(renderer, wlib, form, camera, windowed):
    """primitive_cases.TEX_FORMS — the five-object scene with its floor textured by the 3 x 5 and its cube by the noise, and the pear added,
    textured by the 5 x 3 — at 64 x 36 (the pear is brute-forced).  The panorama's windows are chosen in the other alternation: at rest the
    first leaves 83 % of its 750 hit pixels well-conditioned for colours at this size, the other 92 % (chosen on the CPU oracle)."""
    _through_a_camera(renderer, wlib, pc.textured_forms_scene(camera), 64, 36, "textured", form, camera, windowed, flip=(form == "panorama"))


# ---- 3. the texture fetch at each of its places in the source ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diag_renderer():
    r = Renderer(0, diag=True)
    yield r
    r.close()


def test_every_texture_fetch_in_the_source_is_reached(renderer, diag_renderer, wlib):
    """`sample_texture` is called at three places: in `trace` (rpt_kernels.hip.h), which every product kernel shades through — reached by
    kernels 1, 3, 41 and 43 here, as by the cases and camera forms above; in `shade_uniform` (rpt_persistent.hip.h), the shading of the
    persistent-workgroup kernels — reached by kernel 60; and in `render_strip_queued` (rpt_persistent.hip.h), the ray-queue kernel —
    reached by kernel 61.  60 and 61 are measurement arms of the diagnostic library (tests/test_gpu_diag_arms.py), plain pinhole only:
    each renders the textured scene at rest, and its float RGB is held to the model like any other form (the records are the product's)."""
    W, H = 64, 36
    scene = pc.textured_forms_scene("rest")
    objs = scene.objects()
    model = truth.model_frame(scene, objs, eo.pinhole_dirs(W, H))
    _setup(renderer, scene, W, H)
    product = _check_forms(renderer, "textured rest pinhole", model, objs, (1, 3, 41, 43))
    rec = renderer.render_events().copy()
    _reset(renderer)
    assert product and not product & {60, 61}, product
    r, reached = diag_renderer, set()
    for variant in (60, 61):
        r.set_variant(variant)
        r.upload_scene(scene)
        r.set_scene_params(scene, W, H)
        r.set_rows(0, 1, False)
        r.set_output(None)
        r.set_debug_rgb(True)
        r.render()
        assert r.last_variant() == variant
        reached.add(r.last_variant())
        truth.check_frame(f"textured rest pinhole kernel {variant}", model, objs, rec.reshape(-1), r.read_debug_rgb().copy().reshape(-1, 3))
    assert reached == {60, 61}, reached
