"""The device's sky pixels — debug RGB and packed bytes — against the float64 model of tests/sky_truth.py (DESIGN.md "Environment map",
"What pins it besides the restatement"): directly, not through the oracle, with the bound and the constants of sky_truth and the
assertions and caps of tests/test_sky_ground_truth.py, imported and not measured again.  Every case of tests/sky_cases.py runs through
every form the context offers for it: the pinhole's sky kernels by set_variant (603, 641, 643, 644, and on a scene outside the exact
reciprocal's domain the IEEE forms of 641 and 643), the panorama's (703, 741 + IEEE form, 744), the lens's and the turned head's (823, 861,
863, 864; E handed over un-turned), the ray map's (1223, 1261 + IEEE form, 1264), the windowed ones on `cubes`, blocking and in flight.
Which pixels are sky is the model's verdict (primitive_truth), never the device's; a pixel the model calls a clear hit must equal the
frame without the sky.  rpt_probe which = 7 is held to the model at the crafted directions.

The kernels reached are held against the `sky` entries of the kernel-choice record (tests/golden/kernel_choice.json through
tests/kernel_choice_cases.py), so that a sky kernel added there cannot go unseen here.  That record drives the pinhole, the lens and the
panorama; the ray map and the windows are not among its axes, so their numbers are listed here by hand (RAYMAP_SKY, WINDOWED_SKY).  The
windowed walk forms (2641, 2741, 3261) are not reached: the windowed cases are `cubes`, which has no mesh."""
import itertools
import json
import os

import numpy as np
import pytest

import kernel_choice_cases as kc
import sky_cases as sc
import test_sky_ground_truth as truth
import window_oracle as wo
from relativitypathtracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_choice.json")
RAYMAP_SKY = {(1223, False), (1261, True), (1261, False), (1264, False)}          # (rpt_last_variant, rpt_last_exact_rcp)
WINDOWED_SKY = {(2603, False), (2644, False), (2703, False), (2744, False), (3223, False), (3264, False)}
_REACHED, _RAN = set(), set()


@pytest.fixture(scope="module")
def wlib(tmp_path_factory):
    return wo.build_library(tmp_path_factory.mktemp("gpu_sky_truth"))


@pytest.fixture(scope="module")
def huge_obj(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_sky_truth_obj") / "huge.obj")
    with open(path, "w") as f:
        f.write(kc.HUGE_OBJ)
    return path


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    _reset(r)
    r.close()


def _setup(r, scene, W, H, v_fov=0.0, pano=None, ray_map=None, ypr=(0.0, 0.0, 0.0), windows=None):
    """tests/test_gpu_primitive_ground_truth.py's _setup; the sky and Doppler are set by the caller."""
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
    r.set_doppler(False, False)
    r.set_environment(None)
    r.set_environment_frame(None)
    r.set_object_windows(None)
    r.set_orientation(0.0, 0.0, 0.0)
    r.set_field_of_view(0.0)
    r.set_projection("pinhole")


def _frame(r, in_flight=False):
    if in_flight:
        r.render_async()
        r.sync()
    else:
        r.render()
    return r.read_framebuffer()["rgba"].reshape(-1, 4).copy(), r.read_debug_rgb().reshape(-1, 3).copy()


def _variants(case, flavour):
    """What set_variant offers for the case's camera and scene: the panorama renders variants 0 and 3 only; a scene without a mesh has no
    walk to choose."""
    if flavour in ("analytic", "cubes") or case.form.startswith("pano"):
        return (0, 3)
    return (0, 3, 41, 43)


def _run_case(renderer, wlib, huge_obj, name):
    case = sc.CASES[name]
    W, H = case.frame
    img = sc.image(case.image)
    view = sc.form_rays(case.form, case.frame)[3]
    flavours = ("analytic", "mesh", "mesh_ieee") if case.scene == "allsky" else ("cubes",)
    for interval in sorted({s[0] for s in sc.settings(case)}):
        for flavour in flavours:
            if case.scene == "allsky":
                scene = sc.scene_of(case, interval, "analytic" if flavour == "analytic" else "mesh", huge_obj if flavour == "mesh_ieee" else None)
                windows = None
                sky, hit, undecided = sc.verdict(case, scene, interval)
            else:
                scene, windows, sky, hit, undecided = truth.case_verdict(case, interval, wlib)
            _setup(renderer, scene, W, H, windows=windows, **view)
            E = sc.device_matrix(case, scene)
            for flags in [s[1] for s in sc.settings(case) if s[0] == interval]:
                model = sc.model(case, interval, flags, scene.params["white_point"])
                renderer.set_doppler(bool(flags & 1), bool(flags & 2))
                seen = []
                for variant, in_flight in [(v, False) for v in _variants(case, flavour)] + [(0, True)]:
                    renderer.set_variant(variant)
                    renderer.set_environment(None)
                    rgba0, rgb0 = _frame(renderer, in_flight)
                    renderer.set_environment(img)
                    renderer.set_environment_frame(E)                  # un-turned: the library re-bases it at the launch
                    rgba, rgb = _frame(renderer, in_flight)
                    kernel, exact = renderer.last_variant(), bool(renderer.last_exact_rcp())
                    _REACHED.add((kernel, exact))
                    assert (kernel >= 2000) == case.windowed, (name, kernel)
                    what = f"{name} {flavour} interval {interval} flags {flags} variant {variant} kernel {kernel}{'' if exact or kernel % 100 not in (41, 43, 61, 63) else ' (IEEE form)'} {'in flight' if in_flight else 'blocking'}"
                    assert np.array_equal(rgb.view(np.uint32)[hit], rgb0.view(np.uint32)[hit]) and np.array_equal(rgba[hit], rgba0[hit]), f"{what}: a hit pixel changed with the sky"
                    if any(np.array_equal(rgb.view(np.uint32), s.view(np.uint32)) and np.array_equal(rgba, b) for s, b in seen):
                        continue                                       # bit for bit a form already checked
                    seen.append((rgb, rgba))
                    truth.check_sky(what, case, model, sky, undecided, rgb, rgba)
                assert seen
    _RAN.add(name)
    _reset(renderer)


@pytest.mark.parametrize("name", sc.case_ids())
def test_device_sky_agrees_with_the_model(renderer, wlib, huge_obj, name):
    _run_case(renderer, wlib, huge_obj, name)


@pytest.mark.parametrize("size", sc.IMAGES)
def test_device_lookup_at_crafted_directions(renderer, size):
    """rpt_probe which = 7 at the axes, both sides of the seam, within 1e-3 of each pole, texel centres and corners."""
    W, H = size
    img = sc.image(size)
    d = sc.crafted_directions(W, H)
    renderer.set_environment(img)
    out = renderer.probe(7, d, 5)
    renderer.set_environment(None)
    r = truth.check_lookup(f"rpt_probe 7, {W} x {H}", d, img, out)
    assert r["held"] >= 0.95 * len(d)


def recorded_sky_kernels():
    """(rpt_last_variant, rpt_last_exact_rcp) of every launch the kernel-choice record made with the sky on, one sample per pixel."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    p = golden["products"]["render"]
    names = [a[0] for a in p["axes"]]
    assert names == [a[0] for a in kc.products()["render"]["axes"]] and "sky" in names
    out = set()
    for combo, i in zip(itertools.product(*[a[1] for a in p["axes"]]), kc.unpack_index(p["index"])):
        c, o = dict(zip(names, combo)), golden["outcomes"][i]
        if c["sky"] and c["msaa"] == 1 and c["adaptive_aa"] == 1 and o[0] == 0:
            out.add((int(o[2]), bool(o[3])))
    return out


def test_every_sky_kernel_of_the_choice_table_was_held_to_the_model(renderer, wlib, huge_obj):
    for name in sc.case_ids():                       # (a case deselected on the command line runs here: the set must not depend on the selection)
        if name not in _RAN:
            _run_case(renderer, wlib, huge_obj, name)
    recorded = recorded_sky_kernels()
    assert {k for k, _ in recorded} == {603, 641, 643, 644, 703, 741, 744, 823, 861, 863, 864}, sorted(recorded)
    expected = recorded | RAYMAP_SKY | WINDOWED_SKY
    print("sky kernels held to the model (variant, exact reciprocal):", sorted(_REACHED))
    assert _REACHED == expected, (sorted(expected - _REACHED), sorted(_REACHED - expected))
