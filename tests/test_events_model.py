"""The event pass without a GPU (DESIGN.md "Event pass"): the C-ABI is declared, exported and bound; the record is 32 bytes on every
side; the CPU restatement (tests/native/event_oracle.c on the unchanged oracle) gives records that sit on the light cone, agree with
the oracle's own flash decision, and match an analytic sphere; the picture helper maps equal delays to equal colours."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import events_oracle as eo
import oracle_ffi
from relativitypathtracer_amd import events as ev_mod
from relativitypathtracer_amd.events import EVENT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["rpt_set_events_output", "rpt_render_events", "rpt_render_events_async", "rpt_read_events", "rpt_pick", "rpt_last_events_variant",
             "rpt_last_events_exact_rcp"]
RPT_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("events"))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rpt_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(_ffi.hip_lib_path())
    for name in NEW_CALLS:
        assert name in declared, f"include/rpt.h does not declare {name}"
        assert hasattr(raw, name), f"librpt_hip.so does not export {name}"
        assert name in _ffi.HIP_SYMBOLS, f"_ffi.HIP_SYMBOLS does not list {name}"


def test_record_is_32_bytes_on_every_side(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "rpt_layout.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(rpt_event), '
                   'offsetof(rpt_event, object), offsetof(rpt_event, dist), offsetof(rpt_event, event), offsetof(rpt_event, uv)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=gnu11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [32, 0, 4, 8, 24]
    assert EVENT_DTYPE.itemsize == 32
    assert [EVENT_DTYPE.fields[n][1] for n in ("object", "dist", "event", "uv")] == [0, 4, 8, 24]
    import relativitypathtracer_amd
    assert relativitypathtracer_amd.EVENT_DTYPE is EVENT_DTYPE


def test_every_new_call_refuses_a_null_context():
    from relativitypathtracer_amd import _ffi
    h = _ffi.hip()
    rec = np.zeros(1, dtype=EVENT_DTYPE)
    assert h.rpt_set_events_output(None, None) == RPT_ERR_ARG
    assert h.rpt_render_events(None) == RPT_ERR_ARG
    assert h.rpt_render_events_async(None) == RPT_ERR_ARG
    assert h.rpt_read_events(None, rec.ctypes.data, 32) == RPT_ERR_ARG
    assert h.rpt_pick(None, 0, 0, rec.ctypes.data) == RPT_ERR_ARG
    assert h.rpt_last_events_variant(None) == RPT_ERR_ARG
    exact = C.c_int(7)
    assert h.rpt_last_events_exact_rcp(None, C.byref(exact)) == RPT_ERR_ARG and exact.value == 7


# ---- the analytic anchor -----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("d,r", [(5.0, 2.0), (12.0, 0.5), (3.25, 1.75)])
def test_sphere_at_rest_straight_ahead(lib, d, r):
    """A sphere of radius r at rest at distance d straight ahead of a resting camera: the centre pixel (x = W/2, y = H/2 look exactly
    along +z) records the float the oracle's intersect_sphere returns for that ray, within 4 ulp of d - r; the corners are misses."""
    W, H = 128, 72
    scene = eo.scene_from_text(f"Os\n p0,0,{d},0,0,1,0,{r},{r},{r}\n v0,0,0\nR\n", interval=-1)
    rec = eo.oracle_events(lib, scene, W, H)
    c = rec[H // 2, W // 2]
    assert c["object"] == 0
    obj = scene.objects()[0]
    origin4 = np.ascontiguousarray(obj["stationaryCam"], dtype=np.float32)
    dir4 = (obj["Lorentz"].astype(np.float32) @ np.array([-1, 0, 0, 1], dtype=np.float32)).astype(np.float32)
    want = np.zeros(1, dtype=np.float32)
    a, _ = eo.oracle_args(scene, W, H)
    assert lib.rpt_event_oracle_sphere_dist(C.byref(a), 0, origin4.ctypes.data, dir4.ctypes.data, want.ctypes.data) == 0
    assert c["dist"].view(np.uint32) == want[0].view(np.uint32)
    assert _ulps(c["dist"], np.float32(d - r)) <= 4, (float(c["dist"]), d - r)
    # at rest the event is the hit point at the look-back time: (-dist, 0, 0, dist)
    assert np.allclose(c["event"], [-float(c["dist"]), 0.0, 0.0, float(c["dist"])], rtol=0, atol=1e-6)
    miss = np.zeros(1, dtype=EVENT_DTYPE)[0]
    miss["object"] = -1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert rec[y, x].tobytes() == miss.tobytes(), (x, y)


# ---- the null cone -----------------------------------------------------------------------------------------------------------------
# Every hit record taken back to the camera frame (events.camera_frame_events) must satisfy |dx| = |dt| = dist up to float error.  The
# bound is the oracle's own error, measured here: the largest relative residual over all eight shipped scenes x {rest, 0.9c} at
# 128 x 72 (the rest camera at each scene's own time, the 0.9c camera as it passes the origin), interval -1, no pixel excluded, is
# 1.088e-05 (cubes.txt at 0.9c, 58 hit pixels: objects at 0.9c against a camera at 0.9c; the other fifteen cases lie between 8.4e-08 and
# 2.7e-06 — run with -s to see each), and the assertion is 8 x that value.
MEASURED_NULL_CONE_RESIDUAL = 1.088e-05
NULL_CONE_FACTOR = 8.0


def null_cone_bound():
    return NULL_CONE_FACTOR * MEASURED_NULL_CONE_RESIDUAL


@pytest.mark.parametrize("camera", sorted(eo.CAMERAS))
@pytest.mark.parametrize("name", eo.SHIPPED)
def test_oracle_records_lie_on_the_null_cone(lib, name, camera):
    W, H = 128, 72
    scene = eo.load_scene(name, camera, interval=-1)
    rec = eo.oracle_events(lib, scene, W, H)
    hit = rec["object"] >= 0
    assert hit.any(), f"{name} {camera}: nothing hit"
    res = eo.null_cone_residual(rec, scene)
    print(f"null cone {name:15s} {camera:5s}: {int(hit.sum())} hit pixels, largest relative residual {res:.3e}")
    assert np.isfinite(res)
    assert res <= null_cone_bound(), f"{name} {camera}: residual {res:.3e} > {null_cone_bound():.3e}"
    # the look-back time of the helper is -dist on every hit pixel
    lb = ev_mod.look_back_time(rec, -1)
    assert np.array_equal(lb[hit], -rec["dist"][hit].astype(np.float64)) and np.isnan(lb[~hit]).all()
    # scene_frame_events composes the camera's inverse boost: intervals are invariant, so the scene-frame displacement is null as well
    sf = ev_mod.scene_frame_events(rec, scene, scene.camera_lorentz()[1])[hit]
    s2 = (sf[:, 1:] ** 2).sum(axis=1) - sf[:, 0] ** 2
    scale = (sf ** 2).sum(axis=1)
    assert np.all(np.abs(s2) <= 4 * null_cone_bound() * scale + 1e-12)


# ---- flash consistency -------------------------------------------------------------------------------------------------------------
FLASH_SCENE = ("Os\n p-1,0,6,0,0,1,0,2,2,2\n v0.6,0,0\n c0.30,0.40,0.50\n f1.5,0.6\n"
               "Oc\n p3,-1,7,0.5,0,1,0,1,1,1\n v0,0,0\n c0.5,0.2,0.2\nA0.5\nR\n")


@pytest.mark.parametrize("t", [0.0, 2.2, 7.9])
def test_flash_set_equals_the_pixels_the_oracle_doubles(lib, t):
    """event[0] is the proper-time coordinate the flash test reads: the flashing object's pixels with event[0] - period *
    floor(event[0] / period) < duration (in float) are EXACTLY those whose colour differs between the oracle's frame with the flash
    period set and its frame with the period zeroed."""
    W, H = 160, 90
    scene = eo.scene_from_text(FLASH_SCENE, t=t, interval=-1)
    objs = scene.objects()
    assert objs[0]["flashPeriod"] > 0 and objs[1]["flashPeriod"] == 0
    rec = eo.oracle_events(lib, scene, W, H)
    _, rgb_on, _ = oracle_ffi.render(scene, W, H)
    off = objs.copy()
    off["flashPeriod"] = 0
    _, rgb_off, _ = oracle_ffi.render(scene, W, H, objects=off)
    mine = rec["object"] == 0
    assert mine.sum() > 500
    period, duration = np.float32(objs[0]["flashPeriod"]), np.float32(objs[0]["flashDuration"])
    e0 = rec["event"][..., 0].astype(np.float32)
    phase = (e0 - period * np.floor(e0 / period).astype(np.float32)).astype(np.float32)
    lit = mine & (phase < duration)
    doubled = mine & np.any(rgb_on != rgb_off, axis=-1)
    assert np.array_equal(lit, doubled), f"t = {t}: {int((lit ^ doubled).sum())} pixels disagree"
    assert not np.any((rgb_on != rgb_off).any(axis=-1) & ~mine)
    assert 0 < lit.sum() < mine.sum(), "the flash boundary should cross the object at these times"


# ---- the picture helper ------------------------------------------------------------------------------------------------------------
def test_delay_map_equal_delays_equal_colours_misses_black():
    rec = np.zeros((4, 6), dtype=EVENT_DTYPE)
    rec["object"] = -1
    rec["object"][0, :] = 0
    rec["dist"][0, :] = [1.0, 2.5, 2.5, 7.0, 1.0, 7.0]
    rec["object"][2, 1] = 3
    rec["dist"][2, 1] = 2.5
    img = ev_mod.delay_map(rec, -1)
    assert img.shape == (4, 6, 3) and img.dtype == np.uint8
    assert np.array_equal(img[0, 1], img[0, 2]) and np.array_equal(img[0, 1], img[2, 1])       # equal look-back times, whatever the object
    assert np.array_equal(img[0, 0], img[0, 4]) and np.array_equal(img[0, 3], img[0, 5])
    assert not np.array_equal(img[0, 0], img[0, 1]) and not np.array_equal(img[0, 1], img[0, 3])
    assert (img[rec["object"] < 0] == 0).all() and (img[rec["object"] >= 0].max(axis=-1) > 0).all()
    # an isochrone: the first tenth of every band is darker than the rest of it
    band = np.zeros((1, 2), dtype=EVENT_DTYPE)
    band["dist"][0] = [3.05, 3.5]
    assert ev_mod.delay_map(band, -1, band=1.0, t_max=10.0)[0, 0].sum() < ev_mod.delay_map(band, -1, band=1.0, t_max=10.0)[0, 1].sum()
    # light propagation off: no delay anywhere, one colour for every hit
    flat = ev_mod.delay_map(rec, 0)
    assert len({tuple(c) for c in flat[rec["object"] >= 0]}) == 1 and (flat[rec["object"] < 0] == 0).all()
