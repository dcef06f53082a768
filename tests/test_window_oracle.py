"""tests/native/window_oracle.c — the CPU oracle with the per-object time windows restated (DESIGN.md "Time windows") — checked where
no GPU is needed: with no windows, or every window at its default, it is the oracle (the committed golden frames byte for byte), and on
the test scenes the three rules each act.  tests/test_gpu_windows.py then holds every windowed kernel to this restatement byte for byte.

The windows come from window_oracle.choose_windows: one bound of several objects' windows at the median emission time of the object's
visible pixels, a light's lower bound at the median time its light left it.  Non-vacuity, asserted per scene on the CPU alone:
  (a) at least 5 % of the pixels differ from the un-windowed frame, (b) at least 5 % still hit something, (c) some pixel shows a
  farther object through a rejected nearer one, (d) some shadow is removed because its occluder is outside its window, (e) some light
  is outside its window at a lit pixel.
Every scene the windowed GPU tests use is held to this: arch, shadows, cubes, rulers_delay and the generated 66-object scene meet all
five.  cubes.txt and rulers.txt have no light of their own, so the tests use them with a lamp and a shadow-taking surface added
(window_oracle.LIT).  "rulers" is that scene as the file asks for it, with light propagation off (interval 0): there trace() does not
enter its light loop at all (opencl_kernel.cl:573), so no shadow ray and no light exist for (d) and (e) to speak of, whatever the scene;
it is the case of rule 4, and meets (a), (b) and (c)."""
import os

import numpy as np
import pytest

import events_oracle as eo
import oracle_ffi
import window_oracle as wo
from conftest import CONFIGS, load_config

W, H = 128, 72
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return wo.build_library(tmp_path_factory.mktemp("windows"))


def _scene(name):
    return wo.load(name)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_default_windows_reproduce_the_golden_frames(lib, name):
    g = np.load(os.path.join(GOLDEN, f"oracle_{name}_128x72.npz"))
    scene = load_config(name)
    assert np.array_equal(scene.buffers()["objects"], g["objects"]), "Object[] bytes drifted"
    for windows in (None, wo.default_windows(len(scene.objects()))):
        px, rgb, ev, book = wo.render(lib, scene, W, H, windows)
        assert np.array_equal(px["rgba"].reshape(H, W, 4), g["rgba"])
        assert np.array_equal(rgb.view(np.uint32), g["rgb"].view(np.uint32))
        assert not (book & ~np.uint8(wo.HIT)).any()
    want = oracle_ffi.render(scene, W, H)[0]
    assert px.tobytes() == want.tobytes()                      # all 16 bytes of every pixel
    assert ev.tobytes() == eo.oracle_events(eo.build_library(os.path.dirname(lib._name)), scene, W, H).tobytes()


def test_the_doppler_and_sky_forms_with_default_windows_are_their_oracles(lib, tmp_path):
    import doppler_oracle as do
    import raymap_cases as rc
    scene = load_config("cubes")
    dirs = eo.pinhole_dirs(W, H)
    want = do.render(do.build_oracle(tmp_path), scene, W, H, 3, dirs=dirs)[:2]
    got = wo.render(lib, scene, W, H, wo.default_windows(len(scene.objects())), flags=3)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    y, x = np.mgrid[0:32, 0:64]
    img = np.ascontiguousarray(np.stack([40 + 3 * x, 30 + 6 * y, 220 - 2 * ((x + y) % 64)], -1).astype(np.uint8))
    E = scene.camera_lorentz()[1]
    want = rc.environment_frame(rc.environment_oracle(tmp_path), scene, W, H, dirs.reshape(H, W, 3), E, img, 3)
    got = wo.render(lib, scene, W, H, None, flags=3, sky=img, sky_frame=E)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def _stats(lib, scene, interval=None, flip=False):
    w = wo.choose_windows(lib, scene, W, H, interval=interval, flip=flip)
    base = wo.render(lib, scene, W, H, None, interval=interval)
    px, rgb, ev, book = wo.render(lib, scene, W, H, w, interval=interval)
    n = float(W * H)
    return dict(windows=w, events=ev, base_events=base[2], changed=(px["rgba"] != base[0]["rgba"]).any(axis=-1).sum() / n,
                hit=(ev["object"] >= 0).sum() / n, behind=int((book & wo.BEHIND_REJECTED > 0).sum()),
                shadow=int((book & wo.SHADOW_REMOVED > 0).sum()), light_out=int((book & wo.LIGHT_OUT > 0).sum()))


@pytest.mark.parametrize("name", [n for n in wo.SCENES if n != "rulers"])
def test_the_three_rules_act_on_every_scene_with_light_delay(lib, name):
    s = _stats(lib, _scene(name), flip=wo.FLIP.get(name, False))
    print(name, {k: v for k, v in s.items() if k not in ("windows", "events", "base_events")})
    assert np.isfinite(s["windows"]).sum() >= 3
    assert s["changed"] >= 0.05 and s["hit"] >= 0.05
    assert s["behind"] >= 1, "no pixel shows a farther object through a rejected nearer one"
    assert s["shadow"] >= 1, "no shadow is removed because its occluder is outside its window"
    assert s["light_out"] >= 1, "no light is outside its window at a lit pixel"


def test_rule_four_acts_on_rulers_with_light_propagation_off(lib):
    scene = _scene("rulers")
    assert scene.params["interval"] == 0 and scene.objects()["light"].any()
    s = _stats(lib, scene)
    assert np.isfinite(s["windows"]).sum() >= 3
    assert s["changed"] >= 0.05 and s["hit"] >= 0.05 and s["behind"] >= 1
    assert s["shadow"] == 0 and s["light_out"] == 0          # (interval 0: the light loop is not entered, there is nothing to window)


@pytest.mark.parametrize("name", wo.SCENES)
def test_every_windowed_record_lies_in_its_window_and_only_rejected_winners_change(lib, name):
    s = _stats(lib, _scene(name), flip=wo.FLIP.get(name, False))
    ev, base, w = s["events"], s["base_events"], s["windows"]
    hit = ev["object"] >= 0
    assert wo.accepts(w, ev["object"][hit], ev["event"][..., 0][hit]).all()
    # a pixel whose un-windowed winner lies in its window keeps it: a window only removes hits
    kept = (base["object"] >= 0)
    kept[kept] = wo.accepts(w, base["object"][kept], base["event"][..., 0][kept])
    assert ev[kept].tobytes() == base[kept].tobytes()
    # an object that is never there (t0 >= t1) is not seen, does not shade and does not shine: the scene without it
    never = wo.default_windows(len(w))
    victim = int(np.bincount(base["object"][base["object"] >= 0]).argmax())
    never[victim] = (1.0, 1.0)
    assert not (wo.render(lib, _scene(name), W, H, never)[2]["object"] == victim).any()
