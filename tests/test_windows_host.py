"""The host side of the time windows (DESIGN.md "Time windows"), no GPU: the DSL's `w` command and Scene.windows(), and
relativitypathtracer_amd.worldline — its boost against the host's own Lorentz matrix, legs that meet at the breakpoints, what it refuses."""
import math

import numpy as np
import pytest

from relativitypathtracer_amd import Scene, worldline


def _scene(text, v=(0.0, 0.0, 0.0), t=0.0):
    s = Scene()
    s.inputScene(text)
    s.set_camera(v, t)
    s.update_objects()
    return s


def test_a_scene_without_w_has_no_windows():
    assert _scene("Os p0,0,5,0,0,1,0,1,1,1\nOc p2,0,5,0,0,1,0,1,1,1\nR\n").windows() is None
    assert Scene.from_file("ladder_paradox").windows() is None


def test_the_w_command_sets_the_current_objects_window():
    s = _scene("Os p0,0,5,0,0,1,0,1,1,1 w-1.5,2.25\nOc p2,0,5,0,0,1,0,1,1,1\nOs w-inf,3 p1,1,5,0,0,1,0,1,1,1\nOc w4,inf\nOc w5,1\nR\n")
    w = s.windows()
    assert w.dtype == np.float32 and w.shape == (5, 2)
    inf = np.float32(np.inf)
    assert w.tolist() == [[-1.5, 2.25], [-inf, inf], [-inf, 3.0], [4.0, inf], [5.0, 1.0]]
    assert len(s.objects()) == 5          # the object record is the reference's: nothing of the window is in it
    assert s.objects().dtype.itemsize == 320


def test_w_before_any_object_or_without_two_numbers_is_a_warning_not_a_window():
    s = Scene()
    assert "w1,2" in s.inputScene("w1,2\nOs p0,0,5,0,0,1,0,1,1,1\nR\n")
    assert s.windows() is None
    for bad in ("w5", "wabc", "w5,", "w,5", "w1,2,3", "w1,x", "wnan,1", "w"):
        s = Scene()
        diagnostics = s.inputScene(f"Os p0,0,5,0,0,1,0,1,1,1 {bad}\nR\n")
        assert s.windows() is None, bad
        assert bad in diagnostics, (bad, diagnostics)


def test_windows_is_cached_per_parse_and_read_only():
    s = Scene()
    s.inputScene("Os p0,0,5,0,0,1,0,1,1,1 w1,2\nR\n")
    w = s.windows()
    assert w is s.windows() and not w.flags.writeable


@pytest.mark.parametrize("v", [(0.6, 0.0, 0.0), (0.0, -0.3, 0.5), (0.2, 0.3, -0.7), (0.0, 0.0, 0.0)])
def test_boost_is_the_hosts_lorentz_matrix(v):
    """For a resting camera Object.Lorentz is the host's float32 Lorentz(v): the float64 boost agrees with it to the rounding of the
    host's own matrix — gamma is formed from float32 1 - |v|^2 (relative error up to 2^-24 / (1 - |v|^2) in gamma^2) and each entry by a
    few float32 operations: 8 units of 2^-24 relative to gamma / (1 - |v|^2) covers it."""
    s = _scene(f"Os p0,0,5,0,0,1,0,1,1,1 v{v[0]},{v[1]},{v[2]}\nR\n")
    host = s.objects()["Lorentz"][0].astype(np.float64)
    v32 = np.asarray(v, dtype=np.float32).astype(np.float64)
    b = worldline.boost(v32)
    g = b[0, 0]
    assert np.max(np.abs(host - b)) <= 8 * 2.0 ** -24 * g / (1.0 - float(v32 @ v32))


def test_consecutive_legs_meet_at_the_breakpoints():
    events = [(0.0, 0.0, 0.0, 5.0), (10.0, 0.0, 0.0, 11.0), (15.0, 2.0, 1.0, 9.0), (30.0, 2.0, 1.0, 9.0)]
    wl = worldline.piecewise(events, v_before=(0.1, 0.0, 0.0), v_after=(0.0, 0.0, -0.5))
    assert len(wl) == 5
    assert wl[0].window[0] == -math.inf and wl[-1].window[1] == math.inf
    assert np.allclose(wl[1].velocity, (0.0, 0.0, 0.6), rtol=0, atol=1e-15)
    for j in range(len(wl) - 1):
        end, start = wl[j].centre_at(wl[j].window[1]), wl[j + 1].centre_at(wl[j + 1].window[0])
        scale = np.maximum(np.abs(end), 1.0)
        assert np.all(np.abs(end - start) <= 1e-12 * scale), (j, end, start)
        assert np.all(np.abs(end - np.asarray(events[j])) <= 1e-12 * scale)
    w = wl.windows()
    assert w.dtype == np.float32 and w.shape == (5, 2) and np.all(w[1:, 0] < w[1:, 1])


def test_to_dsl_round_trips_through_the_scene_parser():
    wl = worldline.piecewise([(0.0, 0.0, 0.0, 5.0), (10.0, 0.0, 0.0, 11.0), (20.0, 0.0, 0.0, 5.0)])
    s = _scene(wl.to_dsl("Os", scale=(0.5, 0.5, 0.5), extra="c1,0,0") + "R\n")
    assert np.array_equal(s.windows(), wl.windows())
    assert np.allclose(s.velocities()[:, :3], [leg.velocity for leg in wl], atol=1e-7)
    assert np.allclose(s.objects()["M"][:, :3, 3], [leg.position for leg in wl], rtol=1e-6)
    assert np.allclose(s.objects()["color"][:, :3], (1, 0, 0))


def test_what_piecewise_refuses():
    with pytest.raises(ValueError):
        worldline.piecewise([(0.0, 0, 0, 0), (1.0, 0, 0, 1.0)])            # light-like
    with pytest.raises(ValueError):
        worldline.piecewise([(0.0, 0, 0, 0), (1.0, 0, 2.0, 0)])            # superluminal
    with pytest.raises(ValueError):
        worldline.piecewise([(0.0, 0, 0, 0), (0.0, 0, 0, 0)])              # not later
    with pytest.raises(ValueError):
        worldline.piecewise([(1.0, 0, 0, 0), (0.5, 0, 0, 0)])              # earlier
    with pytest.raises(ValueError):
        worldline.piecewise([(0.0, 0, 0, 0)])                              # one event, no open leg
    with pytest.raises(ValueError):
        worldline.piecewise([(0.0, 0, 0, 0), (1.0, 0, 0, 0)], v_after=(0.0, 1.0, 0.0))
