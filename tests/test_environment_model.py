"""The sky of rpt_set_environment (DESIGN.md "Environment map") on the CPU: the camera matrices librpt_scene hands out for it, the
aberration and the Doppler factor they give in float64, and the new entry points in both libraries.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from relativitypathtracer_amd import Scene, _ffi

REST_SPHERE = "Os\n p0,0,8,0,0,1,0,1,1,1\n v0,0,0\nR\n"      # one object of zero velocity: its Lorentz is the sky's frame


def _scene(v=(0.0, 0.0, 0.0)):
    s = Scene()
    s.inputScene(REST_SPHERE)
    s.set_camera(v, 0.0)
    return s


OBLIQUE = tuple(float(c) for c in np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]))
AXES = {"+z": (0.0, 0.0, 1.0), "oblique": OBLIQUE}


# ---- rpt_scene_get_camera_lorentz ----------------------------------------------------------------------------------------------
def test_camera_lorentz_fails_before_the_first_update():
    s = _scene()
    with pytest.raises(Exception, match="update_objects"):
        s.camera_lorentz()
    lib = _ffi.scene_lib()
    buf = (C.c_float * 16)()
    assert lib.rpt_scene_get_camera_lorentz(s._h, buf, buf) != 0
    assert lib.rpt_scene_get_camera_lorentz(None, buf, buf) != 0


@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("beta", [0.0, 0.2, 0.5, 0.95, 0.99])
def test_inverse_matrix_is_the_lorentz_of_an_object_at_rest(axis, beta):
    v = tuple(beta * c for c in AXES[axis])
    s = _scene(v)
    s.update_objects()
    lorentz, inv = s.camera_lorentz()
    obj = s.objects()[0]
    assert np.array_equal(inv.view(np.uint32), obj["Lorentz"].view(np.uint32))            # bit for bit
    assert np.array_equal(lorentz.view(np.uint32), obj["InvLorentz"].view(np.uint32))
    prod = lorentz.astype(np.float64) @ inv.astype(np.float64)
    gamma2 = 1.0 / (1.0 - beta * beta)
    assert np.max(np.abs(prod - np.eye(4))) <= 16 * 2.0 ** -24 * gamma2                    # float entries up to gamma, products up to gamma^2
    if beta == 0.0:
        assert np.array_equal(lorentz, np.eye(4, dtype=np.float32)) and np.array_equal(inv, np.eye(4, dtype=np.float32))
    # the matrices follow the camera: a second update with another velocity replaces them
    s.set_camera((0.0, 0.1, 0.0), 0.0)
    s.update_objects()
    assert np.array_equal(s.camera_lorentz()[1].view(np.uint32), s.objects()[0]["Lorentz"].view(np.uint32))
    assert (beta == 0.0) or not np.array_equal(s.camera_lorentz()[1], inv)


def test_null_outputs_are_allowed():
    s = _scene((0.0, 0.0, 0.5))
    s.update_objects()
    lib = _ffi.scene_lib()
    a, b = (C.c_float * 16)(), (C.c_float * 16)()
    assert lib.rpt_scene_get_camera_lorentz(s._h, a, None) == 0
    assert lib.rpt_scene_get_camera_lorentz(s._h, None, b) == 0
    lorentz, inv = s.camera_lorentz()
    assert np.array_equal(np.array(a[:], dtype=np.float32), lorentz.reshape(-1))
    assert np.array_equal(np.array(b[:], dtype=np.float32), inv.reshape(-1))


# ---- the model in float64, on those matrices -------------------------------------------------------------------------------------
def _sky_direction_and_factor(E, n):
    """k = E (interval, n) with interval = -1; the direction the sky is looked up at, and D_env = interval / k.t."""
    n = np.asarray(n, dtype=np.float64)
    n = n / np.linalg.norm(n)
    k = E.astype(np.float64) @ np.array([-1.0, *n])
    return k[1:] / np.linalg.norm(k[1:]), -1.0 / k[0]


def _perpendicular(a):
    p = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
    return p / np.linalg.norm(p)


@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("beta", [0.2, 0.5, 0.95])
def test_aberration_formula(axis, beta):
    """A sky direction at polar angle theta' from the velocity (sky frame) is seen at theta, cos theta = (cos theta' + beta) / (1 + beta cos theta')."""
    a = np.array(AXES[axis])
    s = _scene(tuple(beta * a))
    s.update_objects()
    E = s.camera_lorentz()[1]
    b32 = float(np.linalg.norm(np.float32(beta) * a.astype(np.float32)))
    p = _perpendicular(a)
    tol = 1e-6 + 4e-7 / (1 - beta)
    for theta in np.linspace(0.0, math.pi, 37):
        n = math.cos(theta) * a + math.sin(theta) * p          # camera-frame direction at polar angle theta
        d, _ = _sky_direction_and_factor(E, n)
        cos_sky = float(d @ a)
        # invert the formula: cos theta' = (cos theta - beta) / (1 - beta cos theta)
        want = (math.cos(theta) - b32) / (1 - b32 * math.cos(theta))
        assert cos_sky == pytest.approx(want, abs=tol), (theta, cos_sky, want)
        assert (math.cos(theta)) == pytest.approx((want + b32) / (1 + b32 * want), abs=1e-9)
        # the azimuth about the velocity is unchanged
        if 0.1 < theta < math.pi - 0.1:
            side = d - cos_sky * a
            assert float(side @ p) / np.linalg.norm(side) == pytest.approx(1.0, abs=1e-5)


@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("beta", [0.2, 0.6, 0.95, 0.99])
def test_environment_doppler_factor(axis, beta):
    a = np.array(AXES[axis])
    s = _scene(tuple(beta * a))
    s.update_objects()
    E = s.camera_lorentz()[1]
    b32 = float(np.linalg.norm((np.float32(beta) * a.astype(np.float32)).astype(np.float64)))
    blue = math.sqrt((1 + b32) / (1 - b32))
    gamma = 1 / math.sqrt(1 - b32 * b32)
    tol = 1e-6 + 4e-7 / (1 - beta)
    assert _sky_direction_and_factor(E, a)[1] == pytest.approx(blue, rel=tol)               # ahead
    assert _sky_direction_and_factor(E, -a)[1] == pytest.approx(1 / blue, rel=tol)          # behind
    assert _sky_direction_and_factor(E, _perpendicular(a))[1] == pytest.approx(1 / gamma, rel=2e-6)      # transverse in the camera frame
    rest = _scene()
    rest.update_objects()
    assert _sky_direction_and_factor(rest.camera_lorentz()[1], a)[1] == 1.0                 # at rest: exactly 1


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    hip = C.CDLL(_ffi.hip_lib_path())
    for name in ("rpt_set_environment", "rpt_set_environment_frame"):
        assert hasattr(hip, name), name
        assert name in _ffi.HIP_SYMBOLS
    assert hasattr(_ffi.scene_lib(), "rpt_scene_get_camera_lorentz")
    text = open(__file__.replace("tests/test_environment_model.py", "include/rpt.h")).read()
    assert "int rpt_set_environment(rpt_ctx *ctx, const unsigned char *rgb8, int width, int height);" in text
    assert "int rpt_set_environment_frame(rpt_ctx *ctx, const float lorentz[16]);" in text


def test_argument_checks_need_no_device():
    lib = _ffi.hip()
    assert lib.rpt_set_environment(None, None, 0, 0) == 1                 # RPT_ERR_ARG: no context
    assert lib.rpt_set_environment_frame(None, None) == 1
