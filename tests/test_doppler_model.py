"""The Doppler model of rpt_set_doppler (DESIGN.md "Doppler and beaming") on the CPU: the signs and values of the two frequency
factors as the kernels form them from the Lorentz matrices librpt_scene builds, the float32 colour operator against float64, and
the C-ABI's argument check.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import doppler_model as dm
from relativitypathtracer_amd import Scene, _ffi


def _objects(text, camera_v=(0.0, 0.0, 0.0), t=0.0):
    s = Scene()
    s.inputScene(text)
    s.set_camera(camera_v, t)
    s.update_objects()
    return s.objects()


def _ray(n):
    n = np.asarray(n, dtype=np.float64)
    n = n / np.linalg.norm(n)
    return np.array([-1.0, n[0], n[1], n[2]])      # rayDir = (interval, n) with light propagation on


def _d_cam(obj, n):
    """interval / dot(Lorentz[0], rayDir): observed over emitted frequency of light from `obj` reaching the camera along -n."""
    L0 = obj["Lorentz"][0].astype(np.float64)
    return -1.0 / float(L0 @ _ray(n))


@pytest.mark.parametrize("beta", [0.2, 0.6, 0.95, 0.99])
def test_camera_factor_head_on_and_transverse(beta):
    b32 = float(np.float32(beta))                  # the scene holds velocities in float
    blue = math.sqrt((1 + b32) / (1 - b32))
    gamma = 1 / math.sqrt(1 - b32 * b32)
    tol = 1e-6 + 2e-7 / (1 - beta)                 # float32 matrix rows: gamma (1 - beta) cancels ~ 1 / (1 - beta) ulp
    # a body ahead (+z) approaching the camera at rest, then receding
    app = _objects(f"Os\n p0,0,8,0,0,1,0,1,1,1\n v0,0,{-beta}\nR\n")[0]
    rec = _objects(f"Os\n p0,0,8,0,0,1,0,1,1,1\n v0,0,{beta}\nR\n")[0]
    assert _d_cam(app, (0, 0, 1)) == pytest.approx(blue, rel=tol)
    assert _d_cam(rec, (0, 0, 1)) == pytest.approx(1 / blue, rel=tol)
    # the camera flying at the body at rest: the same blue shift (only relative motion counts)
    cam = _objects("Os\n p0,0,8,0,0,1,0,1,1,1\n v0,0,0\nR\n", camera_v=(0.0, 0.0, beta))[0]
    assert _d_cam(cam, (0, 0, 1)) == pytest.approx(blue, rel=tol)
    # a ray transverse to the body's motion in the camera frame: the transverse Doppler effect, 1 / gamma
    side = _objects(f"Os\n p0,0,8,0,0,1,0,1,1,1\n v{beta},0,0\nR\n")[0]
    assert _d_cam(side, (0, 0, 1)) == pytest.approx(1 / gamma, rel=1e-6)
    # at rest: exactly 1
    rest = _objects("Os\n p0,0,8,0,0,1,0,1,1,1\n v0,0,0\nR\n")[0]
    assert np.float32(-1.0) / np.float32(rest["Lorentz"][0] @ _ray((0, 0, 1)).astype(np.float32)) == np.float32(1.0)


def _d_light(light, surface, L_lightframe):
    """The kernel's light factor: lightDir_ObjFrame.t / lightDir_LightFrame.t with lightDir_LightFrame = (interval |L|, L)."""
    L = np.asarray(L_lightframe, dtype=np.float64)
    ld_light = np.array([-np.linalg.norm(L), *L])
    ld_cam = light["InvLorentz"].astype(np.float64) @ ld_light
    ld_obj = surface["Lorentz"].astype(np.float64) @ ld_cam
    return ld_obj[0] / ld_light[0]


@pytest.mark.parametrize("beta", [0.3, 0.9])
def test_light_factor_signs(beta):
    b32 = float(np.float32(beta))
    blue = math.sqrt((1 + b32) / (1 - b32))
    # a surface at rest at the origin side, a light ahead of it on the z axis moving toward it (-z) or away (+z); L points from the
    # hit point to the light (+z) in the light's frame
    for v, want in ((-beta, blue), (beta, 1 / blue)):
        objs = _objects(f"Oc\n p0,0,4,0,0,1,0,1,1,1\n v0,0,0\nOs\n p0,0,12,0,0,1,0,0.5,0.5,0.5\n l1\n v0,0,{v}\nR\n")
        surface, light = objs[0], objs[1]
        assert _d_light(light, surface, (0, 0, 6)) == pytest.approx(want, rel=1e-6 + 2e-7 / (1 - beta))
    # light at rest: exactly no shift
    objs = _objects("Oc\n p0,0,4,0,0,1,0,1,1,1\nOs\n p0,0,12,0,0,1,0,0.5,0.5,0.5\n l1\nR\n")
    assert _d_light(objs[1], objs[0], (0.3, -0.2, 6)) == pytest.approx(1.0, abs=0)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_operator_float32_against_float64(flags):
    rng = np.random.default_rng(7 + flags)
    D, c = dm.kat_inputs(20000, rng)
    got = dm.S32(D, c, flags).astype(np.float64)
    want = dm.S64(D.astype(np.float64), c.astype(np.float64), flags)
    scale = np.maximum(np.abs(want), np.abs(c.astype(np.float64)).max(axis=1, keepdims=True) * np.maximum(1.0, D.astype(np.float64)[:, None] ** 4))
    # a few ulp of the channel's scale (the spectrum is steep near a knot: the float32 abscissa's rounding moves it by a few ulp)
    err = np.abs(got - want) / np.where(scale > 0, scale, 1.0)
    # next to a knot the float32 quotient nu / D can land on the other side of it: those samples differ by the slope times an ulp
    assert np.quantile(err, 0.999) < 4e-7 and err.max() < 1e-5, err.max()


def test_operator_identity_continuity_and_support():
    rng = np.random.default_rng(11)
    c = (rng.uniform(0, 3, size=(4096, 3))).astype(np.float32)
    for flags in (0, 1, 2, 3):
        one = dm.S32(np.ones(4096, np.float32), c, flags)
        assert np.array_equal(one.view(np.uint32), c.view(np.uint32))      # D == 1: c bit for bit
    # continuity across every knot: the values on both sides of a knot approach the knot's value
    r, g, b = np.float32(0.3), np.float32(0.7), np.float32(1.9)
    vals = {dm.K0: 0.0, dm.NU_R: r, dm.NU_G: g, dm.NU_B: b, dm.K4: 0.0}
    for k, v in vals.items():
        at = dm.spectrum32(np.array([k], np.float32), r, g, b)[0]
        lo = dm.spectrum32(np.array([np.nextafter(k, np.float32(0))], np.float32), r, g, b)[0]
        hi = dm.spectrum32(np.array([np.nextafter(k, np.float32(9))], np.float32), r, g, b)[0]
        assert at == np.float32(v)
        assert abs(lo - v) < 1e-5 and abs(hi - v) < 1e-5
    # zero beyond the outer knots, for any colour
    u = np.concatenate([np.linspace(-5, float(dm.K0), 1000), np.linspace(float(dm.K4), 50, 1000)]).astype(np.float32)
    z = dm.spectrum32(u, np.full(u.shape, 5, np.float32), np.full(u.shape, 5, np.float32), np.full(u.shape, 5, np.float32))
    assert not z.any()
    # a colour shifted past one knot spacing fades to black (infrared / ultraviolet)
    assert not dm.S32(np.array([1e-3, 1e3], np.float32), np.ones((2, 3), np.float32), 1).any()


def test_set_doppler_rejects_null_context_without_a_device():
    lib = _ffi.hip()
    assert lib.rpt_set_doppler(None, 1) == 1            # RPT_ERR_ARG
    assert lib.rpt_set_debug_doppler(None, C.c_void_p(1)) == 1
    buf = (C.c_float * 11)()
    assert lib.rpt_read_debug_doppler(None, buf, 44) == 1
