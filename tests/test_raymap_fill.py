"""rpt_raymap_fill (include/rpt.h; host code, no device needed) against its restatement in float64 numpy (tests/raymap_cases.py): every
component, the set of pixels without a ray, known directions, the share of the frame an inscribed fisheye leaves dark, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from raymap_cases import DEG, KINDS, fill64, rho64
from relativitypathtracer_amd import _ffi
from relativitypathtracer_amd.renderer import raymap

TWO_PI_F = float(np.float32(2.0 * math.pi))        # the float nearest 2 pi: the closed end of the fisheyes' range
BELOW_TWO_PI_F = float(np.nextafter(np.float32(2.0 * math.pi), np.float32(0.0)))
SIZES = [(96, 96), (100, 52), (33, 47), (1, 1), (12, 4)]      # (both even or both odd: no pixel centre of an inscribed circle has rho = 1)
FOVS = {"fisheye": [10.0 * DEG, 180.0 * DEG, 220.0 * DEG, TWO_PI_F], "equisolid": [90.0 * DEG, 180.0 * DEG, TWO_PI_F],
        "stereographic": [60.0 * DEG, 180.0 * DEG, 300.0 * DEG, BELOW_TWO_PI_F]}


def _ulps(got, want64):
    """|got - fl(want)| in units of the float spacing at fl(want)"""
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("kind", list(FOVS))
@pytest.mark.parametrize("fit", [0, 1])
def test_azimuthal_maps_equal_float64(kind, fit):
    for W, H in SIZES:
        _, _, rho = rho64(W, H, fit)
        assert np.abs(rho - 1.0).min() > 1e-12, (W, H, fit)        # about the INPUTS: no pixel centre sits on the image circle
        for fov in FOVS[kind]:
            got = raymap(kind, W, H, fov=fov, fit=fit)
            want, none = fill64(kind, W, H, fov, fit)
            # about the INPUTS again: the bound below is that of two correctly rounded evaluations of ONE real number.  cos theta next to a
            # zero of the cosine is theta's own rounding error (about 2^-51), not a number both sides share, so no ray of these cases may
            # have |cos theta| < 1e-7 (the error is then below 2^-27 relative, an eighth of the float's half ulp); sin theta next to pi likewise
            ray = ~none & (rho > 0)
            assert np.abs(want[..., 2][ray]).min(initial=1.0) >= 1e-7 and np.hypot(want[..., 0], want[..., 1])[ray].min(initial=1.0) >= 1e-7, (kind, W, H, fov, fit)
            assert got.shape == (H, W, 3) and got.dtype == np.float32
            assert np.array_equal(np.all(got == 0, axis=-1), none), (kind, W, H, fov, fit)      # the no-ray set is exactly {rho > 1}
            # two correctly rounded double evaluations can straddle a float rounding boundary: one float ulp, no more
            assert _ulps(got, want).max() <= 1.0, (kind, W, H, fov, fit, _ulps(got, want).max())
            assert np.isfinite(got).all()
        if fit == 1:
            assert not none.any()


@pytest.mark.parametrize("H", [1, 7, 20, 64])
def test_cube_strip_equals_float64(H):
    got = raymap("cube_strip", 6 * H, H)
    want, none = fill64("cube_strip", 6 * H, H)
    assert not none.any() and not np.all(got == 0, axis=-1).any()
    assert _ulps(got, want).max() <= 1.0


def test_known_directions():
    # the centre pixel pair of an even frame straddles +z symmetrically
    for kind in FOVS:
        d = raymap(kind, 64, 48, fov=2.0, fit=0)
        l, r = d[24, 31], d[24, 32]
        assert l[0] == -r[0] and l[0] < 0 and l[1] == r[1] and l[2] == r[2] and l[2] > 0.99
        assert np.array_equal(d[23, 31] * (1, -1, 1), d[24, 31])
    # an odd frame has a centre pixel: rho = 0, exactly +z
    assert np.array_equal(raymap("fisheye", 33, 33, fov=3.0)[16, 16], (0, 0, 1))
    # the equidistant fisheye at 2 pi: the rim of the image circle looks along -z
    d = raymap("fisheye", 1001, 1001, fov=TWO_PI_F, fit=0)[500, 1000]         # rho = 1000 / 1001
    assert d[2] < -0.9999 and abs(d[1]) == 0 and 0 < d[0] < 0.004
    # the cube strip's face centres look along the axes, in the order +x, -x, +y, -y, +z, -z
    d = raymap("cube_strip", 126, 21)
    for f, axis in enumerate([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]):
        assert np.array_equal(d[10, 21 * f + 10], axis), f
    # ... each face a 90-degree pinhole whose up is +y (the +-y faces: -+z): the top row's centre leans towards up by (H - 1) / H
    for f, up in enumerate([(0, 1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (0, 1, 0)]):
        lean = d[20, 21 * f + 10] - d[10, 21 * f + 10]
        assert np.allclose(lean, np.array(up) * (20.0 / 21.0), rtol=0, atol=1e-7), f
    # 180 degrees inscribed: the rim lies in the plane z = 0
    d = raymap("fisheye", 200, 200, fov=math.pi, fit=0)
    assert abs(d[100, 199][2]) < 0.01 and d[100, 199][0] > 0.9999


def test_share_of_pixels_without_a_ray():
    d = raymap("fisheye", 96, 96, fov=math.pi, fit=0)
    share = float(np.all(d == 0, axis=-1).mean())
    assert abs(share - (1.0 - math.pi / 4.0)) <= 0.02, share
    assert not np.all(raymap("fisheye", 96, 96, fov=math.pi, fit=1) == 0, axis=-1).any()


def test_refusals():
    lib = _ffi.hip()
    out = np.zeros((8, 48, 3), dtype=np.float32)

    def call(kind, params, W=48, H=8, dst=out.ctypes.data):
        p = None if params is None else (C.c_float * len(params))(*params)
        return lib.rpt_raymap_fill(kind, p, W, H, dst)

    assert call(KINDS["fisheye"], (2.0, 0.0)) == 0
    assert call(KINDS["cube_strip"], None) == 0
    for kind in (-1, 4, 99):                                                   # a kind that is none
        assert call(kind, (2.0, 0.0)) == 1
    assert call(KINDS["stereographic"], (TWO_PI_F, 0.0)) == 1                    # strictly below 2 pi
    assert call(KINDS["stereographic"], (BELOW_TWO_PI_F, 0.0)) == 0
    for kind in ("fisheye", "equisolid"):
        assert call(KINDS[kind], (TWO_PI_F, 0.0)) == 0                         # the closed end
        assert call(KINDS[kind], (float(np.nextafter(np.float32(TWO_PI_F), np.float32(7.0))), 0.0)) == 1
    for kind in ("fisheye", "equisolid", "stereographic"):
        for bad in ((0.0, 0.0), (-1.0, 0.0), (math.nan, 0.0), (math.inf, 0.0), (2.0, 2.0), (2.0, 0.5), (2.0, math.nan)):
            assert call(KINDS[kind], bad) == 1, (kind, bad)
        assert call(KINDS[kind], None) == 1
        assert call(KINDS[kind], (2.0, 0.0), W=0) == 1 and call(KINDS[kind], (2.0, 0.0), H=-3) == 1
        assert call(KINDS[kind], (2.0, 0.0), dst=None) == 1
    assert call(KINDS["cube_strip"], None, W=47, H=8) == 1                     # W != 6 H
    assert call(KINDS["cube_strip"], None, W=8, H=48) == 1
    assert call(KINDS["cube_strip"], (2.0, 0.0)) == 1                          # the strip takes no parameters
    assert call(KINDS["fisheye"], (2.0, 0.0), W=1 << 15, H=1 << 15) == 1         # 3 W H >= 2^31 (refused before anything is written)
    with pytest.raises(ValueError):
        raymap("fisheye", 48, 8, fov=7.0)
    with pytest.raises(ValueError):
        raymap("gnomonic", 48, 8)
