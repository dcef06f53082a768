"""rpt_projection_tables (include/rpt.h): the equirectangular camera's column and row tables are float32-rounded sine and cosine of
angles evaluated in double, with the conventions of the header.  Host code only: runs without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from relativitypathtracer_amd import _ffi
from relativitypathtracer_amd.renderer import projection_tables

TWO_PI, PI = float(np.float32(2 * math.pi)), float(np.float32(math.pi))


def _want(width, height, h_fov, v_fov, yaw):
    h, v, y0 = (float(np.float32(t)) for t in (h_fov, v_fov, yaw))
    lam = y0 + h * ((np.arange(width, dtype=np.float64) + 0.5) / width - 0.5)
    phi = v * ((np.arange(height, dtype=np.float64) + 0.5) / height - 0.5)
    return (np.stack([np.sin(lam), np.cos(lam)], -1).astype(np.float32), np.stack([np.sin(phi), np.cos(phi)], -1).astype(np.float32))


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)        # sign-magnitude -> a monotonic integer line
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


CASES = [(512, 256, TWO_PI, PI, 0.0), (2048, 1024, TWO_PI, PI, 0.0), (3840, 1920, TWO_PI, PI, 0.0), (1, 1, TWO_PI, PI, 0.0),
         (333, 77, 1.5, 0.9, 0.3), (640, 480, math.pi / 2, math.pi / 3, -2.0), (1000, 3, 0.001, 0.002, 100.0),
         (257, 513, 5.0, 3.0, 1e4), (7, 5, 2e-6, 1e-6, -7.25)]


@pytest.mark.parametrize("w,h,h_fov,v_fov,yaw", CASES)
def test_tables_are_rounded_double_sin_cos(w, h, h_fov, v_fov, yaw):
    cols, rows = projection_tables(w, h, h_fov, v_fov, yaw)
    wc, wr = _want(w, h, h_fov, v_fov, yaw)
    assert cols.shape == (w, 2) and rows.shape == (h, 2) and cols.dtype == np.float32
    got, want = np.concatenate([cols.ravel(), rows.ravel()]), np.concatenate([wc.ravel(), wr.ravel()])
    d = _ulps(got, want)
    assert d.max() <= 1, (d.max(), np.flatnonzero(d > 1)[:5])
    assert (d == 0).mean() >= 0.999


def test_default_parameters_are_the_full_sphere():
    a = projection_tables(96, 48)
    b = projection_tables(96, 48, TWO_PI, PI, 0.0)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    lib = _ffi.hip()
    cols, rows = np.empty((96, 2), np.float32), np.empty((48, 2), np.float32)
    assert lib.rpt_projection_tables(1, None, 96, 48, cols.ctypes.data, rows.ctypes.data) == 0
    assert np.array_equal(cols, a[0]) and np.array_equal(rows, a[1])


def _dirs(cols, rows):
    s_l, c_l = cols[:, 0][None, :], cols[:, 1][None, :]
    s_p, c_p = rows[:, 0][:, None], rows[:, 1][:, None]
    return np.stack([c_p * s_l, np.broadcast_to(s_p, (rows.shape[0], cols.shape[0])), c_p * c_l], -1)     # (H, W, 3), row 0 = bottom


def test_conventions():
    W, H = 65, 33
    d = _dirs(*projection_tables(W, H))
    lon = np.degrees(np.arctan2(d[..., 0], d[..., 2]))
    lat = np.degrees(np.arcsin(np.clip(d[..., 1], -1, 1)))
    # yaw 0, odd W and H: the centre pixel looks at +z
    assert np.abs(d[H // 2, W // 2] - np.float32([0, 0, 1])).max() < 1e-6
    assert np.abs(d[H // 2, W // 2 + 1:, 0] + d[H // 2, W // 2 - 1::-1, 0]).max() < 1e-6       # symmetric about the centre
    # columns grow towards +x: longitude increases from -180 to +180, the right half looks to +x
    assert np.all(np.diff(lon[H // 2]) > 0) and lon[H // 2, 0] < -170 and lon[H // 2, -1] > 170
    assert np.all(d[:, W // 2 + 1:, 0] > 0) and np.all(d[:, :W // 2, 0] < 0)
    # row 0 is the bottom: latitude increases with the row
    assert np.all(np.diff(lat[:, W // 4]) > 0) and lat[0, 0] < -80 and lat[-1, 0] > 80
    # W = 2H: square pixels on the full sphere
    c2, r2 = projection_tables(128, 64)
    dl = np.diff(np.unwrap(np.arctan2(c2[:, 0], c2[:, 1]))).mean()
    dp = np.diff(np.arcsin(r2[:, 0])).mean()
    assert abs(dl - dp) < 1e-5


@pytest.mark.parametrize("yaw", [0.5, -1.25, math.pi / 2, 3.0])
def test_yaw_shifts_the_longitude(yaw):
    W, H = 200, 100
    c0, r0 = projection_tables(W, H)
    c1, r1 = projection_tables(W, H, yaw=yaw)
    assert np.array_equal(r0, r1)
    l0, l1 = np.arctan2(c0[:, 0], c0[:, 1]).astype(np.float64), np.arctan2(c1[:, 0], c1[:, 1]).astype(np.float64)
    shift = np.angle(np.exp(1j * (l1 - l0)))
    assert np.abs(shift - float(np.float32(yaw))).max() < 1e-5
    # a quarter turn: the centre looks at +x
    if yaw == math.pi / 2:
        d = _dirs(c1, r1)[H // 2, W // 2 - 1:W // 2 + 1].mean(axis=0)
        assert d[0] > 0.999


def test_bad_arguments_are_refused():
    lib = _ffi.hip()
    cols, rows = np.empty((16, 2), np.float32), np.empty((16, 2), np.float32)

    def call(mode, params, w=16, h=8, c=cols.ctypes.data, r=rows.ctypes.data):
        p = None if params is None else (C.c_float * 3)(*params)
        return lib.rpt_projection_tables(mode, p, w, h, c, r)

    assert call(1, (1.0, 1.0, 0.0)) == 0
    for mode in (0, 2, -1):                                        # the pinhole has no tables; unknown modes
        assert call(mode, None) == 1
    for params in ((0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (TWO_PI * 1.0001, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, PI * 1.0001, 0.0),
                   (math.nan, 1.0, 0.0), (1.0, math.nan, 0.0), (1.0, 1.0, math.inf), (1.0, 1.0, math.nan), (math.inf, 1.0, 0.0)):
        assert call(1, params) == 1, params
    assert call(1, (TWO_PI, PI, -1e30)) == 0                       # the bounds themselves, any finite yaw
    for w, h in ((0, 8), (16, 0), (-1, 8), (16, -5), (1 << 16, 1 << 16)):
        assert call(1, None, w, h) == 1, (w, h)
    assert call(1, None, c=None) == 1 and call(1, None, r=None) == 1
    with pytest.raises(ValueError):
        projection_tables(16, 8, mode="fisheye")
    with pytest.raises(ValueError):
        projection_tables(16, 8, v_fov=4.0)
