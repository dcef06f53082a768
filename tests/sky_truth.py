"""Float64 model of the environment map (DESIGN.md "Environment map"): what a pixel that hits nothing shows — TEST INFRASTRUCTURE.

A helper, no tests in it.  Plain numpy, float64 throughout, written from the geometry and from special relativity, as
tests/primitive_truth.py is for objects.  It shares nothing with tests/native/environment_oracle.c or the kernels but the model's stated
constants: the (u, v) convention (u = 1/2 + atan2(z, x) / 2 pi, v = 1/2 + asin(y) / pi), the texel at x / W with no half-texel offset,
row 0 at v = 1, wrap in columns, clamp in rows, byte / 255, S_f's knots (doppler_model.S64), Hable's curve and the white point
(primitive_truth.tonemap), the truncating pack, and the head's R = Ry(yaw) Rx(pitch) Rz(roll).  It reads no float32 matrix: not
Scene.camera_lorentz(), not rpt_orient_matrix.  The sky-frame look-back vector comes from the two velocities alone.

Rules
-----
 * A pixel looks along the unit vector n of its float32 camera direction (taken as float64), in the head's basis; the camera frame's
   direction is R n.
 * The light it receives travelled along the camera-frame displacement (interval, R n) (interval = -1: backwards in time, the look-back
   path; interval = 0: no light delay, the same formula on (0, R n)).  In the sky's rest frame that displacement is
   k = boost(v_sky) boost(-v_cam) (interval, R n): both velocities in the scene frame, primitive_truth.boost.
 * The sky is infinitely far away and at rest there: the pixel shows the image at d = k_xyz / |k_xyz|.
 * D_env = interval / k_t, the ratio of received to emitted frequency; 1 with interval 0 or with the Doppler flags 0.
 * The image is bilinear in (U, V) = (W u, H (1 - v)) between texel (x, y) at integer (U, V) = (x, y); column W is column 0, row H is row
   H - 1 (and row -1 row 0).
 * colour = S_f(D_env, sample); mapped = min(hable(colour) / hable(white), 1); byte = floor(255 mapped).

The float32 bound (DESIGN.md "Environment map", "How far float32 may put a sky pixel from the float64 model"; eps = 2^-24)
----------------------------------------------------------------------------------------------------------------------
Direction.  The float program normalises n (4 eps), re-bases E by R (one rounding per entry), and forms k by four-term dots (4 eps of
sum |E_ij| |r_j|); its E itself is off the exact product by e_E relative to A = |boost(v_sky)| |boost(-v_cam)| entrywise (`e_matrix`: eps
for a matrix handed over as the float32 rounding of the exact one; (1.5 g_sky^2 + 1.5 g_cam^2 + 16) eps for the library's own, the bound
tests/test_primitive_ground_truth.py::matrix_bounds holds Object.Lorentz to).  So, per component,
    |dk_i|  <=  (e_E + 9 eps) sum_j A_ij w_j,     w = (|interval|, 1, 1, 1)
    dn      =   |dk_xyz| / |k_xyz| + 4 eps         (the normalisation)
    dD / D  =   |dk_t| / |k_t| + eps               (the division)
A's 2-norm is a = gamma (1 + beta) of the sky against the camera and |k_xyz| >= |r| / a, so dn grows as eps a^2: the cancellation
ahead of a fast camera, where the sky's directions bunch up.
Coordinates.  |du| <= dn / (2 pi h) + ATAN2_ERROR / (2 pi) + 2 eps, h = hypot(d.x, d.z) (exactly on the axis, h = 0, atan2(+-0, +-0) is
exact and only the last two terms remain); |dv| <= min(dn / (pi sqrt(1 - d.y^2)), sqrt(2 dn) / pi) + ASIN_ERROR / pi + 2 eps.
Colour.  The sample is continuous (across cell borders and the seam) and bilinear in each cell, so while W |du| < 1 and H |dv| < 1
    |dc|  <=  W |du| Gx + H |dv| Gy + 8 eps
with Gx / Gy the largest differences between horizontally / vertically adjacent texels of the 3 x 3 cells around the model's cell
(4 x 4 texels, columns wrapped, rows clamped), per channel.  Otherwise the pixel has no finite bound.
After the lookup.  S_f by the model's own finite difference: S_f is linear in the colour with coefficients >= 0 and piecewise linear in
nu / D, so |dS| <= max over D(1 -+ dD / D) of |S_f(D', c) - S_f(D, c)| + max over D, D' of S_f(., dc), plus 24 eps max(c) D^p for its own
arithmetic (p = 3 with shift and beaming, 4 with beaming alone, 0 otherwise).  The tonemap is increasing for x >= 0: the two ends of
[colour - dS, colour + dS] bound the mapped colour — an interval, not an estimate — plus 8 eps (mapped + 1 / hable(white)) for Hable's
curve in float32.  The packed byte lies between the packs of the two ends of that interval: one step at the most wherever 255 tol <= 1/2.
Measured constants (tests/test_sky_ground_truth.py measures them on the CPU, never on the device): ATAN2_ERROR and ASIN_ERROR, four times
the largest absolute error of the restatement's atan2f / asinf against float64 over the directions of every case."""
from __future__ import annotations

import numpy as np

import doppler_model as dm
import primitive_truth as pt

EPS = 2.0 ** -24
ROUNDINGS = 8.0
# 4 x the largest |atan2f - atan2| (2.28e-07: an ulp of a float near pi) and |asinf - asin| (6.24e-08) of the CPU restatement's two functions
# over 18 010 directions: the crafted ones of both images and 400 sky-frame directions of every case of tests/sky_cases.py
# (tests/test_sky_ground_truth.py::test_measured_constants measures them again, prints them and holds them to these figures)
MEASURED_ATAN2_ERROR, MEASURED_ASIN_ERROR = 2.3e-07, 6.3e-08
ATAN2_ERROR = 4 * MEASURED_ATAN2_ERROR
ASIN_ERROR = 4 * MEASURED_ASIN_ERROR


def rotation(yaw=0.0, pitch=0.0, roll=0.0):
    """R = Ry(yaw) Rx(pitch) Rz(roll) of the float32 angles, in float64 (DESIGN.md "Free-look camera": the convention)."""
    y, p, r = (float(np.float32(a)) for a in (yaw, pitch, roll))
    c, s = np.cos(y), np.sin(y)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    c, s = np.cos(p), np.sin(p)
    Rx = np.array([[1, 0, 0], [0, c, s], [0, -s, c]])
    c, s = np.cos(r), np.sin(r)
    Rz = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def sky_frame(v_cam, v_sky=(0.0, 0.0, 0.0)):
    """Camera frame -> the sky's rest frame, both velocities in the scene frame (float32 values taken as float64)."""
    vc = np.asarray(v_cam, dtype=np.float32).astype(np.float64)
    vs = np.asarray(v_sky, dtype=np.float32).astype(np.float64)
    return pt.boost(vs) @ pt.boost(-vc)


def library_matrix_error(v_cam, v_sky=(0.0, 0.0, 0.0)):
    """e_E of the library's own float32 product of two float32 boosts, relative to |boost(v_sky)| |boost(-v_cam)|: matrix_bounds' figure."""
    g2 = lambda v: 1.0 / (1.0 - float(np.dot(np.float32(v).astype(np.float64), np.float32(v).astype(np.float64))))      # noqa: E731
    return (1.5 * g2(v_sky) + 6.0 + 1.5 * g2(v_cam) + 6.0 + 4.0) * EPS


# ---- the model's rules, one function each (tests/test_sky_ground_truth.py swaps each for a wrong one to show that the comparison bites) ----
def head(n, R):
    """The camera-frame direction of the head's direction n: R n, row-wise."""
    return n @ R.T


def uv_of(d):
    d = np.asarray(d, dtype=np.float64)
    return 0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi), np.arcsin(np.clip(d[:, 1], -1.0, 1.0)) / np.pi + 0.5


def texel_coords(u, v, W, H):
    return W * u, H * (1.0 - v)


def wrap_column(x, W):
    return x % W


def clamp_row(y, H):
    return np.clip(y, 0, H - 1)


def doppler_factor(interval, k_t):
    return float(interval) / k_t


def shift_and_beam(D, colour, flags):
    return dm.S64(D, colour, flags)


def sample(img, u, v):
    """The bilinear sample at (u, v) and what its bound needs: (colour (n, 3), Gx (n, 3), Gy (n, 3), x0, y0)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    T = img.astype(np.float64) / 255.0
    Uc, Vc = texel_coords(u, v, W, H)
    x0 = np.clip(np.floor(Uc), 0, W - 1).astype(np.int64)
    y0 = np.clip(np.floor(Vc), 0, H - 1).astype(np.int64)
    a, b = (Uc - x0)[:, None], (Vc - y0)[:, None]
    x1, y1 = wrap_column(x0 + 1, W), clamp_row(y0 + 1, H)
    colour = (1.0 - b) * ((1.0 - a) * T[y0, x0] + a * T[y0, x1]) + b * ((1.0 - a) * T[y1, x0] + a * T[y1, x1])
    xs = wrap_column(x0[:, None] + np.arange(-1, 3), W)
    ys = clamp_row(y0[:, None] + np.arange(-1, 3), H)
    block = T[ys[:, :, None], xs[:, None, :]]                                 # (n, 4 rows, 4 columns, 3 channels)
    Gx = np.abs(np.diff(block, axis=2)).max(axis=(1, 2))
    Gy = np.abs(np.diff(block, axis=1)).max(axis=(1, 2))
    return colour, Gx, Gy, x0, y0


def pack(mapped):
    """floor(255 x), saturating: the reference's (unsigned char)(c * 255)."""
    return np.clip(np.floor(255.0 * np.asarray(mapped, dtype=np.float64)), 0, 255).astype(np.int64)


def _doppler_power(flags):
    return 3 if flags == (dm.SHIFT | dm.BEAMING) else (4 if flags == dm.BEAMING else 0)


def lookup(dirs, img, dn=4 * EPS):
    """The lookup alone (rpt_probe which = 7) at directions `dirs` (normalised here): u, v, colour and their bounds."""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out = {"d": d}
    out["u"], out["v"] = uv_of(d)
    _coordinates(out, np.full(len(d), dn), img)
    return out


def _coordinates(out, dn, img):
    d = out["d"]
    H, W = np.asarray(img).shape[:2]
    h = np.hypot(d[:, 0], d[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        du = np.where(h > 0.0, dn / (2 * np.pi * h), 0.0) + ATAN2_ERROR / (2 * np.pi) + 2 * EPS
        dv = np.minimum(dn / (np.pi * np.sqrt(np.maximum(1.0 - d[:, 1] ** 2, 0.0))), np.sqrt(2 * dn) / np.pi) + ASIN_ERROR / np.pi + 2 * EPS
    colour, Gx, Gy, x0, y0 = sample(img, out["u"], out["v"])
    finite = (W * du < 1.0) & (H * dv < 1.0)
    dc = np.where(finite[:, None], (W * du)[:, None] * Gx + (H * dv)[:, None] * Gy + ROUNDINGS * EPS, np.inf)
    out.update(h=h, tol_u=du, tol_v=dv, linear=colour, tol_linear=dc, texel=np.stack([x0, y0], axis=1), Gx=Gx, Gy=Gy)


def frame(dirs, img, v_cam=(0.0, 0.0, 0.0), v_sky=(0.0, 0.0, 0.0), ypr=(0.0, 0.0, 0.0), interval=-1, flags=0, white_point=(1.0, 1.0, 1.0),
          e_matrix=EPS):
    """The model's sky for per-pixel float32 camera directions `dirs` (N, 3; not necessarily unit).  Returns a dict of (N, ...) arrays:
    d (the sky-frame direction), u, v, linear (the sample), D, colour (after S_f), mapped, bytes;  the conditioning terms a (scalar: the
    2-norm of E), dn, rel_D, h, tol_u, tol_v, tol_linear, tol_colour, tol_mapped (inf: no finite bound), byte_lo, byte_hi, texel."""
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    N = len(dirs)
    n = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    n_cam = head(n, rotation(*ypr))
    vc = np.asarray(v_cam, dtype=np.float32).astype(np.float64)
    vs = np.asarray(v_sky, dtype=np.float32).astype(np.float64)
    E = sky_frame(vc, vs)
    A = np.abs(pt.boost(vs)) @ np.abs(pt.boost(-vc))
    r = np.hstack([np.full((N, 1), float(interval)), n_cam])
    k = r @ E.T
    ks = np.linalg.norm(k[:, 1:], axis=1)
    d = k[:, 1:] / ks[:, None]
    dk = (e_matrix + 9 * EPS) * (A @ np.array([abs(float(interval)), 1.0, 1.0, 1.0]))
    dn = np.full(N, np.linalg.norm(dk[1:])) / ks + 4 * EPS
    out = {"d": d, "a": float(np.linalg.norm(E, 2)), "dn": dn, "k": k}
    out["u"], out["v"] = uv_of(d)
    _coordinates(out, dn, img)
    lin, dc = out["linear"], out["tol_linear"]
    shifted = flags != 0 and interval != 0
    if shifted:
        D = doppler_factor(interval, k[:, 0])
        rel_D = dk[0] / np.abs(k[:, 0]) + EPS
        S = lambda Dv, c: shift_and_beam(Dv, c, flags)          # noqa: E731
        colour = S(D, lin)
        ends = (D * (1.0 - rel_D), D * (1.0 + rel_D))
        fin = np.isfinite(dc).all(axis=1)
        dcf = np.where(fin[:, None], dc, 0.0)
        tol = np.maximum(np.abs(S(ends[0], lin) - colour), np.abs(S(ends[1], lin) - colour))
        tol = tol + np.maximum(np.maximum(S(ends[0], dcf), S(ends[1], dcf)), S(D, dcf))
        tol = tol + 3 * ROUNDINGS * EPS * lin.max(axis=1, keepdims=True) * (np.maximum(D, 1.0) ** _doppler_power(flags))[:, None]
        tol = np.where(fin[:, None], tol, np.inf)
    else:
        D, rel_D, colour, tol = np.ones(N), np.zeros(N), lin, dc
    wp = np.asarray(white_point, dtype=np.float64)
    mapped = pt.tonemap(colour, wp)
    with np.errstate(invalid="ignore"):
        hi = pt.tonemap(np.where(np.isfinite(tol), colour + tol, 0.0), wp)
        lo = pt.tonemap(np.maximum(np.where(np.isfinite(tol), colour - tol, 0.0), 0.0), wp)
    tol_m = np.maximum(hi - mapped, mapped - lo) + ROUNDINGS * EPS * (mapped + 1.0 / pt.hable(wp).min())
    tol_m = np.where(np.isfinite(tol), tol_m, np.inf)
    out.update(D=D, rel_D=rel_D, colour=colour, tol_colour=tol, mapped=mapped, tol_mapped=tol_m, bytes=pack(mapped),
               byte_lo=pack(np.where(np.isfinite(tol_m), mapped - tol_m, 0.0)), byte_hi=pack(np.where(np.isfinite(tol_m), mapped + tol_m, 1.0)))
    return out


def compare(model, rgb, rgba=None, mask=None):
    """Tonemapped float RGB (N, 3) and packed bytes (N, >= 3) of a float program against the model on the pixels of `mask`: a dict with
    n (pixels compared), ratio (largest error / bound), worst (its pixel), loose (share of compared pixels whose bound exceeds 2 / 255
    in some channel, no finite bound included), bad (pixels beyond their bound), byte_bad (pixels whose bytes leave [byte_lo, byte_hi])."""
    N = len(model["mapped"])
    mask = np.ones(N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
    rgb = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    tol = model["tol_mapped"]
    err = np.abs(rgb - model["mapped"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(np.isfinite(tol), err / tol, 0.0)
    ratio = np.where(mask[:, None], ratio, 0.0).max(axis=1)               # (a NaN of the float program: beyond any bound)
    ratio = np.where(np.isnan(ratio) & mask, np.inf, ratio)
    out = {"n": int(mask.sum()), "ratio": float(ratio.max(initial=0.0)), "worst": int(np.argmax(ratio)) if N else -1,
           "loose": float(((tol > 2.0 / 255.0).any(axis=1) & mask).sum() / max(int(mask.sum()), 1)), "bad": np.flatnonzero(ratio > 1.0),
           "byte_bad": np.zeros(0, dtype=np.int64)}
    if rgba is not None:
        b = np.asarray(rgba).reshape(N, -1)[:, :3].astype(np.int64)
        out["byte_bad"] = np.flatnonzero(mask & ((b < model["byte_lo"]) | (b > model["byte_hi"])).any(axis=1))
    return out
