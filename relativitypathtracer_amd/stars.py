"""Star catalogues for the star-field pass (include/rpt.h, rpt_set_stars) and a float64 model of where the pass puts them.

A catalogue is a numpy array of STAR_DTYPE: the 32-byte rpt_star records — `dir`, the direction one looks in to see the star, in the
sky's rest frame (x to the right, y up, z ahead; any non-zero length), and `rgb`, its linear colour at rest on the scale of object
colours.  random_catalogue and from_arrays make one, save / load keep it as raw records (what `rpt_render_main --stars FILE` reads),
Renderer.set_stars and render_scene(..., stars=) take it.  project() is rules 1-4 of the pass in float64: for previews without a
device, and the reference of the physics tests.  Host code only; nothing here touches the GPU."""
from __future__ import annotations

import math
from typing import Mapping, Optional, Sequence

import numpy as np

STAR_DTYPE = np.dtype([("dir", "<f4", (3,)), ("rgb", "<f4", (3,)), ("_pad", "<f4", (2,))])
assert STAR_DTYPE.itemsize == 32

# the three primaries of the Doppler model (DESIGN.md "Doppler and beaming"): CIE 1931 RGB, nm
WAVELENGTHS_NM = (700.0, 546.1, 435.8)
NU_R, NU_B = 546.1 / 700.0, 546.1 / 435.8
NU_K0, NU_K4 = 2.0 * NU_R - 1.0, 2.0 * NU_B - 1.0
_HC_OVER_K_NM = 1.438776877e7       # h c / k in nm K


def blackbody_rgb(temperature) -> np.ndarray:
    """(..., 3) float64: Planck's B_nu at the three primaries' frequencies for a temperature in kelvin, scaled so that the largest
    channel is 1 — the samples the Doppler model's piecewise-linear spectrum goes through."""
    T = np.asarray(temperature, dtype=np.float64)[..., None]
    lam = np.asarray(WAVELENGTHS_NM, dtype=np.float64)
    x = _HC_OVER_K_NM / (lam * T)
    b = (1.0 / lam) ** 3 / np.expm1(x)
    return b / b.max(axis=-1, keepdims=True)


def _catalogue(directions, rgb) -> np.ndarray:
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    if d.shape != c.shape:
        raise ValueError("one colour per direction")
    out = np.zeros(d.shape[0], dtype=STAR_DTYPE)
    out["dir"] = d
    out["rgb"] = c
    return out


def random_catalogue(n: int, seed: int = 0, alpha: float = 1.5, faintest: float = 0.02, brightest: float = 50.0,
                     temperatures: Sequence[float] = (3000.0, 12000.0), return_temperatures: bool = False):
    """n stars uniform on the sphere.  Brightness: a power law, N(> S) ~ S^-alpha from `faintest` up, cut at `brightest` (alpha = 1.5
    is what a uniform population in flat space gives).  Colour: a blackbody of a temperature drawn log-uniformly from `temperatures`,
    through blackbody_rgb, times the brightness.  return_temperatures=True returns (catalogue, temperatures): the float32 kelvin per
    star that Renderer.set_star_temperatures takes (the colours are built from those rounded values)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1.0, 1.0, n)
    lon = rng.uniform(-math.pi, math.pi, n)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d = np.stack([r * np.sin(lon), z, r * np.cos(lon)], -1)
    flux = np.minimum(faintest * (1.0 - rng.uniform(0.0, 1.0, n)) ** (-1.0 / alpha), brightest)
    T = np.exp(rng.uniform(math.log(temperatures[0]), math.log(temperatures[1]), n))
    if return_temperatures:
        T32 = T.astype(np.float32)
        return _catalogue(d, blackbody_rgb(T32) * flux[:, None]), T32
    return _catalogue(d, blackbody_rgb(T) * flux[:, None])


def from_arrays(ra, dec, magnitude, temperature, magnitude_zero: float = 1.0, return_temperatures: bool = False):
    """A catalogue from columns of a real one: right ascension and declination in radians (dir = (cos dec sin ra, sin dec, cos dec
    cos ra): declination is the latitude above the x-z plane, ra = 0 lies ahead), apparent magnitude (a star of magnitude 0 gets the
    brightness magnitude_zero, five magnitudes are a factor of 100) and temperature in kelvin (blackbody_rgb).
    return_temperatures=True returns (catalogue, temperatures): the float32 kelvin per star that Renderer.set_star_temperatures takes
    (the colours are built from those rounded values)."""
    ra, dec, mag, T = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (ra, dec, magnitude, temperature))
    if not (ra.shape == dec.shape == mag.shape == T.shape):
        raise ValueError("ra, dec, magnitude and temperature have one entry per star")
    d = np.stack([np.cos(dec) * np.sin(ra), np.sin(dec), np.cos(dec) * np.cos(ra)], -1)
    flux = magnitude_zero * 10.0 ** (-0.4 * mag)
    if return_temperatures:
        T32 = T.astype(np.float32)
        return _catalogue(d, blackbody_rgb(T32) * flux[:, None]), T32
    return _catalogue(d, blackbody_rgb(T) * flux[:, None])


def save(path, catalogue) -> None:
    """The raw 32-byte records, one after the other."""
    np.ascontiguousarray(catalogue, dtype=STAR_DTYPE).tofile(path)


def load(path) -> np.ndarray:
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size % 32:
        raise ValueError(f"{path}: {raw.size} bytes are no whole number of 32-byte star records")
    return raw.view(STAR_DTYPE).copy()


def _spectrum(u, c):
    """The Doppler model's emitted spectrum through (K0, 0), (nu_R, r), (1, g), (nu_B, b), (K4, 0), float64, vectorised over stars."""
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    zero = np.zeros_like(u)
    xa = np.select([u < NU_R, u < 1.0, u < NU_B], [NU_K0, NU_R, 1.0], NU_B)
    xb = np.select([u < NU_R, u < 1.0, u < NU_B], [NU_R, 1.0, NU_B], NU_K4)
    ya = np.select([u < NU_R, u < 1.0, u < NU_B], [zero, r, g], b)
    yb = np.select([u < NU_R, u < 1.0, u < NU_B], [r, g, b], zero)
    t = (u - xa) / (xb - xa)
    out = ya * (1.0 - t) + yb * t
    return np.where((u > NU_K0) & (u < NU_K4), out, 0.0)


def point_source_colour(flags: int, D, rgb) -> np.ndarray:
    """Rule 3 in float64: S_f(D, rgb) of the Doppler model (bit 0 the shift, bit 1 beaming: x D^3 with the shift, x D^4 alone), then
    / D^2 when beaming is set — a point source's flux goes with D (with the shift) or D^2 (bolometric)."""
    D = np.asarray(D, dtype=np.float64)
    c = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    o = c.copy()
    with np.errstate(all="ignore"):
        if flags & 1:
            o = np.stack([_spectrum(NU_R / D, c), _spectrum(1.0 / D, c), _spectrum(NU_B / D, c)], -1)
            if flags & 2:
                o = o * (D ** 3)[:, None]
        elif flags & 2:
            o = c * (D ** 4)[:, None]
        if flags & 2:
            o = o / (D ** 2)[:, None]
    return o


def x_green(temperature) -> np.ndarray:
    """x_G = (h c / k) / (546.1 nm T) in float64, 0 where T is 0 (not a thermal source): what the library uploads, before its rounding
    to float."""
    T = np.asarray(temperature, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(T == 0.0, 0.0, _HC_OVER_K_NM / (WAVELENGTHS_NM[1] * np.where(T == 0.0, 1.0, T)))


def thermal_colour(flags: int, D, rgb, T) -> np.ndarray:
    """T_f(flags, D, rgb, T) in float64, the colour rule of a source with a temperature: with the shift (bit 0), channel k
    is rgb_k expm1(x_k) / expm1(x_k / D), x_k = (h c / k) / (lambda_k T) — for rgb = A blackbody_rgb(T), A times the Planck samples of
    D T on the same scale —, over D^3 unless beaming (bit 1) is set as well.  Without the shift, and for every source whose T is 0, it
    is S_f (point_source_colour before its / D^2).  D (n,), rgb (n, 3), T (n,) or a scalar."""
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    c = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), D.shape)
    with np.errstate(all="ignore"):
        plain = point_source_colour(flags, D, c)
        if flags & 2:
            plain = plain * (D ** 2)[:, None]           # (S_f itself: point_source_colour has divided by D^2)
        if not flags & 1:
            return plain
        nu = np.array([NU_R, 1.0, NU_B])
        x = x_green(np.where(T == 0.0, 1.0, T))[:, None] * nu[None, :]
        y = x / D[:, None]
        q = np.exp(x - y) * (-np.expm1(-x)) / (-np.expm1(-y))
        if not flags & 2:
            q = q / (D ** 3)[:, None]
        o = np.where((D == 1.0)[:, None], c, c * q)
    return np.where((T == 0.0)[:, None], plain, o)


def sky_to_camera(E, interval: int, orientation: Optional[Sequence[float]] = None) -> np.ndarray:
    """Rule 1 in float64: G = (E diag(1, R))^-1, R the orientation's rotation; with interval == 0 the inverse of the spatial block only,
    under a first row and column of the identity."""
    from .renderer import rotation_matrix
    e = np.array(E, dtype=np.float64).reshape(4, 4)
    if orientation is not None:
        turn = np.eye(4)
        turn[1:, 1:] = rotation_matrix(*orientation)
        e = e @ turn
    if interval != 0:
        return np.linalg.inv(e)
    g = np.eye(4)
    g[1:, 1:] = np.linalg.inv(e[1:, 1:])
    return g


def project(catalogue, E, interval: int, camera: Mapping, doppler: int = 0, temperatures=None) -> dict:
    """Rules 1-4 of the star-field pass in float64.  catalogue: STAR_DTYPE records; E: the sky matrix (Renderer.set_environment_frame);
    interval: the scene's (0 = light delay off); camera: a mapping with width and height and
        mode="pinhole" (default), optionally v_fov (the lens; absent or 0: the reference's) — or
        mode="equirect", optionally h_fov, v_fov, yaw (defaults: the full sphere) —
    and optionally orientation=(yaw, pitch, roll); doppler: the flags of Renderer.set_doppler (1 shift, 2 beaming); temperatures: kelvin
    per star as Renderer.set_star_temperatures takes them (0: not thermal), or None: rule 3's S_f becomes thermal_colour.
    Returns a dict of arrays, one entry per star: n (N, 3) the unit camera direction, D the Doppler factor (1 with interval 0),
    rgb (N, 3) the colour after rule 3, X and Y the continuous pixel position (pixel x at X = x for the pinhole, pixel centre at x + 0.5
    for the panorama; NaN where the star is not visible), visible (D finite and > 0, and n.z > 0 for the pinhole)."""
    cat = np.ascontiguousarray(catalogue, dtype=STAR_DTYPE)
    W, H = float(camera["width"]), float(camera["height"])
    mode = camera.get("mode", "pinhole")
    s = np.asarray(cat["dir"], dtype=np.float64)
    s = s / np.linalg.norm(s, axis=1, keepdims=True)
    G = sky_to_camera(E, interval, camera.get("orientation"))
    q = np.concatenate([np.full((len(s), 1), float(interval)), s], axis=1) @ G.T
    with np.errstate(all="ignore"):
        n = q[:, 1:] / np.linalg.norm(q[:, 1:], axis=1, keepdims=True)
        if interval != 0:
            D = q[:, 0] / float(interval)
            visible = np.isfinite(D) & (D > 0.0)
            rgb = point_source_colour(doppler, D, cat["rgb"]) if doppler else np.asarray(cat["rgb"], dtype=np.float64)
            if doppler and temperatures is not None:
                rgb = thermal_colour(doppler, D, cat["rgb"], temperatures)
                if doppler & 2:
                    rgb = rgb / (D ** 2)[:, None]
        else:
            D = np.ones(len(s))
            visible = np.ones(len(s), dtype=bool)
            rgb = np.asarray(cat["rgb"], dtype=np.float64)
        if mode == "equirect":
            h_fov, v_fov, yaw = (float(np.float32(camera.get(k, d))) for k, d in (("h_fov", 2.0 * math.pi), ("v_fov", math.pi), ("yaw", 0.0)))
            lam = np.arctan2(n[:, 0], n[:, 2]) - yaw
            lam = lam - 2.0 * math.pi * np.floor((lam + math.pi) / (2.0 * math.pi))
            phi = np.arcsin(np.clip(n[:, 1], -1.0, 1.0))
            X = W * (lam / h_fov + 0.5) - 0.5
            Y = H * (phi / v_fov + 0.5) - 0.5
        elif mode == "pinhole":
            v_fov = float(camera.get("v_fov", 0.0) or 0.0)
            lens = float(np.float32(math.tan(0.5 * float(np.float32(v_fov))))) if v_fov != 0.0 else 1.0
            visible = visible & (n[:, 2] > 0.0)
            X = W * (0.5 + (0.5 * n[:, 0] / n[:, 2]) / (lens * (W / H)))
            Y = H * (0.5 + (0.5 * n[:, 1] / n[:, 2]) / lens)
        else:
            raise ValueError(f"project: the camera's mode is 'pinhole' or 'equirect', not {mode!r} (a ray map has no inverse)")
    X = np.where(visible, X, np.nan)
    Y = np.where(visible, Y, np.nan)
    return {"n": n, "D": D, "rgb": rgb, "X": X, "Y": Y, "visible": visible}
