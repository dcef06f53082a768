"""Particle sets for the particle pass (include/rpt.h, rpt_set_particles) and a float64 model of where the pass puts them.

A set is a numpy array of PARTICLE_DTYPE: the 32-byte rpt_particle records — `pos`, the particle's position in the REST FRAME of the
scene's object number `object` (the coordinates of an event record's event[1..3]), and `rgb`, its linear colour at rest on the scale of
object colours.  from_arrays, lattice and at_events make one, save / load keep it as raw records (what `rpt_render_main --particles FILE`
reads), Renderer.set_particles and render_scene(..., particles=) take it.  project() is rules 1-4 of the pass in float64: for previews
without a device, and the reference of the physics tests.  Host code only; nothing here touches the GPU."""
from __future__ import annotations

import math
from typing import Mapping, Optional

import numpy as np

from .events import EVENT_DTYPE, _objects_array
from .stars import point_source_colour, thermal_colour

PARTICLE_DTYPE = np.dtype([("pos", "<f4", (3,)), ("object", "<i4"), ("rgb", "<f4", (3,)), ("_pad", "<f4")])
assert PARTICLE_DTYPE.itemsize == 32

INVERSE_SQUARE = 1      # RPT_PARTICLES_INVERSE_SQUARE


def from_arrays(pos, object, rgb) -> np.ndarray:
    """A set from columns: pos (n, 3), object one index or n of them, rgb one colour or n of them."""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(p), dtype=PARTICLE_DTYPE)
    out["pos"] = p
    out["object"] = np.broadcast_to(np.asarray(object, dtype=np.int64).reshape(-1) if np.ndim(object) else int(object), (len(p),))
    out["rgb"] = np.broadcast_to(np.asarray(rgb, dtype=np.float64).reshape(-1, 3), (len(p), 3))
    return out


def lattice(object: int, lo, hi, steps, rgb) -> np.ndarray:
    """steps[0] x steps[1] x steps[2] lamps (one number: the same along every axis) on a regular grid from the corner lo to the corner
    hi, both inclusive, at rest in the frame of `object` — the textbook lattice that shows length contraction and Terrell rotation.
    x varies fastest."""
    n = [int(s) for s in (np.broadcast_to(np.asarray(steps), (3,)))]
    if min(n) < 1:
        raise ValueError("lattice: at least one lamp along every axis")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    axes = [np.linspace(lo[k], hi[k], n[k]) if n[k] > 1 else np.array([0.5 * (lo[k] + hi[k])]) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return from_arrays(np.stack([x, y, z], -1).reshape(-1, 3), object, rgb)


def at_events(records, rgb, stride: int = 1) -> np.ndarray:
    """Particles on the events the hit pixels of an event frame recorded (Renderer.render_events): pos = event[1..3], object = the
    record's, every stride-th hit pixel in memory order.  They sit ON the surfaces the frame sees, at rest with them."""
    rec = np.ascontiguousarray(records, dtype=EVENT_DTYPE).reshape(-1)
    hit = rec[rec["object"] >= 0][::max(1, int(stride))]
    return from_arrays(hit["event"][:, 1:4], hit["object"], rgb)


def save(path, particles) -> None:
    """The raw 32-byte records, one after the other."""
    np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE).tofile(path)


def load(path) -> np.ndarray:
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size % 32:
        raise ValueError(f"{path}: {raw.size} bytes are no whole number of 32-byte particle records")
    return raw.view(PARTICLE_DTYPE).copy()


def window_accepts(t0, t1, t):
    """in(W, t) of DESIGN.md "Time windows": !(t < t0) && !(t >= t1)."""
    return ~(t < t0) & ~(t >= t1)


def project(particles, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0, options: Optional[Mapping] = None,
            windows=None, temperatures=None) -> dict:
    """Rules 1-4 of the particle pass in float64.  particles: PARTICLE_DTYPE records; objects: the Object[] the frames were rendered with
    (a Scene, its objects(), or n x 320 raw bytes — under an orientation the re-based ones of renderer.orient_objects; the camera's
    own `orientation` key is NOT applied here); camera: a mapping with mode="pinhole" (default), optionally v_fov (the lens) — or
    mode="equirect", optionally h_fov, v_fov, yaw; interval: -1 (light delay) or 0; flags: those of Renderer.set_doppler (1 shift,
    2 beaming); options: dict(inverse_square=..., depth_bias=...) as Renderer.set_particle_options takes; windows: (n, 2) {t0, t1} per
    object, or None; temperatures: kelvin per particle as Renderer.set_particle_temperatures takes them (0: not thermal), or None: rule
    3's S_f becomes stars.thermal_colour.  Returns a dict of arrays, one entry per particle: visible, X and Y (pixel x at X = x for the pinhole, pixel centre
    at x + 0.5 for the panorama; NaN where not visible), dist (the camera-frame distance, what rpt_event.dist measures), r (the
    rest-frame distance), D (dist / r; 1 with interval 0), te (the emission time in the object's rest frame), k (N, 4) the emission
    event's displacement from the camera event in the camera frame, n (N, 3) and rgb (N, 3) the colour after rule 3."""
    if interval not in (-1, 0):
        raise ValueError("project: the light cone has a closed form for interval -1 and 0 only")
    p = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE).reshape(-1)
    return project_columns(p["pos"].astype(np.float64), p["object"].astype(np.int64), p["rgb"].astype(np.float64), objects, camera, W, H,
                           interval, flags, options, windows, temperatures)


def project_columns(pos, idx, rgb0, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0,
                    options: Optional[Mapping] = None, windows=None, temperatures=None) -> dict:
    """project() on float64 columns — pos (N, 3), idx (N,) object indices, rgb0 (N, 3) — for positions that are no float32 numbers
    (segments.project's nodes)."""
    options = dict(options or {})
    objs = _objects_array(objects)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(objs)):
        raise ValueError(f"project: a particle names object {int(idx.max())}, the Object[] holds {len(objs)}")
    inv = objs["InvLorentz"].astype(np.float64).reshape(-1, 4, 4)[idx]
    cam = objs["stationaryCam"].astype(np.float64).reshape(-1, 4)[idx]
    with np.errstate(all="ignore"):
        w = pos - cam[:, 1:]
        r = np.sqrt((w * w).sum(axis=1))
        visible = (r > 0.0) & np.isfinite(r)
        tau = -r if interval == -1 else -(inv[:, 0, 1:] * w).sum(axis=1) / inv[:, 0, 0]
        k = np.einsum("nij,nj->ni", inv, np.concatenate([tau[:, None], w], axis=1))
        dist = np.sqrt((k[:, 1:] ** 2).sum(axis=1))
        visible &= (dist > 0.0) & np.isfinite(dist)
        n = k[:, 1:] / dist[:, None]
        te = cam[:, 0] + tau
        if windows is not None:
            win = np.asarray(windows, dtype=np.float64).reshape(-1, 2)[idx]
            visible &= window_accepts(win[:, 0], win[:, 1], te)
        if flags and interval != 0:
            D = dist / r
            visible &= (D > 0.0) & np.isfinite(D)
            rgb = point_source_colour(flags, D, rgb0)
            if temperatures is not None:
                rgb = thermal_colour(flags, D, rgb0, temperatures)
                if flags & 2:
                    rgb = rgb / (D ** 2)[:, None]
        else:
            D = dist / r if interval != 0 else np.ones(len(idx))
            rgb = rgb0.copy()
        if options.get("inverse_square"):
            rgb = rgb / (r * r)[:, None]
        mode = camera.get("mode", "pinhole")
        if mode == "equirect":
            h_fov, v_fov, yaw = (float(np.float32(camera.get(key, d))) for key, d in (("h_fov", 2.0 * math.pi), ("v_fov", math.pi), ("yaw", 0.0)))
            lam = np.arctan2(n[:, 0], n[:, 2]) - yaw
            lam = lam - 2.0 * math.pi * np.floor((lam + math.pi) / (2.0 * math.pi))
            phi = np.arcsin(np.clip(n[:, 1], -1.0, 1.0))
            X = W * (lam / h_fov + 0.5) - 0.5
            Y = H * (phi / v_fov + 0.5) - 0.5
        elif mode == "pinhole":
            v_fov = float(camera.get("v_fov", 0.0) or 0.0)
            lens = float(np.float32(math.tan(0.5 * float(np.float32(v_fov))))) if v_fov != 0.0 else 1.0
            visible &= n[:, 2] > 0.0
            X = W * (0.5 + (0.5 * n[:, 0] / n[:, 2]) / (lens * (float(W) / float(H))))
            Y = H * (0.5 + (0.5 * n[:, 1] / n[:, 2]) / lens)
        else:
            raise ValueError(f"project: the camera's mode is 'pinhole' or 'equirect', not {mode!r} (a ray map has no inverse)")
        visible &= (np.abs(X) < 1e9) & (np.abs(Y) < 1e9)
    X = np.where(visible, X, np.nan)
    Y = np.where(visible, Y, np.nan)
    return {"visible": visible, "X": X, "Y": Y, "dist": dist, "r": r, "D": D, "te": te, "k": k, "n": n, "rgb": rgb}
