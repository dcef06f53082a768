"""Ballistic sets for the ballistic pass (include/rpt.h, rpt_set_ballistics) and a float64 model of where the pass puts them.

A set is a numpy array of BALLISTIC_DTYPE: the 48-byte rpt_ballistic records — `pos`, where the particle is at time 0 of the rest-frame
clock of the scene's object number `object`, `u`, its proper velocity gamma * beta in that frame, `t0` and `t1`, the window of that clock
in which it shines, and `rgb`, its linear colour at rest in its OWN frame.  The object is only the frame the worldline is written in: the
particle does not ride it.  from_arrays, jet and shell make a set, save / load keep it as raw records (what `rpt_render_main --ballistics
FILE` reads), Renderer.set_ballistics and render_scene(..., ballistics=) take it.  project() is rules 1-6 of the pass in float64: for
previews without a device, and the reference of the physics tests.  Host code only; nothing here touches the GPU."""
from __future__ import annotations

import math
from typing import Mapping, Optional

import numpy as np

from .events import _objects_array
from .particles import window_accepts
from .stars import point_source_colour, thermal_colour

BALLISTIC_DTYPE = np.dtype([("pos", "<f4", (3,)), ("object", "<i4"), ("rgb", "<f4", (3,)), ("t0", "<f4"), ("u", "<f4", (3,)), ("t1", "<f4")])
assert BALLISTIC_DTYPE.itemsize == 48

INVERSE_SQUARE = 1      # RPT_PARTICLES_INVERSE_SQUARE, which rpt_set_ballistic_options reuses


def proper_velocity(beta) -> np.ndarray:
    """u = gamma * beta for velocities beta (..., 3) in units of c, |beta| < 1."""
    b = np.asarray(beta, dtype=np.float64)
    b2 = (b * b).sum(axis=-1, keepdims=True)
    if (b2 >= 1.0).any():
        raise ValueError("proper_velocity: |beta| must be below 1")
    return b / np.sqrt(1.0 - b2)


def from_arrays(pos, object, rgb, beta=None, u=None, t0=-math.inf, t1=math.inf, epoch=0.0) -> np.ndarray:
    """A set from columns: pos (n, 3), where each particle is at the object's time `epoch` (one number or n); object one index or n of
    them; rgb one colour or n; the velocity as beta (units of c) or as the proper velocity u = gamma * beta, one vector or n (neither:
    at rest); t0, t1 one number or n.  Stored: pos - beta * epoch, the place at time 0."""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if beta is not None and u is not None:
        raise ValueError("from_arrays: give beta or u, not both")
    if beta is not None:
        u = proper_velocity(np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1, 3), (n, 3)))
    u = np.broadcast_to(np.zeros(3) if u is None else np.asarray(u, dtype=np.float64).reshape(-1, 3), (n, 3))
    b = u / np.sqrt(1.0 + (u * u).sum(axis=1))[:, None]
    out = np.zeros(n, dtype=BALLISTIC_DTYPE)
    out["pos"] = p - b * np.broadcast_to(np.asarray(epoch, dtype=np.float64).reshape(-1), (n,))[:, None]
    out["object"] = np.broadcast_to(np.asarray(object, dtype=np.int64).reshape(-1) if np.ndim(object) else int(object), (n,))
    out["rgb"] = np.broadcast_to(np.asarray(rgb, dtype=np.float64).reshape(-1, 3), (n, 3))
    out["u"] = u
    out["t0"] = np.broadcast_to(np.asarray(t0, dtype=np.float64).reshape(-1), (n,))
    out["t1"] = np.broadcast_to(np.asarray(t1, dtype=np.float64).reshape(-1), (n,))
    return out


def jet(object: int, origin, direction, beta: float, emit_times, rgb) -> np.ndarray:
    """Blobs that leave `origin` at the object's times emit_times and fly along `direction` at beta (units of c): one record per
    time, each shining from the moment it leaves — the textbook jet whose blobs seem to cross the sky faster than light."""
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    d = d / np.linalg.norm(d)
    t = np.asarray(emit_times, dtype=np.float64).reshape(-1)
    return from_arrays(np.broadcast_to(np.asarray(origin, dtype=np.float64).reshape(3), (len(t), 3)), object, rgb, beta=float(beta) * d, t0=t, epoch=t)


def shell(object: int, centre, t_emit: float, beta: float, n: int, rgb) -> np.ndarray:
    """n particles that leave `centre` at the object's time t_emit in evenly spread directions (a Fibonacci spiral on the sphere), all
    at beta: an exploding shell, a sphere of radius beta (t - t_emit) in that frame, shining from t_emit on."""
    if int(n) < 1:
        raise ValueError("shell: at least one particle")
    i = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / float(n)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    dirs = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return from_arrays(np.broadcast_to(np.asarray(centre, dtype=np.float64).reshape(3), (int(n), 3)), object, rgb, beta=float(beta) * dirs,
                       t0=float(t_emit), epoch=float(t_emit))


def save(path, ballistics) -> None:
    """The raw 48-byte records, one after the other."""
    np.ascontiguousarray(ballistics, dtype=BALLISTIC_DTYPE).tofile(path)


def load(path) -> np.ndarray:
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size % 48:
        raise ValueError(f"{path}: {raw.size} bytes are no whole number of 48-byte ballistic records")
    return raw.view(BALLISTIC_DTYPE).copy()


def apparent_velocity(beta: float, theta: float) -> float:
    """The textbook transverse apparent velocity, in units of c, of a source moving at beta at the angle theta (radians) to the line
    of sight, towards the observer for theta < pi / 2: beta sin(theta) / (1 - beta cos(theta)).  Above 1 for beta > 1 / sqrt(2) at the
    right angles."""
    return beta * math.sin(theta) / (1.0 - beta * math.cos(theta))


def _frames(objects):
    """(InvLorentz (n, 4, 4), stationaryCam (n, 4)) in float64: from a mapping that holds them under those names — matrices that need
    not be float32 numbers — or from whatever particles.project takes."""
    if isinstance(objects, Mapping):
        return np.asarray(objects["InvLorentz"], dtype=np.float64).reshape(-1, 4, 4), np.asarray(objects["stationaryCam"], dtype=np.float64).reshape(-1, 4)
    objs = _objects_array(objects)
    return objs["InvLorentz"].astype(np.float64).reshape(-1, 4, 4), objs["stationaryCam"].astype(np.float64).reshape(-1, 4)


def seen_from_emission(visible, inv, tau, w, r, rgb0, camera: Mapping, W: int, H: int, interval: int, flags: int, options: Mapping, temperatures) -> dict:
    """Rules 5-7 of the ballistic pass in float64, shared with rockets.project: the emission event (tau, w) (N,), (N, 3) from the camera
    event in the object's frame, r (N,) the camera's distance in the source's rest frame, `visible` what is not skipped so far.  Returns
    visible, X, Y, dist, D, k, n, rgb."""
    with np.errstate(all="ignore"):
        k = np.einsum("nij,nj->ni", inv, np.concatenate([tau[:, None], w], axis=1))
        dist = np.sqrt((k[:, 1:] ** 2).sum(axis=1))
        visible &= (dist > 0.0) & np.isfinite(dist)
        n = k[:, 1:] / dist[:, None]
        if flags and interval != 0:
            D = dist / r
            visible &= (D > 0.0) & np.isfinite(D)
            rgb = point_source_colour(flags, D, rgb0)
            if temperatures is not None:
                rgb = thermal_colour(flags, D, rgb0, temperatures)
                if flags & 2:
                    rgb = rgb / (D ** 2)[:, None]
        else:
            D = dist / r if interval != 0 else np.ones(len(tau))
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
    return {"visible": visible, "X": X, "Y": Y, "dist": dist, "D": D, "k": k, "n": n, "rgb": rgb}


def project(ballistics, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0, options: Optional[Mapping] = None,
            temperatures=None) -> dict:
    """Rules 1-6 of the ballistic pass in float64.  ballistics: BALLISTIC_DTYPE records; objects, camera, interval, flags, options,
    temperatures: as particles.project takes them (objects may also be a mapping with float64 "InvLorentz" (n, 4, 4) and
    "stationaryCam" (n, 4)); there are no object windows: a record has its own.  Returns a dict of arrays, one entry per record, shaped
    as particles.project's: visible, X, Y, dist, r — here r', the camera's distance in the particle's OWN rest frame —, D (dist / r';
    1 with interval 0), te (the emission time on the object's clock), k (N, 4), n (N, 3), rgb (N, 3); and a (u . w0: <= 0 for a
    particle that approaches), tau, pos_e (N, 3) where the particle is at te, in the object's frame."""
    if interval not in (-1, 0):
        raise ValueError("project: the light cone has a closed form for interval -1 and 0 only")
    p = np.ascontiguousarray(ballistics, dtype=BALLISTIC_DTYPE).reshape(-1)
    return project_columns(p["pos"].astype(np.float64), p["object"].astype(np.int64), p["rgb"].astype(np.float64), p["u"].astype(np.float64),
                           p["t0"].astype(np.float64), p["t1"].astype(np.float64), objects, camera, W, H, interval, flags, options, temperatures)


def project_columns(pos, idx, rgb0, u, t0, t1, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0,
                    options: Optional[Mapping] = None, temperatures=None) -> dict:
    """project() on float64 columns — pos (N, 3), idx (N,) object indices, rgb0 (N, 3), u (N, 3), t0 and t1 (N,) — for worldlines whose
    numbers are no float32 numbers (one written in another frame, by a float64 change of frame)."""
    options = dict(options or {})
    invs, cams = _frames(objects)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(invs)):
        raise ValueError(f"project: a record names object {int(idx.max())}, the Object[] holds {len(invs)}")
    inv, cam = invs[idx], cams[idx]
    with np.errstate(all="ignore"):
        g = np.sqrt(1.0 + (u * u).sum(axis=1))
        beta = u / g[:, None]
        w0 = (pos + beta * cam[:, :1]) - cam[:, 1:]
        ww = (w0 * w0).sum(axis=1)
        a = (u * w0).sum(axis=1)
        r = np.sqrt(ww + a * a)
        visible = (r > 0.0) & np.isfinite(r)
        if interval == -1:
            tau = np.where(a <= 0.0, g * (a - r), -(g * ww) / (a + r))
        else:
            tau = -(inv[:, 0, 1:] * w0).sum(axis=1) / (inv[:, 0, 0] + (inv[:, 0, 1:] * beta).sum(axis=1))
        w = w0 + beta * tau[:, None]
        te = cam[:, 0] + tau
        visible &= window_accepts(t0, t1, te)
    seen = seen_from_emission(visible, inv, tau, w, r, rgb0, camera, W, H, interval, flags, options, temperatures)
    return dict(seen, r=r, te=te, a=a, tau=tau, pos_e=w + cam[:, 1:])
