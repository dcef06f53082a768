"""Host-side helpers for the per-pixel event records of Renderer.render_events (include/rpt_layout.h: rpt_event; DESIGN.md "Event
pass").  numpy only, float64 throughout: nothing here touches a device or a library.

A record holds, for the closest hit of a pixel's primary ray, the object's index, the camera-frame distance `dist`, the emission event
(t, x, y, z) in the HIT OBJECT'S rest frame and the surface (u, v); object == -1 marks a miss (every other field 0).
"""
from __future__ import annotations

import numpy as np

EVENT_DTYPE = np.dtype([("object", "<i4"), ("dist", "<f4"), ("event", "<f4", (4,)), ("uv", "<f4", (2,))])
assert EVENT_DTYPE.itemsize == 32


def _objects_array(objects) -> np.ndarray:
    """Object[] as the structured array of scene.OBJECT_DTYPE, from a Scene, that array, or n x 320 raw bytes."""
    from .scene import OBJECT_DTYPE, Scene
    if isinstance(objects, Scene):
        return objects.objects()
    arr = np.ascontiguousarray(objects)
    if arr.dtype == OBJECT_DTYPE:
        return arr.reshape(-1)
    return arr.view(np.uint8).reshape(-1).view(OBJECT_DTYPE)


def look_back_time(events: np.ndarray, interval: int) -> np.ndarray:
    """interval * dist per pixel, float64: the camera-frame time of the emission relative to the camera event — -dist with light
    propagation on (interval -1), 0 with it off.  NaN on a miss."""
    ev = np.asarray(events)
    t = float(interval) * ev["dist"].astype(np.float64)
    return np.where(ev["object"] >= 0, t, np.nan)


def camera_frame_events(events: np.ndarray, objects) -> np.ndarray:
    """Every hit pixel's event taken back to the camera frame by its hit object's InvLorentz: (..., 4) float64 (dt, dx, dy, dz), the
    DISPLACEMENT from the camera event — InvLorentz (event - stationaryCam), stationaryCam being the camera event in the object's rest
    frame.  For a light-like look-back path |dx| = |dt| = dist.  NaN on a miss.  objects: the Object[] the pass was rendered with (a
    Scene, its objects(), or raw bytes; under an orientation the re-based ones of Renderer.orient_objects)."""
    ev = np.asarray(events)
    objs = _objects_array(objects)
    out = np.full(ev.shape + (4,), np.nan, dtype=np.float64)
    hit = ev["object"] >= 0
    if hit.any():
        idx = ev["object"][hit]
        inv = objs["InvLorentz"].astype(np.float64)[idx]              # (n, 4, 4), rows t, x, y, z
        e = ev["event"][hit].astype(np.float64) - objs["stationaryCam"].astype(np.float64)[idx]
        out[hit] = np.einsum("nij,nj->ni", inv, e)
    return out


def scene_frame_events(events: np.ndarray, objects, camera_inv_lorentz) -> np.ndarray:
    """camera_frame_events taken on through the camera's inverse boost (Scene.camera_lorentz()[1]) into the scene's rest frame:
    (..., 4) float64 displacement from the camera event in scene coordinates.  NaN on a miss."""
    cam = camera_frame_events(events, objects)
    m = np.asarray(camera_inv_lorentz, dtype=np.float64).reshape(4, 4)
    return cam @ m.T


def delay_map(events: np.ndarray, interval: int, band: float = 1.0, t_max: float | None = None) -> np.ndarray:
    """False-colour image of the look-back time: (..., 3) uint8.  The hue runs from near (red) to far (blue) over [0, t_max] (default:
    the largest delay of the frame); every `band` units of delay an isochrone — the tenth of each band next to its boundary is drawn
    dark.  Equal look-back times get equal colours; misses are black.  With light propagation off every hit is one colour."""
    ev = np.asarray(events)
    hit = ev["object"] >= 0
    delay = np.abs(np.where(hit, float(interval) * ev["dist"].astype(np.float64), 0.0))
    delay = np.where(np.isfinite(delay), delay, 0.0)
    top = float(t_max) if t_max is not None else (float(delay[hit].max()) if hit.any() else 0.0)
    x = np.clip(delay / top, 0.0, 1.0) if top > 0.0 else np.zeros_like(delay)
    # a three-knot ramp red -> green -> blue, linear in between
    r = np.clip(1.0 - 2.0 * x, 0.0, 1.0)
    g = 1.0 - np.abs(2.0 * x - 1.0)
    b = np.clip(2.0 * x - 1.0, 0.0, 1.0)
    rgb = np.stack([r, g, b], -1)
    rgb = 0.25 + 0.75 * rgb
    if band > 0.0:
        phase = delay / float(band) - np.floor(delay / float(band))
        rgb = np.where((phase < 0.1)[..., None], rgb * 0.35, rgb)
    out = np.round(rgb * 255.0).astype(np.uint8)
    out[~hit] = 0
    return out
