"""Host-side helpers for the per-pixel event records of Renderer.render_events (include/rpt_layout.h: rpt_event; DESIGN.md "Event
pass").  numpy only: nothing here touches a device or a library.  float64 throughout, except `overlay`, which restates the overlay
pass's float32 and integer rules exactly (include/rpt.h, rpt_set_overlay; DESIGN.md "Overlay pass").

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


# the layer bits of include/rpt.h (RPT_OVERLAY_*)
OVERLAY_OUTLINES, OVERLAY_ISO_DELAY, OVERLAY_ISO_CLOCK, OVERLAY_LATTICE, OVERLAY_DELAY_TINT = 1, 2, 4, 8, 16
OVERLAY_DEFAULTS = dict(outlines=False, outline_rgba=(255, 255, 255, 255), delay_step=None, delay_rgba=(255, 255, 0, 255),
                        clock_step=None, clock_rgba=(0, 255, 255, 255), lattice_step=None, lattice_rgba=(255, 0, 255, 255),
                        tint=False, tint_t_max=0.0, tint_alpha=128)


def overlay_settings(**layers) -> dict:
    """The keyword form of an overlay description, shared by `overlay` and Renderer.set_overlay, with every default filled in:
    outlines (bool) / outline_rgba; delay_step (None = off) / delay_rgba; clock_step / clock_rgba; lattice_step — None, one step for
    all three axes or (sx, sy, sz) with 0 skipping an axis — / lattice_rgba; tint (bool) / tint_t_max (0 = the frame's largest delay) /
    tint_alpha.  Colours are (R, G, B, A) in 0..255, A being the weight the layer is blended with.  The result also holds `layers`, the
    OR of the RPT_OVERLAY_* bits that are on.  Unknown keywords raise TypeError; the values are checked where they are used."""
    unknown = set(layers) - set(OVERLAY_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown overlay keyword(s): {sorted(unknown)}")
    s = dict(OVERLAY_DEFAULTS, **layers)
    lat = s["lattice_step"]
    if lat is not None:
        lat = tuple(float(v) for v in (lat if np.ndim(lat) else (lat,) * 3))
        if len(lat) != 3:
            raise ValueError("lattice_step is one step or three (sx, sy, sz)")
    s["lattice_step"] = lat
    for key in ("outline_rgba", "delay_rgba", "clock_rgba", "lattice_rgba"):
        c = tuple(int(v) for v in s[key])
        if len(c) != 4 or min(c) < 0 or max(c) > 255:
            raise ValueError(f"{key} is (R, G, B, A) in 0..255")
        s[key] = c
    if not 0 <= int(s["tint_alpha"]) <= 255:
        raise ValueError("tint_alpha is 0..255")
    s["layers"] = ((OVERLAY_OUTLINES if s["outlines"] else 0) | (OVERLAY_ISO_DELAY if s["delay_step"] is not None else 0)
                   | (OVERLAY_ISO_CLOCK if s["clock_step"] is not None else 0) | (OVERLAY_LATTICE if lat is not None else 0)
                   | (OVERLAY_DELAY_TINT if s["tint"] else 0))
    return s


def _step_inverse(step, what: str) -> np.float32:
    step = np.float32(step)
    if not (np.isfinite(step) and step > 0):
        raise ValueError(f"{what} must be finite and > 0")
    return np.float32(1.0) / step


def _on_contour(s: np.ndarray, inv: np.float32, obj: np.ndarray) -> np.ndarray:
    """The contour rule for one scalar plane (before the "hit pixel" clause): cell = floor(s * inv) in float32; True where the right
    or the upper neighbour inside the frame has the same object and another cell, both products being finite and below 2^30."""
    with np.errstate(all="ignore"):
        p = s.astype(np.float32) * inv
        valid = np.abs(p) < np.float32(2.0 ** 30)                       # (False for a NaN)
    cell = np.floor(np.where(valid, p, np.float32(0))).astype(np.int64)
    on = np.zeros(s.shape, dtype=bool)
    on[:, :-1] |= valid[:, :-1] & valid[:, 1:] & (obj[:, :-1] == obj[:, 1:]) & (cell[:, :-1] != cell[:, 1:])
    on[:-1] |= valid[:-1] & valid[1:] & (obj[:-1] == obj[1:]) & (cell[:-1] != cell[1:])
    return on


def _blend(img: np.ndarray, mask: np.ndarray, rgb, alpha: int) -> None:
    """out = (c * a + old * (255 - a) + 127) // 255 on R, G, B of the pixels in `mask`, in place; the fourth byte stays."""
    old = img[..., :3].astype(np.uint32)
    c = np.asarray(rgb, dtype=np.uint32)[..., :3]
    a = np.uint32(alpha)
    out = (c * a + old * (np.uint32(255) - a) + np.uint32(127)) // np.uint32(255)
    img[..., :3] = np.where(mask[..., None], out, old).astype(np.uint8)


def overlay(frame_rgba: np.ndarray, events: np.ndarray, interval: int, **layers):
    """The overlay pass (Renderer.render_overlay; include/rpt.h, rpt_set_overlay) in numpy, byte for byte: float32 products, np.floor
    and integer blends.  frame_rgba: the H x W x 4 uint8 colours of the frame (any shape of H W 4 bytes, e.g. read_framebuffer()["rgba"]);
    events: the (H, W) records of the same view, row 0 the bottom row as everywhere; interval: -1 or 0, the frame's; the layers as
    keywords (overlay_settings).  Returns (the H x W x 4 uint8 result, the number of pixels whose RGBA changed).  The layers go on in
    the pass's order — tint, lattice, clock, delay, outlines — so applying it twice blends twice, as the pass does."""
    s = overlay_settings(**layers)
    ev = np.asarray(events)
    if ev.ndim != 2:
        raise ValueError("events is the (H, W) array of records")
    before = np.ascontiguousarray(frame_rgba, dtype=np.uint8).reshape(ev.shape + (4,))
    img = before.copy()
    obj = ev["object"]
    hit = obj >= 0
    with np.errstate(all="ignore"):
        delay = np.abs(np.float32(interval) * ev["dist"].astype(np.float32))
    if s["tint"]:
        t_max = np.float32(s["tint_t_max"])
        if not (np.isfinite(t_max) and t_max >= 0):
            raise ValueError("tint_t_max is > 0, or 0 for the frame's largest delay")
        d = np.where(np.isfinite(delay), delay, np.float32(0))
        if t_max == 0:
            t_max = d[hit].max() if hit.any() else np.float32(0)
        x = np.clip(d / t_max, np.float32(0), np.float32(1)) if t_max > 0 else np.zeros_like(d)
        x2 = np.float32(2) * x
        ramp = np.stack([np.clip(np.float32(1) - x2, np.float32(0), np.float32(1)), np.float32(1) - np.abs(x2 - np.float32(1)),
                         np.clip(x2 - np.float32(1), np.float32(0), np.float32(1))], -1)
        rgb = np.rint((np.float32(0.25) + np.float32(0.75) * ramp) * np.float32(255))
        assert rgb.dtype == np.float32
        _blend(img, hit, rgb.astype(np.uint32), int(s["tint_alpha"]))
    if s["lattice_step"] is not None:
        if not any(s["lattice_step"]):
            raise ValueError("the lattice needs a step > 0 on at least one axis")
        on = np.zeros(ev.shape, dtype=bool)
        for axis, step in enumerate(s["lattice_step"]):
            if step != 0:
                on |= _on_contour(ev["event"][..., 1 + axis], _step_inverse(step, "a lattice step that is not 0"), obj)
        _blend(img, on & hit, s["lattice_rgba"], s["lattice_rgba"][3])
    if s["clock_step"] is not None:
        _blend(img, _on_contour(ev["event"][..., 0], _step_inverse(s["clock_step"], "clock_step"), obj) & hit, s["clock_rgba"], s["clock_rgba"][3])
    if s["delay_step"] is not None:
        _blend(img, _on_contour(delay, _step_inverse(s["delay_step"], "delay_step"), obj) & hit, s["delay_rgba"], s["delay_rgba"][3])
    if s["outlines"]:
        on = np.zeros(ev.shape, dtype=bool)
        on[:, :-1] |= obj[:, :-1] != obj[:, 1:]
        on[:-1] |= obj[:-1] != obj[1:]
        _blend(img, on, s["outline_rgba"], s["outline_rgba"][3])
    return img, int((img != before).any(axis=-1).sum())
