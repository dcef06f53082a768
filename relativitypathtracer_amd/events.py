"""Host-side helpers for the per-pixel event records of Renderer.render_events (include/rpt_layout.h: rpt_event; DESIGN.md "Event
pass").  numpy only: nothing here touches a device or a library.  float64 throughout, except `overlay`, which restates the overlay
pass's float32 and integer rules exactly (include/rpt.h, rpt_set_overlay; DESIGN.md "Overlay pass"), and `readout`, which does the
same for the readout pass (rpt_set_readouts; DESIGN.md "Readout pass").

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


# ---- the readout pass (include/rpt.h, rpt_set_readouts; DESIGN.md "Readout pass") ------------------------------------------------------
# segments a..g and the decimal point: (x0, x1, y0, y1) in sixteenths of a character cell; bit k of a cell's mask lights row k
READOUT_SEGMENTS = ((3, 11, 13, 15), (10, 12, 8, 14), (10, 12, 2, 8), (3, 11, 1, 3), (2, 4, 2, 8), (2, 4, 8, 14), (3, 11, 7, 9), (13, 15, 1, 3))
READOUT_DIGIT_MASKS = (0x3f, 0x06, 0x5b, 0x4f, 0x66, 0x6d, 0x7d, 0x07, 0x7f, 0x6f)
READOUT_SUBSAMPLES = (-0.375, -0.125, 0.125, 0.375)
READOUT_DEFAULT_RECT = (0.1, 0.25, 0.9, 0.75)


def readout_settings(rate=1.0, offset=0.0, digits=0, decimals=0, rect=READOUT_DEFAULT_RECT, on_rgba=(255, 0, 0, 255), off_rgba=(0, 0, 0, 160)) -> dict:
    """One object's display, validated as rpt_set_readouts validates it (ValueError where the library returns RPT_ERR_ARG): the value
    shown is offset + rate * event[0] with `decimals` places in `digits` character cells (0 = this object has no display), inside
    rect = (u0, v0, u1, v1) of the hit's (u, v) (u0 > u1 or v0 > v1 mirrors it); lit segments are blended with on_rgba, the rest of the
    rectangle with off_rgba, both (R, G, B, A) in 0..255 (A = 0 leaves the picture).  The floats are rounded to float32 here."""
    digits, decimals = int(digits), int(decimals)
    rect = tuple(rect)
    if len(rect) != 4:
        raise ValueError("rect is (u0, v0, u1, v1)")
    floats = [np.float32(f) for f in (rate, offset) + rect]
    if not all(np.isfinite(f) for f in floats):
        raise ValueError("rate, offset and the rectangle must be finite")
    if not 0 <= digits <= 9:
        raise ValueError("digits is 0 (no display) or 1..9")
    if digits and not (0 <= decimals <= 6 and decimals < digits):
        raise ValueError("decimals is 0..6 and below digits")
    if digits and (floats[2] == floats[4] or floats[3] == floats[5]):
        raise ValueError("the rectangle is empty: u0 == u1 or v0 == v1")
    colours = []
    for name, c in (("on_rgba", on_rgba), ("off_rgba", off_rgba)):
        c = tuple(int(b) for b in c)
        if len(c) != 4 or min(c) < 0 or max(c) > 255:
            raise ValueError(f"{name} is (R, G, B, A) in 0..255")
        colours.append(c)
    return dict(rate=floats[0], offset=floats[1], digits=digits, decimals=decimals, rect=tuple(floats[2:]), on_rgba=colours[0], off_rgba=colours[1])


def _readout_coverage(events: np.ndarray, readouts):
    """(shown, n_in, n_on, value) per pixel: whether the pixel is a hit of an object with a display, how many of its 16 sub-samples lie
    inside the rectangle and how many on a lit segment, and the scaled value sv the pixel shows (NaN where not shown)."""
    ev = np.asarray(events)
    if ev.ndim != 2:
        raise ValueError("events is the (H, W) array of records")
    f32 = np.float32
    table = [readout_settings(**d) if d is not None else None for d in (readouts or [])]
    obj = ev["object"]
    if obj.size and int(obj.max()) >= len(table) and table:
        raise ValueError(f"the records hold object {int(obj.max())}; readouts has {len(table)} entries (one per object)")
    n = max(len(table), 1)
    per = {k: np.zeros(n, dtype=f32) for k in ("rate", "offset", "scale", "u0", "v0", "inv_w", "inv_h")}
    digits_of, decimals_of = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for k, d in enumerate(table):
        if d is None or d["digits"] == 0:
            continue
        u0, v0, u1, v1 = d["rect"]
        per["rate"][k], per["offset"][k], per["scale"][k] = d["rate"], d["offset"], f32(10 ** d["decimals"])
        per["u0"][k], per["v0"][k] = u0, v0
        per["inv_w"][k], per["inv_h"][k] = f32(1.0) / (u1 - u0), f32(1.0) / (v1 - v0)
        digits_of[k], decimals_of[k] = d["digits"], d["decimals"]
    o = np.clip(obj, 0, n - 1)
    digits, decimals = digits_of[o], decimals_of[o]
    shown = (obj >= 0) & (obj < len(table)) & (digits != 0)
    u, v, e = ev["uv"][..., 0].astype(f32), ev["uv"][..., 1].astype(f32), ev["event"][..., 0].astype(f32)
    with np.errstate(all="ignore"):
        # the value and the nine cells' masks
        sv = (per["rate"][o] * e + per["offset"][o]) * per["scale"][o]
        assert sv.dtype == f32
        neg = sv < 0
        over = ~(np.abs(sv) < f32(1e9))
        mag = np.floor(np.where(over, f32(0), np.abs(sv))).astype(np.int64)
        over |= mag >= 10 ** np.maximum(digits - neg, 0)
        masks = np.zeros(ev.shape + (9,), dtype=np.int64)
        digit_masks = np.array(READOUT_DIGIT_MASKS, dtype=np.int64)
        for k in range(9):
            m = digit_masks[(mag // 10 ** np.maximum(digits - 1 - k, 0)) % 10]
            if k == 0:
                m = np.where(neg, 0x40, m)
            m = m | np.where((decimals > 0) & (k == digits - 1 - decimals), 0x80, 0)
            masks[..., k] = np.where(over, 0x40, m)
        # the footprint: differences to the right and the upper neighbour of the same object, 0 at an edge
        du_x, dv_x, du_y, dv_y = (np.zeros(ev.shape, dtype=f32) for _ in range(4))
        same = obj[:, :-1] == obj[:, 1:]
        du_x[:, :-1] = np.where(same, u[:, 1:] - u[:, :-1], f32(0))
        dv_x[:, :-1] = np.where(same, v[:, 1:] - v[:, :-1], f32(0))
        same = obj[:-1] == obj[1:]
        du_y[:-1] = np.where(same, u[1:] - u[:-1], f32(0))
        dv_y[:-1] = np.where(same, v[1:] - v[:-1], f32(0))
        n_in, n_on = np.zeros(ev.shape, dtype=np.int64), np.zeros(ev.shape, dtype=np.int64)
        fdigits = digits.astype(f32)
        for ai in READOUT_SUBSAMPLES:
            for aj in READOUT_SUBSAMPLES:
                us = (u + f32(ai) * du_x) + f32(aj) * du_y
                vs = (v + f32(ai) * dv_x) + f32(aj) * dv_y
                s = (us - per["u0"][o]) * per["inv_w"][o]
                t = (vs - per["v0"][o]) * per["inv_h"][o]
                assert s.dtype == f32 and t.dtype == f32
                inside = shown & (s >= 0) & (s < 1) & (t >= 0) & (t < 1)
                cs = np.where(inside, s, f32(0)) * fdigits
                c = np.minimum(np.floor(cs).astype(np.int64), np.maximum(digits - 1, 0))
                lx = cs - c.astype(f32)
                mask = np.take_along_axis(masks, c[..., None], axis=-1)[..., 0]
                lit = np.zeros(ev.shape, dtype=bool)
                for bit, (x0, x1, y0, y1) in enumerate(READOUT_SEGMENTS):
                    lit |= ((mask >> bit) & 1).astype(bool) & (lx >= f32(x0 / 16)) & (lx < f32(x1 / 16)) & (t >= f32(y0 / 16)) & (t < f32(y1 / 16))
                n_in += inside
                n_on += inside & lit
    return shown, n_in, n_on, np.where(shown, sv, f32(np.nan)), table, o


def readout_coverage(events: np.ndarray, readouts):
    """What the readout pass sees per pixel of the (H, W) records, before it blends: (shown, n_in, n_on, value) — bool: the pixel hits
    an object that has a display; the number of its 16 sub-samples inside the display's rectangle and on a lit segment; float32: the
    scaled value (rate * event[0] + offset) * 10^decimals it shows, NaN where not shown."""
    return _readout_coverage(events, readouts)[:4]


def readout(frame_rgba: np.ndarray, events: np.ndarray, readouts):
    """The readout pass (Renderer.render_readouts; include/rpt.h, rpt_set_readouts) in numpy, byte for byte: seven-segment displays on
    the objects' surfaces that show offset + rate * event[0], the hit object's own time when it emitted the light the pixel receives.
    frame_rgba: the H x W x 4 uint8 colours of the frame; events: the (H, W) records of the same view; readouts: one entry per object,
    None or the keywords of readout_settings as a dict.  Returns (the H x W x 4 uint8 result, the number of pixels whose RGBA changed).
    The value is per PIXEL: across a large moving face neighbouring pixels may show different values — the relativity of simultaneity."""
    shown, n_in, n_on, _, table, o = _readout_coverage(events, readouts)
    before = np.ascontiguousarray(frame_rgba, dtype=np.uint8).reshape(shown.shape + (4,))
    img = before.copy()
    if not table:
        return img, 0
    on = np.array([d["on_rgba"] if d else (0, 0, 0, 0) for d in table], dtype=np.uint32)[o]
    off = np.array([d["off_rgba"] if d else (0, 0, 0, 0) for d in table], dtype=np.uint32)[o]
    for colour, count in ((off, n_in), (on, n_on)):
        a = ((colour[..., 3] * count.astype(np.uint32) + np.uint32(8)) // np.uint32(16))[..., None]
        old = img[..., :3].astype(np.uint32)
        out = (colour[..., :3] * a + old * (np.uint32(255) - a) + np.uint32(127)) // np.uint32(255)
        img[..., :3] = np.where(shown[..., None], out, old).astype(np.uint8)
    return img, int((img != before).any(axis=-1).sum())
