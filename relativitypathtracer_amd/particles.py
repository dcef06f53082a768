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


# ---- lit particles (rpt_set_particle_lighting) -------------------------------------------------------------------------
LIT, SHADOWED, AMBIENT = 1, 2, 4      # RPT_PARTICLES_LIT, RPT_PARTICLES_SHADOWED, RPT_PARTICLES_AMBIENT


def dust(object: int, lo, hi, count: int, rgb, seed: int = 0) -> np.ndarray:
    """count grains uniform at random in the box from the corner lo to the corner hi, at rest in the frame of `object`, of albedo rgb:
    a dust cloud for the lit pass.  Random rather than particles.lattice on purpose: a regular lattice puts whole planes of grains on
    the edge of a shadow or of a light front, where they flicker together."""
    if int(count) < 0:
        raise ValueError("dust: count is negative")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    u = np.random.default_rng(seed).random((int(count), 3))
    return from_arrays(lo + (hi - lo) * u, object, rgb)


def _doppler_operator(flags: int, D, rgb) -> np.ndarray:
    """S_f(D, rgb) of the Doppler model in float64, without the point source's / D^2: what a light's colour goes through."""
    D = np.asarray(D, dtype=np.float64)
    o = point_source_colour(flags, D, rgb)
    return o * (D ** 2)[:, None] if flags & 2 else o


def illuminate(particles, objects, interval: int = -1, doppler: int = 0, ambient: float = 0.0, flags: int = LIT, windows=None) -> dict:
    """Rules D0-D7 of the lit particles in float64, WITHOUT shadows (flags' SHADOWED bit is ignored: no geometry is looked at) and
    without the depth test: what every grain scatters, as if it were seen.  particles, objects, windows: as project takes them;
    interval -1 or 0; doppler: the flags of Renderer.set_doppler; ambient: the scene's; flags: LIT, optionally | AMBIENT (0: the plain
    pass, c_rest = rgb).  Returns a dict: lights (the indices of the objects that are lights, in order), and per grain and light,
    shaped (N, len(lights)): te (the light's emission time in ITS rest frame, P.x + dLF.x), len (the light-frame distance), k (the
    falloff), di (the light's Doppler factor, dObj.x / dLF.x), lit (the pair contributes: len > 0 and finite, and the window holds te),
    contribution (N, len(lights), 3), light_dir (N, len(lights), 4) the grain -> lamp displacement in the camera frame (the lamp's
    emission event is hit_pos + light_dir); per grain: hit_pos (N, 4) the grain's event in the camera frame, c_rest (N, 3) the colour at
    rest (rule D7's input), and rgb (N, 3) the colour after rule 3 (the camera factor D = dist / r through S_f, / D^2 with beaming;
    the optional / r^2 is project's option and is not applied here), D (N,).  With interval 0 (rule D0) or flags 0: lit is all False,
    c_rest = the grains' rgb."""
    if interval not in (-1, 0):
        raise ValueError("illuminate: the light cone has a closed form for interval -1 and 0 only")
    p = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE).reshape(-1)
    objs = _objects_array(objects)
    idx = p["object"].astype(np.int64)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(objs)):
        raise ValueError(f"illuminate: a particle names object {int(idx.max())}, the Object[] holds {len(objs)}")
    pos, rgb0 = p["pos"].astype(np.float64), p["rgb"].astype(np.float64)
    lor = objs["Lorentz"].astype(np.float64).reshape(-1, 4, 4)
    inv = objs["InvLorentz"].astype(np.float64).reshape(-1, 4, 4)
    cam = objs["stationaryCam"].astype(np.float64).reshape(-1, 4)[idx]
    M = objs["M"].astype(np.float64).reshape(-1, 4, 4)
    lights = np.nonzero(objs["light"] != 0)[0]
    N, nl = len(p), len(lights)
    with np.errstate(all="ignore"):
        w = pos - cam[:, 1:]
        r = np.sqrt((w * w).sum(axis=1))
        tau = -r if interval == -1 else -(inv[idx][:, 0, 1:] * w).sum(axis=1) / inv[idx][:, 0, 0]
        kcam = np.einsum("nij,nj->ni", inv[idx], np.concatenate([tau[:, None], w], axis=1))
        dist = np.sqrt((kcam[:, 1:] ** 2).sum(axis=1))
        E = np.concatenate([(cam[:, 0] + tau)[:, None], pos], axis=1)
        hit_pos = np.einsum("nij,nj->ni", inv[idx], E)
        out = {"lights": lights, "hit_pos": hit_pos, "te": np.full((N, nl), np.nan), "len": np.full((N, nl), np.nan),
               "k": np.zeros((N, nl)), "di": np.ones((N, nl)), "lit": np.zeros((N, nl), dtype=bool), "contribution": np.zeros((N, nl, 3)), "light_dir": np.zeros((N, nl, 4))}
        if not (flags & LIT) or interval == 0:
            c_rest = rgb0.copy()
        else:
            c_rest = rgb0 * float(ambient) if flags & AMBIENT else np.zeros_like(rgb0)
            for j, i in enumerate(lights):
                P = hit_pos @ lor[i].T
                d3 = M[i][:3, 3][None, :] - P[:, 1:]
                ln = np.sqrt((d3 * d3).sum(axis=1))
                dLF = np.concatenate([(interval * ln)[:, None], d3], axis=1)
                te = P[:, 0] + dLF[:, 0]
                ok = (ln > 0.0) & np.isfinite(ln)
                if windows is not None:
                    win = np.asarray(windows, dtype=np.float64).reshape(-1, 2)[i]
                    ok &= window_accepts(win[0], win[1], te)
                light_dir = dLF @ inv[i].T
                d_obj = np.einsum("nij,nj->ni", lor[idx], light_dir)
                l3 = d_obj[:, 1:]
                k = 1.0 / (1.0 + 0.1 * np.sqrt((l3 * l3).sum(axis=1)) + 0.01 * (l3 * l3).sum(axis=1))
                di = d_obj[:, 0] / dLF[:, 0]
                col = np.broadcast_to(objs["color"][i].astype(np.float64).reshape(-1)[:3], (N, 3))
                if doppler:
                    col = _doppler_operator(doppler, np.where(ok, di, 1.0), col)
                contribution = np.where(ok[:, None], (rgb0 * k[:, None]) * col, 0.0)
                c_rest = c_rest + contribution
                out["te"][:, j], out["len"][:, j], out["k"][:, j], out["di"][:, j] = te, ln, k, di
                out["lit"][:, j], out["contribution"][:, j], out["light_dir"][:, j] = ok, contribution, light_dir
        if doppler and interval != 0:
            D = dist / r
            rgb = point_source_colour(doppler, D, c_rest)
        else:
            D = dist / r if interval != 0 else np.ones(N)
            rgb = c_rest.copy()
    out.update({"c_rest": c_rest, "rgb": rgb, "D": D, "r": r, "dist": dist})
    return out
