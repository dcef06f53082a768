"""Rod sets for the segment pass (include/rpt.h, rpt_set_segments) and a float64 model of where the pass puts them.

A set is a numpy array of SEGMENT_DTYPE: the 48-byte rpt_segment records — `a` and `b`, the rod's ends in the REST FRAME of the scene's
object number `object` (the coordinates of an event record's event[1..3]), and `rgb`, its linear colour at rest PER UNIT REST-FRAME
LENGTH.  from_arrays, polyline, box_edges and rod_lattice make one, save / load keep it as raw records (what
`rpt_render_main --segments FILE` reads), Renderer.set_segments and render_scene(..., segments=) take it.  as_particles is what a user
had to do before the pass existed: lamps along the rod.  project() is rules S0-S2 of the pass in float64: for previews without a
device, and the reference of the tests.  Host code only; nothing here touches the GPU."""
from __future__ import annotations

import math
from typing import Mapping, Optional

import numpy as np

from . import particles as _particles

SEGMENT_DTYPE = np.dtype([("a", "<f4", (3,)), ("object", "<i4"), ("b", "<f4", (3,)), ("_pad0", "<f4"), ("rgb", "<f4", (3,)), ("_pad1", "<f4")])
assert SEGMENT_DTYPE.itemsize == 48

INVERSE_SQUARE = 1      # RPT_SEGMENTS_INVERSE_SQUARE
MAX_STEPS = 1024        # RPT_SEGMENT_MAX_STEPS
PIECES = (1, 2, 4, 8, 16, 32, 64)
MAX_LOAD = 1 << 21      # count x pieces


def from_arrays(a, b, object, rgb) -> np.ndarray:
    """A set from columns: a and b (n, 3), object one index or n of them, rgb one colour or n of them."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    if len(a) != len(b):
        raise ValueError(f"from_arrays: {len(a)} first ends and {len(b)} second ends")
    out = np.zeros(len(a), dtype=SEGMENT_DTYPE)
    out["a"] = a
    out["b"] = b
    out["object"] = np.broadcast_to(np.asarray(object, dtype=np.int64).reshape(-1) if np.ndim(object) else int(object), (len(a),))
    out["rgb"] = np.broadcast_to(np.asarray(rgb, dtype=np.float64).reshape(-1, 3), (len(a), 3))
    return out


def polyline(points, object: int, rgb) -> np.ndarray:
    """n - 1 rods joining n points in their order, all at rest in the frame of `object`."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(p) < 2:
        raise ValueError("polyline: at least two points")
    return from_arrays(p[:-1], p[1:], object, rgb)


def rod_lattice(object: int, lo, hi, cells, rgb) -> np.ndarray:
    """Every edge of a grid of cells[0] x cells[1] x cells[2] cells (one number: the same along every axis) between the corners lo and
    hi, at rest in the frame of `object`: the lattice of rods that bends into hyperbolae around a fast observer.  One rod per cell edge,
    none twice."""
    n = [int(c) for c in np.broadcast_to(np.asarray(cells), (3,))]
    if min(n) < 1:
        raise ValueError("rod_lattice: at least one cell along every axis")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    axes = [np.linspace(lo[k], hi[k], n[k] + 1) for k in range(3)]
    ends_a, ends_b = [], []
    for axis in range(3):       # the rods along `axis`: one per cell along it and per grid line across it
        u, v = (axis + 1) % 3, (axis + 2) % 3
        i, p, q = np.meshgrid(np.arange(n[axis]), axes[u], axes[v], indexing="ij")
        a, b = np.zeros(i.shape + (3,)), np.zeros(i.shape + (3,))
        a[..., axis], b[..., axis] = axes[axis][i], axes[axis][i + 1]
        a[..., u] = b[..., u] = p
        a[..., v] = b[..., v] = q
        ends_a.append(a.reshape(-1, 3))
        ends_b.append(b.reshape(-1, 3))
    return from_arrays(np.concatenate(ends_a), np.concatenate(ends_b), object, rgb)


def box_edges(object: int, lo, hi, rgb) -> np.ndarray:
    """The 12 edges of the box between the corners lo and hi: the wire frame that looks rotated, not contracted."""
    return rod_lattice(object, lo, hi, 1, rgb)


def save(path, segments) -> None:
    """The raw 48-byte records, one after the other."""
    np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE).tofile(path)


def load(path) -> np.ndarray:
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size % 48:
        raise ValueError(f"{path}: {raw.size} bytes are no whole number of 48-byte segment records")
    return raw.view(SEGMENT_DTYPE).copy()


def as_particles(segments, n) -> np.ndarray:
    """What the pass replaces: n lamps per rod (one number, or one per rod) at the midpoints of n equal parts, each of colour
    rgb |b - a| / n, as particles.PARTICLE_DTYPE records.  The rod's total flux is kept."""
    s = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE).reshape(-1)
    counts = np.broadcast_to(np.asarray(n, dtype=np.int64), (len(s),))
    if len(s) and counts.min() < 1:
        raise ValueError("as_particles: at least one lamp per rod")
    which = np.repeat(np.arange(len(s)), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)
    per = counts[which].astype(np.float64)
    u = (np.arange(len(which)) - first + 0.5) / per
    a, b = s["a"].astype(np.float64)[which], s["b"].astype(np.float64)[which]
    length = np.sqrt(((b - a) ** 2).sum(axis=1))
    return _particles.from_arrays(a + (b - a) * u[:, None], s["object"][which], s["rgb"].astype(np.float64)[which] * (length / per)[:, None])


def nodes(segments, pieces: int) -> np.ndarray:
    """Rule S0's node positions, (n, pieces + 1, 3) in float64 from the float32 ends: a + (b - a) j / P, the last one b."""
    s = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE).reshape(-1)
    a, b = s["a"].astype(np.float64), s["b"].astype(np.float64)
    j = np.arange(pieces + 1, dtype=np.float64) / float(pieces)
    return a[:, None, :] + (b - a)[:, None, :] * j[None, :, None]


def project(segments, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0, options: Optional[Mapping] = None,
            windows=None) -> dict:
    """Rules S0-S2 of the segment pass in float64.  segments: SEGMENT_DTYPE records; objects, camera, interval, flags, windows: as
    particles.project takes them; options: dict(inverse_square=..., depth_bias=..., pieces=...) as Renderer.set_segment_options takes.
    Returns a dict: per node, shaped (n, pieces + 1, ...), everything particles.project returns (visible, X, Y, dist, r, D, te, k, n,
    rgb — the colour per unit length after rule 3); per piece, shaped (n, pieces): `placed` (the segment has a length and both nodes
    are placed), `shift` (what rule S2 adds to the second node's X on the panorama: 0, -Px or +Px), `L`, `m` (0 where the piece is not
    placed or L > 1024) and `len`, (n,) the rest-frame length of one piece."""
    options = dict(options or {})
    P = int(options.get("pieces", 16))
    if P not in PIECES:
        raise ValueError(f"project: pieces is one of {PIECES}, not {P}")
    s = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE).reshape(-1)
    n = len(s)
    pos = nodes(s, P)
    out = _particles.project_columns(pos.reshape(-1, 3), np.repeat(s["object"].astype(np.int64), P + 1),
                                     np.repeat(s["rgb"].astype(np.float64), P + 1, axis=0), objects, camera, W, H, interval, flags,
                                     {"inverse_square": options.get("inverse_square", False)}, windows)
    out = {key: value.reshape((n, P + 1) + value.shape[1:]) for key, value in out.items()}
    d = s["b"].astype(np.float64) - s["a"].astype(np.float64)
    length = np.sqrt((d * d).sum(axis=1)) / P
    live = (length > 0.0) & np.isfinite(length)
    placed = out["visible"][:, :-1] & out["visible"][:, 1:] & live[:, None]
    with np.errstate(all="ignore"):
        X0, X1, Y0, Y1 = out["X"][:, :-1], out["X"][:, 1:], out["Y"][:, :-1], out["Y"][:, 1:]
        shift = np.zeros((n, P))
        if camera.get("mode", "pinhole") == "equirect":
            period = W * (2.0 * math.pi / float(np.float32(camera.get("h_fov", 2.0 * math.pi))))
            shift = np.where(X1 - X0 > 0.5 * period, -period, np.where(X1 - X0 < -0.5 * period, period, 0.0))
        L = np.maximum(np.abs(X1 + shift - X0), np.abs(Y1 - Y0))
        m = np.where(placed & (L <= MAX_STEPS), np.maximum(1, np.ceil(L)), 0)
    out.update(placed=placed, shift=np.where(placed, shift, 0.0), L=np.where(placed, L, np.nan), m=np.nan_to_num(m).astype(np.int64), len=length)
    return out
