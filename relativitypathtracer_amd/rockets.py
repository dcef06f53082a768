"""Rocket sets for the rocket pass (include/rpt.h, rpt_set_rockets) and a float64 model of where the pass puts them.

A set is a numpy array of ROCKET_DTYPE: the 64-byte rpt_rocket records — `pos`, where the rocket is at time 0 of the rest-frame clock of
the scene's object number `object`, `u`, its proper velocity gamma * beta in that frame at that moment, `acc`, the proper acceleration
its crew feels (a 3-vector in the rocket's own instantaneous rest frame at that moment, c = 1), `t0` and `t1`, the window of that clock in
which it shines, and `rgb`, its linear colour at rest in its OWN frame.  The object is only the frame the worldline is written in.
from_arrays, from_ballistics, launch, fleet and trip make a set, as_ballistics approximates one by inertial legs, save / load keep it as
raw records (what `rpt_render_main --rockets FILE` reads), Renderer.set_rockets and render_scene(..., rockets=) take it.  project() is
rules 1-6 of the pass in float64: for previews without a device, and the reference of the physics tests.  Host code only; nothing here
touches the GPU."""
from __future__ import annotations

import math
from typing import Mapping, Optional

import numpy as np

from . import ballistics
from .ballistics import BALLISTIC_DTYPE, proper_velocity
from .particles import window_accepts

ROCKET_DTYPE = np.dtype([("pos", "<f4", (3,)), ("object", "<i4"), ("rgb", "<f4", (3,)), ("t0", "<f4"), ("u", "<f4", (3,)), ("t1", "<f4"),
                         ("acc", "<f4", (3,)), ("reserved", "<f4")])
assert ROCKET_DTYPE.itemsize == 64

INVERSE_SQUARE = 1      # RPT_PARTICLES_INVERSE_SQUARE, which rpt_set_rocket_options reuses


def _dot(a, b):
    return (a * b).sum(axis=-1)


def four_acceleration(u, acc):
    """(g, a0, a): gamma, and the 4-acceleration (a0, a) in the frame in which the proper velocity is u, of a rocket whose crew feels acc
    (rule 1): the boost of (0, acc) out of the rocket's rest frame."""
    g = np.sqrt(1.0 + _dot(u, u))
    a0 = _dot(u, acc)
    return g, a0, acc + u * (a0 / (g + 1.0))[..., None]


def advance(pos, u, acc, t):
    """The state (pos, u, acc) of rule 1 carried along the hyperbola from the frame's time 0 to its time t (rule 3), float64: where the
    rocket is at t, its proper velocity there, and the proper acceleration in ITS rest frame there (the same magnitude).  Returns
    (pos, u, acc, s): s the proper time that passed."""
    pos, u, acc = (np.asarray(x, dtype=np.float64) for x in (pos, u, acc))
    t = np.asarray(t, dtype=np.float64)
    al2 = _dot(acc, acc)
    g, a0, a = four_acceleration(u, acc)
    G = np.sqrt(g * g + 2.0 * a0 * t + al2 * t * t)
    D0 = g * (g + G) + a0 * t
    S0, C0 = t * (g + G) / D0, t * t / D0
    ch0, sh0 = 1.0 + al2 * C0, al2 * S0
    p = pos + u * S0[..., None] + a * C0[..., None]
    u1 = u * ch0[..., None] + a * S0[..., None]
    a01 = g * sh0 + a0 * ch0
    a1 = u * sh0[..., None] + a * ch0[..., None]
    return p, u1, a1 - u1 * (a01 / (G + 1.0))[..., None], proper_time(al2, 2.0 * t / (g + G))


def proper_time(al2, z):
    """s = (2 / alpha) atanh(alpha z / 2), and z where alpha = 0; NaN where |alpha z| >= 2 (no real s: beyond the horizon)."""
    al2, z = np.broadcast_arrays(np.asarray(al2, dtype=np.float64), np.asarray(z, dtype=np.float64))
    x = 0.5 * np.sqrt(al2) * z
    with np.errstate(all="ignore"):
        ratio = np.where(np.abs(x) < 1e-4, 1.0 + x * x / 3.0 + x ** 4 / 5.0, np.arctanh(x) / np.where(x == 0.0, 1.0, x))
    return z * ratio


def redshift_from_pad(alpha: float, s):
    """The Doppler factor of a rocket that left the pad from rest with proper acceleration alpha, seen from the pad in the light it sent
    at its proper time s: exp(-alpha s)."""
    return np.exp(-float(alpha) * np.asarray(s, dtype=np.float64))


def from_arrays(pos, object, rgb, beta=None, u=None, acc=None, t0=-math.inf, t1=math.inf, epoch=0.0) -> np.ndarray:
    """A set from columns: pos (n, 3), where each rocket is at the object's time `epoch` (one number or n); object one index or n of
    them; rgb one colour or n; the velocity at that time as beta (units of c) or as the proper velocity u = gamma * beta, one vector or n
    (neither: at rest); acc the proper acceleration at that time, one vector or n (none: 0); t0, t1 one number or n.  An epoch other than
    0 is moved to time 0 along the hyperbola in float64: stored are the place, the proper velocity and the proper acceleration there."""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if beta is not None and u is not None:
        raise ValueError("from_arrays: give beta or u, not both")
    if beta is not None:
        u = proper_velocity(np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1, 3), (n, 3)))
    u = np.broadcast_to(np.zeros(3) if u is None else np.asarray(u, dtype=np.float64).reshape(-1, 3), (n, 3))
    acc = np.broadcast_to(np.zeros(3) if acc is None else np.asarray(acc, dtype=np.float64).reshape(-1, 3), (n, 3))
    epoch = np.broadcast_to(np.asarray(epoch, dtype=np.float64).reshape(-1), (n,))
    if epoch.any():
        p, u, acc, _ = advance(p, u, acc, -epoch)
    out = np.zeros(n, dtype=ROCKET_DTYPE)
    out["pos"], out["u"], out["acc"] = p, u, acc
    out["object"] = np.broadcast_to(np.asarray(object, dtype=np.int64).reshape(-1) if np.ndim(object) else int(object), (n,))
    out["rgb"] = np.broadcast_to(np.asarray(rgb, dtype=np.float64).reshape(-1, 3), (n, 3))
    out["t0"] = np.broadcast_to(np.asarray(t0, dtype=np.float64).reshape(-1), (n,))
    out["t1"] = np.broadcast_to(np.asarray(t1, dtype=np.float64).reshape(-1), (n,))
    return out


def from_ballistics(records) -> np.ndarray:
    """Ballistic records as rockets that do not accelerate: acc = 0."""
    b = np.ascontiguousarray(records, dtype=BALLISTIC_DTYPE).reshape(-1)
    out = np.zeros(len(b), dtype=ROCKET_DTYPE)
    for field in ("pos", "object", "rgb", "t0", "u", "t1"):
        out[field] = b[field]
    return out


def launch(object: int, origin, acc, n_times, rgb) -> np.ndarray:
    """Rockets that leave `origin` from rest at the object's times n_times (a sequence, or a count n for the times 0, 1, ... n - 1) under
    the proper acceleration acc: one record per time, each shining from the moment it leaves — the textbook relativistic rocket."""
    t = np.arange(int(n_times), dtype=np.float64) if np.ndim(n_times) == 0 else np.asarray(n_times, dtype=np.float64).reshape(-1)
    return from_arrays(np.broadcast_to(np.asarray(origin, dtype=np.float64).reshape(3), (len(t), 3)), object, rgb, acc=acc, t0=t, epoch=t)


def fleet(object: int, positions, acc, rigid: bool = False, rgb=(1.0, 1.0, 1.0)) -> np.ndarray:
    """Rockets at rest at `positions` (n, 3) at the object's time 0 that all start then, along acc.  rigid=False: every rocket has the
    proper acceleration acc — Bell's spaceships, whose spacing in the object's frame stays what it was.  rigid=True: rocket i has the
    magnitude 1 / (1 / alpha + (x_i - x_0).a^) — alpha = |acc| is the first rocket's, a^ the direction —, so that all share one horizon:
    a Born-rigid (Rindler) fleet, whose spacing stays what it was in the rockets' own frames."""
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    a = np.asarray(acc, dtype=np.float64).reshape(3)
    alpha = float(np.linalg.norm(a))
    accs = np.broadcast_to(a, x.shape)
    if rigid:
        if alpha == 0.0:
            raise ValueError("fleet: a rigid fleet needs an acceleration")
        height = 1.0 / alpha + (x - x[0]) @ (a / alpha)
        if (height <= 0.0).any():
            raise ValueError("fleet: a rocket of a rigid fleet lies on or behind the fleet's horizon")
        accs = (a / alpha) / height[:, None]
    return from_arrays(x, object, rgb, acc=accs)


def trip(object: int, origin, direction, acc: float, leg_proper_time: float, rgb) -> np.ndarray:
    """The round trip of the twin paradox from rest at `origin` at the object's time 0: four hyperbolic legs of the proper time
    leg_proper_time each — speed up along `direction`, slow down to rest, speed up homewards, slow down to rest at the origin — with
    the proper acceleration acc (a magnitude).  Four records with abutting windows, each leg's start advanced in float64."""
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    d = d / np.linalg.norm(d)
    alpha, tau = float(acc), float(leg_proper_time)
    t, x, u = 0.0, np.asarray(origin, dtype=np.float64).reshape(3).copy(), np.zeros(3)
    legs = []
    for sign in (1.0, -1.0, -1.0, 1.0):
        g, a0, a = four_acceleration(u, sign * alpha * d)
        sh, ch1 = math.sinh(alpha * tau) / alpha, (math.cosh(alpha * tau) - 1.0) / (alpha * alpha)
        t_end = t + g * sh + a0 * ch1
        legs.append(from_arrays(x[None], object, rgb, u=u[None], acc=(sign * alpha * d)[None], t0=t, t1=t_end, epoch=t))
        x = x + u * sh + a * ch1
        u = u * math.cosh(alpha * tau) + a * sh
        t = t_end
    out = np.concatenate(legs)
    out["t0"][1:] = out["t1"][:-1]      # abutting as float32 numbers
    return out


def as_ballistics(rocket, K: int) -> np.ndarray:
    """Each rocket record as K ballistic legs: its window, which must be finite, cut into K equal parts, and in each part the straight
    worldline that touches the hyperbola at the part's middle.  The legs' windows abut."""
    r = np.ascontiguousarray(rocket, dtype=ROCKET_DTYPE).reshape(-1)
    if int(K) < 1 or not (np.isfinite(r["t0"]).all() and np.isfinite(r["t1"]).all()):
        raise ValueError("as_ballistics: K >= 1 legs of a finite window [t0, t1)")
    edges = r["t0"].astype(np.float64)[:, None] + (r["t1"].astype(np.float64) - r["t0"].astype(np.float64))[:, None] * (np.arange(int(K) + 1) / float(K))
    mid = 0.5 * (edges[:, 1:] + edges[:, :-1])
    rep = lambda x: np.repeat(x.astype(np.float64), int(K), axis=0)
    p, u, _, _ = advance(rep(r["pos"]), rep(r["u"]), rep(r["acc"]), mid.reshape(-1))
    out = ballistics.from_arrays(p, np.repeat(r["object"], int(K)), rep(r["rgb"]), u=u, t0=edges[:, :-1].reshape(-1), t1=edges[:, 1:].reshape(-1), epoch=mid.reshape(-1))
    out["t1"].reshape(len(r), int(K))[:, :-1] = out["t0"].reshape(len(r), int(K))[:, 1:]
    return out


def save(path, rockets) -> None:
    """The raw 64-byte records, one after the other."""
    np.ascontiguousarray(rockets, dtype=ROCKET_DTYPE).tofile(path)


def load(path) -> np.ndarray:
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size % 64:
        raise ValueError(f"{path}: {raw.size} bytes are no whole number of 64-byte rocket records")
    return raw.view(ROCKET_DTYPE).copy()


def project(rockets, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0, options: Optional[Mapping] = None,
            temperatures=None) -> dict:
    """Rules 1-6 of the rocket pass in float64.  rockets: ROCKET_DTYPE records; the rest as ballistics.project takes it.  Returns a
    dict of arrays, one entry per record, shaped as ballistics.project's — visible, X, Y, dist, r (r', the camera's distance in the
    rocket's rest frame at emission), D, te, k, n, rgb, tau, pos_e — and: z (the half-angle variable of the emission event, counted from
    the camera's time), d (1 - alpha^2 z^2 / 4), s (the rocket's proper time at emission, counted from the object's time 0), nq and Aq
    (n and Aq of rule 4), branch (rule 5: 0 the root where n > 0, 1 the root where n <= 0 and Aq < 0, 2 none: Aq >= 0, 3 a root with
    d <= 0; -1 where rule 4 has skipped the record, or on the slice)."""
    if interval not in (-1, 0):
        raise ValueError("project: the light cone has a closed form for interval -1 and 0 only")
    p = np.ascontiguousarray(rockets, dtype=ROCKET_DTYPE).reshape(-1)
    return project_columns(p["pos"].astype(np.float64), p["object"].astype(np.int64), p["rgb"].astype(np.float64), p["u"].astype(np.float64),
                           p["acc"].astype(np.float64), p["t0"].astype(np.float64), p["t1"].astype(np.float64), objects, camera, W, H, interval, flags,
                           options, temperatures)


def project_columns(pos, idx, rgb0, u, acc, t0, t1, objects, camera: Mapping, W: int, H: int, interval: int = -1, flags: int = 0,
                    options: Optional[Mapping] = None, temperatures=None) -> dict:
    """project() on float64 columns — pos (N, 3), idx (N,) object indices, rgb0 (N, 3), u (N, 3), acc (N, 3), t0 and t1 (N,)."""
    options = dict(options or {})
    invs, cams = ballistics._frames(objects)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(invs)):
        raise ValueError(f"project: a record names object {int(idx.max())}, the Object[] holds {len(invs)}")
    inv, cam = invs[idx], cams[idx]
    with np.errstate(all="ignore"):
        # rules 1 and 3
        al2 = _dot(acc, acc)
        g, a0, a = four_acceleration(u, acc)
        T = cam[:, 0]
        G = np.sqrt(g * g + 2.0 * a0 * T + al2 * T * T)
        D0 = g * (g + G) + a0 * T
        visible = D0 > 0.0
        S0, C0 = T * (g + G) / D0, T * T / D0
        ch0, sh0 = 1.0 + al2 * C0, al2 * S0
        p = pos + u * S0[:, None] + a * C0[:, None]
        u1 = u * ch0[:, None] + a * S0[:, None]
        a01 = g * sh0 + a0 * ch0
        a1 = u * sh0[:, None] + a * ch0[:, None]
        # rule 4
        w0 = p - cam[:, 1:]
        ww, nq, m = _dot(w0, w0), _dot(u1, w0), _dot(a1, w0)
        Aq = (m - 1.0) - ww * al2 / 4.0
        r = np.sqrt(nq * nq - Aq * ww)
        placed = visible & (r > 0.0) & np.isfinite(r)
        # rule 5
        if interval == -1:
            z = np.where(nq > 0.0, -(ww / (nq + r)), np.where(Aq < 0.0, (r - nq) / Aq, np.nan))
            branch = np.where(nq > 0.0, 0, np.where(Aq < 0.0, 1, 2))
        else:
            i0 = inv[:, 0, :]
            P = _dot(i0[:, 1:], w0)
            Q = i0[:, 0] * G + _dot(i0[:, 1:], u1)
            R = i0[:, 0] * a01 + _dot(i0[:, 1:], a1)
            z = -(2.0 * P) / (Q + np.sqrt(Q * Q - 4.0 * (0.5 * R - P * al2 / 4.0) * P))
            branch = np.full(len(idx), -1)
        d = 1.0 - al2 * z * z / 4.0
        if interval == -1:
            branch = np.where((branch < 2) & ~(d > 0.0), 3, branch)
        branch = np.where(placed, branch, -1)
        visible = placed & (d > 0.0)
        # rule 6
        S = z / d
        C = z * S / 2.0
        tau = G * S + a01 * C
        w = w0 + u1 * S[:, None] + a1 * C[:, None]
        te = T + tau
        visible &= window_accepts(t0, t1, te)
        s = proper_time(al2, 2.0 * T / (g + G)) + proper_time(al2, z)
    seen = ballistics.seen_from_emission(visible, inv, tau, w, r, rgb0, camera, W, H, interval, flags, options, temperatures)
    return dict(seen, r=r, te=te, tau=tau, pos_e=w + cam[:, 1:], z=z, d=d, s=s, nq=nq, Aq=Aq, branch=branch)
