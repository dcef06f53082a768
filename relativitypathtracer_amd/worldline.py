"""Piecewise-inertial worldlines from per-object time windows ("Time windows").

The renderer moves every object at one constant velocity.  A body whose motion changes — the twin's turnaround, a launch, a bounce — is
K copies of the object, one per leg, each with its own velocity and with the time window of its leg (the DSL's `w` command,
Renderer.set_object_windows): leg j exists between the two breakpoints it joins, measured on its OWN rest-frame clock, which is the
coordinate the windows act on.

Convention (the host's, rpt_vector.cpp Lorentz()): coordinates are (t, x, y, z) with c = 1, and an object of velocity v has

    boost(v) = [[ g,      -g v^T                    ],
                [-g v,    I + (g - 1) v v^T / |v|^2 ]],      g = 1 / sqrt(1 - |v|^2)

as Object.Lorentz while the camera rests at the scene's origin; its rest-frame coordinates of a scene-frame event E are boost(v) . E,
and the translation of its `p` command is a rest-frame position.  A point that passes through the scene-frame events E_j and E_{j+1}
moves at v_j = (x_{j+1} - x_j) / (t_{j+1} - t_j); in its rest frame it sits at the spatial part of boost(v_j) . E_j (the same as that of
boost(v_j) . E_{j+1}), from rest time (boost(v_j) . E_j).t to (boost(v_j) . E_{j+1}).t.  Everything here is float64.

Limit.  A window switches a whole leg on and off on ITS OWN simultaneity plane t_rest = const, and two legs' planes through one breakpoint
differ: only the breakpoint itself — the centre handed to `p` — changes legs at one event.  A body of size R around it is therefore seen
doubled, or missing, over a region of about R * |delta v| around the breakpoint (a point at rest-frame offset r from the centre leaves
leg j at scene time t_k + g_j v_j . r and joins leg j+1 at t_k + g_{j+1} v_{j+1} . r).  Keep bodies small against the legs, or accept
the seam; a rigid accelerated body does not exist in relativity either.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np


def boost(v: Sequence[float]) -> np.ndarray:
    """The host's Lorentz(v) (rpt_vector.cpp) in float64: scene frame -> the rest frame of an object moving at v; rows t, x, y, z."""
    v = np.asarray(v, dtype=np.float64).reshape(3)
    v2 = float(v @ v)
    if not v2 < 1.0:
        raise ValueError(f"|v| = {math.sqrt(v2)} is not below the speed of light")
    m = np.eye(4)
    if v2 == 0.0:
        return m
    g = 1.0 / math.sqrt(1.0 - v2)
    m[0, 0] = g
    m[0, 1:] = -g * v
    m[1:, 0] = -g * v
    m[1:, 1:] = np.eye(3) + (g - 1.0) * np.outer(v, v) / v2
    return m


@dataclass(frozen=True)
class Leg:
    """One inertial leg: `velocity` for the DSL's `v`, `position` (rest frame) for `p`, `window` = (t0, t1) (rest frame) for `w`."""
    velocity: Tuple[float, float, float]
    position: Tuple[float, float, float]
    window: Tuple[float, float]

    def centre_at(self, rest_time: float) -> np.ndarray:
        """The scene-frame event (t, x, y, z) of the leg's centre at its rest-frame time `rest_time`."""
        e = np.array([rest_time, *self.position], dtype=np.float64)
        return boost([-c for c in self.velocity]) @ e


class Worldline:
    def __init__(self, legs: List[Leg]):
        self.legs = legs

    def __len__(self):
        return len(self.legs)

    def __iter__(self):
        return iter(self.legs)

    def __getitem__(self, i):
        return self.legs[i]

    def windows(self) -> np.ndarray:
        """(K, 2) float32, the rows Renderer.set_object_windows takes for the legs' objects."""
        return np.array([leg.window for leg in self.legs], dtype=np.float32)

    def clock_offsets(self, tau0: float = 0.0) -> np.ndarray:
        """One float64 per leg: offset_j + t is the body's proper time at leg j's rest-frame time t — what a display on leg j's object
        needs as its `offset` (rate 1) for the legs to show ONE clock.  A leg's rest-frame time is the body's proper time up to a
        constant, so the proper time is accumulated over the legs' windows; tau0 is its value at the first breakpoint (the end of an
        open-ended first leg, else the start of the first leg).  At every breakpoint offset_j + window_j[1] == offset_{j+1} + window_{j+1}[0]."""
        tau = float(tau0)                   # the proper time at the breakpoint where the next leg begins
        out = []
        for j, leg in enumerate(self.legs):
            t0, t1 = leg.window
            if j == 0 and t0 == -math.inf:
                out.append(tau - t1)        # (the open-ended first leg ends at the first breakpoint)
                continue
            out.append(tau - t0)
            tau += t1 - t0
        return np.array(out, dtype=np.float64)

    def to_dsl(self, shape: str = "Os", scale: Sequence[float] = (1.0, 1.0, 1.0), extra: str = "", readout: Optional[str] = None,
               tau0: float = 0.0) -> str:
        """One `O… p… v… w…` block per leg (repr() of the float64 values: they round to float once, in the scene parser).  shape: the
        object command ("Os", "Oc", "Om0"); scale: the `p` command's three scale factors (no rotation); extra: further commands of every
        leg, e.g. "c1,0,0 l1".  readout: "DIGITS,DECIMALS[,U0,V0,U1,V1]" gives every leg a display of the body's proper time (the
        DSL's `d` command: `d1,OFFSET_j,…` with clock_offsets(tau0)); without it the text is what it was before displays existed."""
        out = []
        offsets = self.clock_offsets(tau0) if readout is not None else None
        for j, leg in enumerate(self.legs):
            p = ",".join(repr(float(c)) for c in leg.position)
            s = ",".join(repr(float(c)) for c in scale)
            v = ",".join(repr(float(c)) for c in leg.velocity)
            w = ",".join("inf" if c == math.inf else ("-inf" if c == -math.inf else repr(float(c))) for c in leg.window)
            d = f" d1,{float(offsets[j])!r},{readout}" if readout is not None else ""
            out.append(f"{shape} p{p},0,0,1,0,{s} v{v} w{w}{d}" + (f" {extra}" if extra else ""))
        return "\n".join(out) + "\n"


def _leg(v: np.ndarray, anchor: np.ndarray, first: Optional[np.ndarray], last: Optional[np.ndarray]) -> Leg:
    b = boost(v)
    rest = b @ anchor
    t0 = -math.inf if first is None else float((b @ first)[0])
    t1 = math.inf if last is None else float((b @ last)[0])
    return Leg(tuple(float(c) for c in v), tuple(float(c) for c in rest[1:]), (t0, t1))


def piecewise(breakpoints, v_before: Optional[Sequence[float]] = None, v_after: Optional[Sequence[float]] = None) -> Worldline:
    """The legs of a point that passes through the K + 1 scene-frame events `breakpoints` ((t, x, y, z) rows, t increasing, consecutive
    pairs timelike separated) at constant velocity between them.  v_before / v_after add an open-ended leg before the first / after
    the last event, with windows (-inf, .) / (., +inf).  Raises ValueError for fewer than two events (without open-ended legs: fewer
    than one), non-increasing times or a leg at or above the speed of light."""
    e = np.asarray(breakpoints, dtype=np.float64)
    if e.ndim != 2 or e.shape[1] != 4 or e.shape[0] < 1 or (e.shape[0] < 2 and v_before is None and v_after is None):
        raise ValueError("breakpoints are at least two (t, x, y, z) rows")
    if not np.all(np.isfinite(e)):
        raise ValueError("breakpoints must be finite")
    legs: List[Leg] = []
    if v_before is not None:
        legs.append(_leg(np.asarray(v_before, dtype=np.float64).reshape(3), e[0], None, e[0]))
    for j in range(e.shape[0] - 1):
        dt = e[j + 1, 0] - e[j, 0]
        if not dt > 0.0:
            raise ValueError(f"breakpoint {j + 1} is not later than breakpoint {j}")
        v = (e[j + 1, 1:] - e[j, 1:]) / dt
        if not float(v @ v) < 1.0:
            raise ValueError(f"breakpoints {j} and {j + 1} are not timelike separated (|v| = {math.sqrt(float(v @ v))})")
        legs.append(_leg(v, e[j], e[j], e[j + 1]))
    if v_after is not None:
        legs.append(_leg(np.asarray(v_after, dtype=np.float64).reshape(3), e[-1], e[-1], None))
    return Worldline(legs)
