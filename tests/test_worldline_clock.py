"""Worldline.clock_offsets and to_dsl(readout=...) (relativitypathtracer_amd/worldline.py; DESIGN.md "Readout pass"): the proper time
a display on a piecewise-inertial body shows.  No GPU."""
import math

import numpy as np
import pytest

from relativitypathtracer_amd import Scene, worldline


def _continuous(wl, offsets):
    for j in range(len(wl) - 1):
        end, start = offsets[j] + wl[j].window[1], offsets[j + 1] + wl[j + 1].window[0]
        assert abs(end - start) <= 1e-12 * max(abs(end), 1.0), (j, end, start)


def test_the_twin_who_travels_at_08_c_for_ten_years_each_way_ages_twelve():
    wl = worldline.piecewise([(0.0, 0.0, 0.0, 5.0), (10.0, 8.0, 0.0, 5.0), (20.0, 0.0, 0.0, 5.0)])
    off = wl.clock_offsets()
    assert off.dtype == np.float64 and off.shape == (2,)
    assert off[0] + wl[0].window[0] == pytest.approx(0.0, abs=1e-12)
    assert off[0] + wl[0].window[1] == pytest.approx(6.0, rel=1e-12)            # 10 / gamma, gamma = 1 / 0.6
    assert off[1] + wl[1].window[1] == pytest.approx(12.0, rel=1e-12)
    _continuous(wl, off)
    home = worldline.piecewise([(0.0, 0.0, 0.0, 5.0), (20.0, 0.0, 0.0, 5.0)])
    assert home.clock_offsets()[0] + home[0].window[1] == pytest.approx(20.0, rel=1e-12)
    assert np.allclose(wl.clock_offsets(tau0=3.5) - off, 3.5, rtol=0, atol=1e-12)


def test_the_offsets_are_continuous_at_every_breakpoint_with_open_ended_legs():
    events = [(0.0, 0.0, 0.0, 5.0), (10.0, 0.0, 0.0, 11.0), (15.0, 2.0, 1.0, 9.0), (30.0, 2.0, 1.0, 9.0)]
    wl = worldline.piecewise(events, v_before=(0.1, 0.0, 0.0), v_after=(0.0, 0.0, -0.5))
    off = wl.clock_offsets(tau0=-4.0)
    assert len(off) == 5 and np.all(np.isfinite(off))
    _continuous(wl, off)
    assert off[0] + wl[0].window[1] == pytest.approx(-4.0, abs=1e-12)           # tau0 at the first breakpoint, where the open leg ends
    # the proper time over the three closed legs: sum of dt sqrt(1 - v^2)
    tau = sum((b[0] - a[0]) * math.sqrt(1.0 - sum((q - p) ** 2 for p, q in zip(a[1:], b[1:])) / (b[0] - a[0]) ** 2) for a, b in zip(events, events[1:]))
    assert off[4] + wl[4].window[0] == pytest.approx(-4.0 + tau, rel=1e-12)


def test_to_dsl_without_the_keyword_is_what_it_was_and_with_it_adds_the_d_command():
    wl = worldline.piecewise([(0.0, 0.0, 0.0, 5.0), (10.0, 8.0, 0.0, 5.0), (20.0, 0.0, 0.0, 5.0)])
    plain = wl.to_dsl("Oc", scale=(0.5, 0.5, 0.5), extra="c1,0,0")
    assert " d" not in plain
    assert plain.splitlines()[0] == "Oc p{},0,0,1,0,0.5,0.5,0.5 v{} w{} c1,0,0".format(",".join(repr(c) for c in wl[0].position), ",".join(repr(c) for c in wl[0].velocity),
                                                                                     ",".join(repr(c) for c in wl[0].window))
    shown = wl.to_dsl("Oc", scale=(0.5, 0.5, 0.5), extra="c1,0,0", readout="4,1,0.2,0.3,0.8,0.7")
    off = wl.clock_offsets()
    for j, (a, b) in enumerate(zip(plain.splitlines(), shown.splitlines())):
        assert b == a.replace(" c1,0,0", f" d1,{float(off[j])!r},4,1,0.2,0.3,0.8,0.7 c1,0,0")
    s = Scene()
    assert s.inputScene(shown + "R\n") == ""
    got = s.readouts()
    assert [d["digits"] for d in got] == [4, 4] and [d["decimals"] for d in got] == [1, 1]
    assert [d["offset"] for d in got] == [np.float32(o) for o in off] and all(d["rate"] == 1 for d in got)
    assert got[0]["rect"] == tuple(np.float32(c) for c in (0.2, 0.3, 0.8, 0.7))
    assert np.array_equal(s.windows(), wl.windows())
