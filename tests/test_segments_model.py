"""The segment pass without a device: tests/native/segments_oracle.c, the C restatement of rules S0-S5 and the reference of
tests/test_gpu_segments.py, against particles_oracle.c (the nodes, bit for bit), against relativitypathtracer_amd.segments.project (the
float64 model), against the flux a rod must carry, and against the lamps a user had to string along a rod before the pass existed; the
seam; and the non-vacuity of tests/segments_cases.py on CPU event frames.

The node bound is §20's with one term added (DERIVED in §22): the oracle's node a + d (j / P) is a float32 number, the model's is not, and
they differ by |d pos| <= 1.01 eps (2 |b - a| + |pos|); that moves the direction by at most sqrt(2) a^2 |d pos| / r.  So per node
    dn = (16.5 a^2 + 4) eps + 1.43 a^2 eps (2 |b - a| + |pos|) / r,      |d dist| / dist <= dn,
and §19's projection steps follow as test_particles_model.py has them.

The flux bound (DERIVED in §22), per channel, for a rod with Doppler and the inverse square off whose taps all land in the frame on miss
pixels: S = sum of the accumulator 2^-24, F = rgb |b - a| in exact arithmetic on the float32 ends,
    -(4 M 2^-24 + 10 eps F) <= S - F <= 10 eps F,       M = the samples the rod took (4 taps each, each truncated by < 2^-24)."""
import math

import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import segments_cases as sg
import stars_cases as sc
from relativitypathtracer_amd import particles, segments
from relativitypathtracer_amd.events import EVENT_DTYPE, _objects_array
from relativitypathtracer_amd.scene import OBJECT_DTYPE

EPS = 2.0 ** -24
ONE = 2.0 ** 24
PIXEL = [("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sg.build_library(tmp_path_factory.mktemp("segments"))


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("segments_events"))


_FRAMES = {}


def _frame(events_lib, scene_name, motion, interval, name, W, H):
    """(scene, Object[] of the view, (H * W) records) of tests/native/event_oracle.c, computed once per view."""
    key = (scene_name, motion, interval, name, W, H)
    if key not in _FRAMES:
        scene = eo.load_scene(scene_name, motion, interval)
        camera = sg.CAMERAS[name]
        _FRAMES[key] = (scene, sg.scene_objects(scene, camera), sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1))
    return _FRAMES[key]


def moving_object(beta=0.0, cam=(0.0, 0.0, 0.0, 0.0)):
    """One Object whose rest frame moves at beta along +x through the camera's (gamma from a Pythagorean triple, or at rest)."""
    g = {0.0: 1.0, 0.6: 1.25, -0.6: 1.25}[beta]
    o = np.zeros(1, dtype=OBJECT_DTYPE)
    o["InvLorentz"][0] = [[g, g * beta, 0, 0], [g * beta, g, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    o["Lorentz"][0] = [[g, -g * beta, 0, 0], [-g * beta, g, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    o["stationaryCam"][0] = cam
    return o


def empty_frame(W, H):
    """Every record a miss, every pixel black."""
    records = np.zeros(W * H, dtype=EVENT_DTYPE)
    records["object"] = -1
    return np.zeros(W * H, dtype=PIXEL), records


def rod_between_pixels(objects, camera, W, H, p0, p1, d, rgb, interval=-1, d1=None):
    n = sc.pixel_direction(camera, W, H, np.array([p0[0], p1[0]], dtype=np.float64), np.array([p0[1], p1[1]], dtype=np.float64))
    return segments.from_arrays(pc.rest_position(objects, 0, n[:1], d, interval), pc.rest_position(objects, 0, n[1:], d if d1 is None else d1, interval), 0, rgb)


# ---- 1. the nodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", sg.INTERVALS)
@pytest.mark.parametrize("motion", sg.MOTIONS)
@pytest.mark.parametrize("name", list(sg.CAMERAS))
def test_the_nodes_are_the_particle_oracles_and_lie_where_the_float64_model_puts_them(lib, events_lib, name, motion, interval):
    W, H = 128, 72
    camera = sg.CAMERAS[name]
    scene, objects, records = _frame(events_lib, "cubes", motion, interval, name, W, H)
    segs, groups, _ = sg.crafted(records, objects, camera, W, H, interval)
    segs = segs[np.r_[groups["surface"], groups["near"], groups["far"], groups["in frame"], groups["leaving"], groups["lattice"]]]
    objs = _objects_array(objects)
    a = np.linalg.norm(objs["InvLorentz"].astype(np.float64), ord=2, axis=(1, 2))[segs["object"]]
    for P in (1, 16, 64):
        for flags, inverse_square in ((0, False), (3, True)):
            v = sg.view(camera, W, H, interval, flags, inverse_square=inverse_square)
            got = sg.oracle_nodes(lib, v, objects, segs, P)
            # rule S0 in numpy's float32: d = b - a, pos = a + d * ((float)j / (float)P), the last node b itself
            d = segs["b"] - segs["a"]
            f = (np.arange(P + 1, dtype=np.float32) / np.float32(P)).astype(np.float32)
            want_pos = (segs["a"][:, None, :] + (d[:, None, :] * f[None, :, None]).astype(np.float32)).astype(np.float32)
            want_pos[:, P, :] = segs["b"]
            assert got["pos"].tobytes() == want_pos.tobytes(), f"P = {P}: the node positions"
            # rule S1 IS the particle pass's placement: bit for bit
            lamps = particles.from_arrays(got["pos"].reshape(-1, 3), np.repeat(segs["object"], P + 1), np.repeat(segs["rgb"], P + 1, axis=0))
            assert lamps["pos"].tobytes() == got["pos"].tobytes()
            placed = sg.particle_place(lib, v, objects, lamps)
            for key in ("visible", "X", "Y", "dist", "rgb", "D", "te", "r"):
                assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(placed[key]).tobytes(), f"P = {P} flags {flags}: {key}"
        # ... and within the derived bound of the float64 model
        got = sg.oracle_nodes(lib, sg.view(camera, W, H, interval, 0), objects, segs, P)
        want = segments.project(segs, objects, camera, W, H, interval, 0, dict(pieces=P))
        length = np.linalg.norm(segs["b"].astype(np.float64) - segs["a"].astype(np.float64), axis=1)
        pos = np.linalg.norm(segments.nodes(segs, P), axis=2)
        aa = (a * a)[:, None]
        dn = (16.5 * aa + 4.0) * EPS + 1.43 * aa * EPS * (2.0 * length[:, None] + pos) / want["r"]
        n = want["n"]
        both = got["visible"] & want["visible"]
        if camera["mode"] == "pinhole":
            s = float(eo.lens_scale(camera["v_fov"])) if camera.get("v_fov") else 1.0
            both &= n[..., 2] >= 0.05
            with np.errstate(all="ignore"):
                tol_x = 1.01 * W / (2 * s * (W / H)) * (1 / n[..., 2] + np.abs(n[..., 0]) / n[..., 2] ** 2) * dn + 5 * EPS * (np.abs(want["X"]) + W)
                tol_y = 1.01 * H / (2 * s) * (1 / n[..., 2] + np.abs(n[..., 1]) / n[..., 2] ** 2) * dn + 5 * EPS * (np.abs(want["Y"]) + H)
            dx = got["X"] - want["X"]
        else:
            assert got["visible"].all() and want["visible"].all()
            h_fov, v_fov = float(np.float32(camera.get("h_fov", 2 * math.pi))), float(np.float32(camera.get("v_fov", math.pi)))
            h = np.hypot(n[..., 0], n[..., 2])
            with np.errstate(all="ignore"):
                tol_x = W / h_fov * (np.minimum(1.01 * dn / h, 2 * math.pi) + 100 * EPS) + 4 * EPS * (np.abs(want["X"]) + W)
                tol_y = H / v_fov * (np.minimum(1.01 * dn / h, 1.01 * np.sqrt(2 * dn)) + 20 * EPS) + 4 * EPS * (np.abs(want["Y"]) + H)
            turn = W * 2 * math.pi / h_fov
            dx = (got["X"] - want["X"] + turn / 2) % turn - turn / 2
        dy = got["Y"] - want["Y"]
        assert both.sum() >= 100, both.sum()
        worst_x, worst_y = np.max(np.abs(dx[both]) / tol_x[both]), np.max(np.abs(dy[both]) / tol_y[both])
        rel = np.abs(got["dist"][both] / want["dist"][both] - 1.0) / dn[both]
        print(f"{name} {motion} interval={interval} P={P}: {both.sum()} nodes, largest |dX| / bound {worst_x:.3f}, |dY| / bound {worst_y:.3f}, |d dist| / bound {rel.max():.3f}")
        assert worst_x <= 1.0 and worst_y <= 1.0 and rel.max() <= 1.0
        # the pieces: where no node lies within the bound of a decision, the oracle and the model cut the rod alike
        pieces = sg.oracle_pieces(lib, sg.view(camera, W, H, interval, 0), objects, segs, P)
        same = pieces["placed"] & want["placed"] & (np.abs(want["L"] - np.round(want["L"])) > 0.01) & (want["L"] < 1000.0)
        assert same.sum() >= 30 and np.array_equal(pieces["m"][same], want["m"][same])
        assert np.array_equal(pieces["shift"][same] != 0, want["shift"][same] != 0)


# ---- 2. flux conservation -------------------------------------------------------------------------------------------------------
def _flux_case(lib, objects, camera, W, H, segs, P):
    pixels, records = empty_frame(W, H)
    v = sg.view(camera, W, H, -1, 0)
    _, counts, d = sg.oracle_pass(lib, v, objects, segs, P, pixels, records, details=True)
    t = d["taps"]
    assert (t[..., 1] == 4 * t[..., 0]).all() and (t[..., 2] == t[..., 1]).all(), "every tap inside the frame, over a miss pixel"
    assert (t[..., 0] > 0).all(), "every piece is drawn"
    S = d["acc"].astype(np.float64).sum(axis=0) / ONE
    F = (segs["rgb"].astype(np.float64) * np.linalg.norm(segs["b"].astype(np.float64) - segs["a"].astype(np.float64), axis=1)[:, None]).sum(axis=0)
    return S, F, d


@pytest.mark.parametrize("P", [1, 4, 64])
@pytest.mark.parametrize("beta", [0.0, 0.6])
def test_a_rod_puts_its_whole_flux_into_the_accumulator(lib, P, beta):
    """rgb |b - a| per channel, within the derived bound: 800 random rods per case, of every length on the screen from 0.01 to 60
    pixels a piece, one at a time (so that the bound is held per rod), pinhole and panorama."""
    rng = np.random.default_rng(5)
    objects = moving_object(beta, (0.5, 0.25, -0.5, 1.0))
    worst_low = worst_high = 0.0
    for camera, (W, H) in ((dict(mode="pinhole"), (256, 144)), (dict(mode="equirect"), (256, 128))):
        sets = []
        for _ in range(400):
            L = float(np.exp(rng.uniform(math.log(0.01), math.log(60.0))))
            span = min(L * P, 0.45 * H)
            p0 = rng.uniform((0.3 * W, 0.3 * H), (0.6 * W, 0.6 * H))
            angle = rng.uniform(0.0, 2.0 * math.pi)
            p1 = p0 + span * np.array([math.cos(angle), math.sin(angle)])
            if not (3 < p1[0] < W - 4 and 3 < p1[1] < H - 4):
                p1 = p0 - span * np.array([math.cos(angle), math.sin(angle)])
            sets.append(rod_between_pixels(objects, camera, W, H, p0, p1, rng.uniform(2.0, 9.0), rng.uniform(0.05, 3.0, 3)))
        for rod in sets:
            S, F, d = _flux_case(lib, objects, camera, W, H, rod, P)
            low, high = -(4 * d["samples"] / ONE + 10 * EPS * F), 10 * EPS * F
            assert ((S - F >= low) & (S - F <= high)).all(), f"{camera['mode']} P = {P}: S - F = {S - F}, allowed {low} .. {high}, {d['samples']} samples"
            assert d["most_adds"] <= 4
            worst_low = max(worst_low, float(np.max((F - S) / (4 * d["samples"] / ONE))))
            worst_high = max(worst_high, float(np.max((S - F) / (EPS * F))))
    print(f"P = {P} beta = {beta}: the sums fall short of F by at most {worst_low:.3f} of the truncation term 4 M 2^-24 and exceed F by at most {worst_high:.2f} eps F (bound 10)")


@pytest.mark.parametrize("L", [0.999, 1.0, 1.001, 0.4999, 2.0, 2.0001])
def test_the_flux_is_kept_where_the_number_of_samples_changes(lib, L):
    """Pieces with L just below, at and just above 1 (one sample, then two) and 2."""
    W, H = 320, 72
    camera = dict(mode="pinhole")
    objects = moving_object(0.0)
    for P in (1, 4, 64):
        rod = rod_between_pixels(objects, camera, W, H, (20.25, 30.5), (20.25 + L * P, 30.5), 3.0, (1.0, 0.5, 0.25))
        S, F, d = _flux_case(lib, objects, camera, W, H, rod, P)
        m = sg.oracle_pieces(lib, sg.view(camera, W, H, -1, 0), objects, rod, P)["m"]
        if P == 1:      # (with more pieces the perspective makes the middle ones a little longer on the screen than the outer ones)
            assert set(np.unique(m)) <= {math.ceil(L - 1e-3), math.ceil(L + 1e-3)}, (L, P, np.unique(m))
        low, high = -(4 * d["samples"] / ONE + 10 * EPS * F), 10 * EPS * F
        assert ((S - F >= low) & (S - F <= high)).all(), f"L = {L} P = {P}: S - F = {S - F}, allowed {low} .. {high}"


# ---- 4. the continuum -----------------------------------------------------------------------------------------------------------
def test_a_rod_is_the_limit_of_lamps_along_it(lib):
    """Doppler and the inverse square off: the rod's total flux equals that of as_particles(rod, n), n the samples the rod took, each
    side within its own derived bound of F (the lamps': 4 n 2^-24 of truncation and 6 eps F — the colour's rounding to float32, three
    for the weights, one for the product, and slack for second order).  With beaming and the inverse square on both totals approximate
    the same integral: 4 n lamps come closer to the rod than n lamps did — asserted where the fixed point's truncation does not
    decide it (see below)."""
    W, H = 256, 144
    camera = dict(mode="pinhole")
    objects = moving_object(0.6, (0.0, 0.5, 0.0, -1.0))
    pixels, records = empty_frame(W, H)
    rod = rod_between_pixels(objects, camera, W, H, (40.3, 50.2), (200.7, 110.9), 4.0, (2.0, 1.0, 0.5), d1=7.0)
    P = 64
    v = sg.view(camera, W, H, -1, 0)
    _, _, d = sg.oracle_pass(lib, v, objects, rod, P, pixels, records, details=True)
    n = d["samples"]
    assert n > 150 and (d["taps"][..., 1] == 4 * d["taps"][..., 0]).all()
    S_rod = d["acc"].astype(np.float64).sum(axis=0) / ONE
    lamps = segments.as_particles(rod, n)
    assert len(lamps) == n
    S_lamps = sg.oracle_lamps(lib, v, objects, lamps, records).astype(np.float64).sum(axis=0) / ONE
    F = rod["rgb"][0].astype(np.float64) * float(np.linalg.norm(rod["b"][0].astype(np.float64) - rod["a"][0].astype(np.float64)))
    assert ((S_rod - F >= -(4 * n / ONE + 10 * EPS * F)) & (S_rod - F <= 10 * EPS * F)).all()
    assert ((S_lamps - F >= -(4 * n / ONE + 6 * EPS * F)) & (S_lamps - F <= 6 * EPS * F)).all()
    print(f"flat: rod - F = {S_rod - F}, lamps - F = {S_lamps - F}, n = {n}")
    # beaming and the inverse square on: n lamps and 4 n lamps against the rod.  The lamps' total tends to the integral (the midpoint
    # rule) less the fixed point's truncation, which GROWS with their number (up to 4 x lamps x 2^-24 per channel); the rod keeps the
    # trapezium rule's residual on its 65 nodes.  Four times the lamps are closer to the rod where the midpoint rule's gain from n to
    # 4 n exceeds the 12 n 2^-24 of truncation they add: for a rod 1000 times as bright (the gain scales with the colour, the
    # truncation does not) that holds and is asserted; for the dim rod above it does not, and the figures are printed.
    v = sg.view(camera, W, H, -1, 2, inverse_square=True)
    for scale, asserted in ((1.0, False), (1000.0, True)):
        lit = rod.copy()
        lit["rgb"] = rod["rgb"] * np.float32(scale)
        _, _, d = sg.oracle_pass(lib, v, objects, lit, P, pixels, records, details=True)
        assert d["samples"] == n
        S_rod = d["acc"].astype(np.float64).sum(axis=0) / ONE
        at_n = sg.oracle_lamps(lib, v, objects, segments.as_particles(lit, n), records).astype(np.float64).sum(axis=0) / ONE
        at_4n = sg.oracle_lamps(lib, v, objects, segments.as_particles(lit, 4 * n), records).astype(np.float64).sum(axis=0) / ONE
        print(f"beamed, over r^2, colour x {scale:g}: rod {S_rod}; {n} lamps differ by {at_n - S_rod}, {4 * n} lamps by {at_4n - S_rod} "
              f"(relative {(at_n - S_rod) / S_rod} and {(at_4n - S_rod) / S_rod}); 12 n 2^-24 = {12 * n / ONE:.3g}")
        if asserted:
            assert (np.abs(at_n - S_rod) - np.abs(at_4n - S_rod) > 12 * n / ONE).all(), "the gain from n to 4 n lamps is no more than the truncation they add"
            assert (np.abs(at_4n - S_rod) < np.abs(at_n - S_rod)).all()


# ---- 5. the seam ----------------------------------------------------------------------------------------------------------------
def test_a_piece_across_the_seam_goes_the_short_way(lib):
    W, H = 128, 72
    objects = moving_object(0.0)
    pixels, records = empty_frame(W, H)

    def ends(yaw):
        lam0, lam1 = yaw + math.pi - 0.1, yaw - math.pi + 0.1
        return segments.from_arrays([(3 * math.sin(lam0), 0.3, 3 * math.cos(lam0))], [(3 * math.sin(lam1), 0.3, 3 * math.cos(lam1))], 0, (1.0, 1.0, 1.0))

    full = dict(mode="equirect")
    v = sg.view(full, W, H, -1, 0)
    piece = sg.oracle_pieces(lib, v, objects, ends(0.0), 1)
    nodes = sg.oracle_nodes(lib, v, objects, ends(0.0), 1)
    assert nodes["X"][0, 0] > W - 4 and nodes["X"][0, 1] < 3, nodes["X"]
    assert piece["placed"].all() and piece["shift"][0, 0] == np.float32(W) and 3.0 < piece["L"][0, 0] < 6.0 and piece["m"][0, 0] == math.ceil(piece["L"][0, 0])
    model = segments.project(ends(0.0), objects, full, W, H, -1, 0, dict(pieces=1))
    assert abs(model["shift"][0, 0] - W) < 1e-4 and model["m"][0, 0] == piece["m"][0, 0]       # (the model's period has the float32 h_fov)
    _, counts, d = sg.oracle_pass(lib, v, objects, ends(0.0), 1, pixels, records, details=True)
    lit = np.nonzero(d["acc"].sum(axis=1).reshape(H, W).any(axis=0))[0]
    assert counts[0] == 1 and 0 in lit and W - 1 in lit and ((lit < 4) | (lit >= W - 4)).all(), lit
    S = d["acc"].astype(np.float64).sum(axis=0) / ONE        # ... and the whole flux arrives: no tap is lost at the seam
    F = float(np.linalg.norm(ends(0.0)["b"][0].astype(np.float64) - ends(0.0)["a"][0].astype(np.float64)))
    assert np.all(np.abs(S - F) <= 4 * d["samples"] / ONE + 10 * EPS * F)
    # the other way round: the shift is -W
    back = ends(0.0).copy()
    back["a"], back["b"] = ends(0.0)["b"], ends(0.0)["a"]
    assert sg.oracle_pieces(lib, v, objects, back, 1)["shift"][0, 0] == np.float32(-W)
    # a partial panorama: the same piece is shifted by its period, Px = W 2 pi / h_fov, and lands outside the frame
    partial = sg.CAMERAS["partial"]
    v = sg.view(partial, W, H, -1, 0)
    Px = np.float32(W) * (np.float32(2.0 * math.pi) / np.float32(partial["h_fov"]))
    piece = sg.oracle_pieces(lib, v, objects, ends(partial["yaw"]), 1)
    assert piece["placed"].all() and abs(piece["shift"][0, 0]) == Px and piece["L"][0, 0] < 20.0
    model = segments.project(ends(partial["yaw"]), objects, partial, W, H, -1, 0, dict(pieces=1))
    assert abs(abs(model["shift"][0, 0]) - float(Px)) < 1e-4
    _, counts, _ = sg.oracle_pass(lib, v, objects, ends(partial["yaw"]), 1, pixels, records, details=True)
    assert counts == (0, 0)


# ---- 6. the non-vacuity of the GPU cases, on CPU event frames, and 3. at most 4 adds per word per piece ---------------------------
@pytest.mark.parametrize("size", sg.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(sg.CAMERAS))
@pytest.mark.parametrize("motion", sg.MOTIONS)
@pytest.mark.parametrize("scene_name", sg.SCENES)
def test_the_shared_cases_show_something(lib, events_lib, scene_name, motion, name, size):
    """Per view and per number of pieces: pieces drawn, pieces hidden behind a hit pixel, pieces partly outside the frame (the full
    sphere has no outside, as in §19) and, under the pinhole — the panorama places every direction, and no piece of it can be longer
    than half a turn or the frame's height, both below 1024 here —, pieces dropped for a node behind the pinhole and pieces dropped
    for L > 1024 (the rod through the pinhole's plane: its nodes next to the plane have a small n.z)."""
    W, H = size
    camera = sg.CAMERAS[name]
    pixels = np.zeros(W * H, dtype=PIXEL)
    pixels["rgba"] = (40, 50, 60, 1)
    for interval in sg.INTERVALS:
        scene, objects, records = _frame(events_lib, scene_name, motion, interval, name, W, H)
        segs, groups, bias = sg.crafted(records, objects, camera, W, H, interval)
        hit = records["object"] >= 0
        for P in sg.PIECES:
            what = f"{scene_name} {motion} {name} {W}x{H} interval {interval} pieces {P}"
            sg.check_shows_something(lib, records, objects, camera, W, H, interval, segs, groups, bias, P, what)
            for flags in sg.FLAGS:
                after, (drawn, changed), d = sg.oracle_pass(lib, sg.view(camera, W, H, interval, flags), objects, segs, P, pixels, records, details=True)
                assert 0 < drawn < len(segs) * P and d["most_adds"] <= 4, what
                diff = (after["rgba"] != pixels["rgba"]).any(axis=1)
                assert int(diff.sum()) == changed
                if not flags & 1:       # (at 0.9c the shift moves the crafted colours out of the band)
                    assert diff[hit].any() and diff[~hit].any(), f"{what}: rods show over hit pixels and over miss pixels"
                assert (after["rgba"][:, 3] == 1).all() and np.array_equal(after["x"], pixels["x"]) and np.array_equal(after["unspecified"], pixels["unspecified"])


def test_the_windowed_case_windows_a_piece_out(lib, events_lib):
    W, H = 128, 72
    wl, scene, segs = sg.turnaround()
    camera = sg.CAMERAS["pinhole"]
    windows = scene.windows()
    objects = sg.scene_objects(scene, camera)
    v = sg.view(camera, W, H, -1, 0)
    assert len(segs) == 36
    for P in sg.PIECES:
        free = sg.oracle_pieces(lib, v, objects, segs, P)["placed"]
        held = sg.oracle_pieces(lib, v, objects, segs, P, windows)["placed"]
        assert (free & ~held).any() and held.any() and not (held & ~free).any(), P
    # a rod half inside its window: the clipping has the granularity of a piece
    nodes_free = sg.oracle_nodes(lib, v, objects, segs, 16)
    nodes_held = sg.oracle_nodes(lib, v, objects, segs, 16, windows)
    partly = (nodes_held["visible"].any(axis=1) & (nodes_free["visible"] & ~nodes_held["visible"]).any(axis=1))
    print(f"{int(partly.sum())} of {len(segs)} rods are cut by their object's window")
    records = sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1)
    pixels = np.zeros(W * H, dtype=PIXEL)
    plain = sg.oracle_pass(lib, v, objects, segs, 16, pixels, records)
    default = np.tile(np.array([-np.inf, np.inf], dtype=np.float32), (len(windows), 1))
    assert sg.oracle_pass(lib, v, objects, segs, 16, pixels, records, default)[0].tobytes() == plain[0].tobytes()
    windowed = sg.oracle_pass(lib, v, objects, segs, 16, pixels, records, windows)
    assert 0 < windowed[1][0] < plain[1][0]


# ---- the chord table of DESIGN.md §22 (printed; nothing is asserted on the distances) ---------------------------------------------
@pytest.mark.parametrize("motion", sg.MOTIONS)
@pytest.mark.parametrize("scene_name", sg.SCENES)
def test_how_far_a_chords_midpoint_lies_from_the_rods_true_midpoint(events_lib, scene_name, motion):
    """For pieces 1, 8 and 64 and the four cameras at 128 x 72, interval -1: the largest distance, in pixels, between the midpoint of a
    piece's chord and segments' float64 projection of the rod's true midpoint, for the crafted set's rod_lattice and for its three
    rods across the frame.  Run with -s to see the table DESIGN.md §22 holds."""
    W, H = 128, 72
    for P in (1, 8, 64):
        worst = {"lattice": 0.0, "in frame": 0.0}
        for name, camera in sg.CAMERAS.items():
            scene, objects, records = _frame(events_lib, scene_name, motion, -1, name, W, H)
            segs, groups, _ = sg.crafted(records, objects, camera, W, H, -1)
            p = segments.project(segs, objects, camera, W, H, -1, 0, dict(pieces=P))
            pos = segments.nodes(segs, P)
            mid = 0.5 * (pos[:, :-1] + pos[:, 1:])
            q = particles.project_columns(mid.reshape(-1, 3), np.repeat(segs["object"].astype(np.int64), P), np.ones((len(segs) * P, 3)), objects, camera, W, H, -1, 0)
            X, Y = q["X"].reshape(len(segs), P), q["Y"].reshape(len(segs), P)
            dx = X - 0.5 * (p["X"][:, :-1] + p["X"][:, 1:] + p["shift"])
            if camera.get("mode") == "equirect":
                turn = W * 2 * math.pi / float(np.float32(camera.get("h_fov", 2 * math.pi)))
                dx = (dx + turn / 2) % turn - turn / 2
            d = np.hypot(dx, Y - 0.5 * (p["Y"][:, :-1] + p["Y"][:, 1:]))
            ok = p["placed"] & (p["m"] > 0) & np.isfinite(d)
            for what in worst:
                g = groups[what]
                if ok[g].any():
                    worst[what] = max(worst[what], float(d[g][ok[g]].max()))
        print(f"{scene_name} {motion} pieces {P}: rod_lattice {worst['lattice']:.4f} px, rods across the frame {worst['in frame']:.4f} px")
        assert all(math.isfinite(v) for v in worst.values())


# ---- 7. the Python layer --------------------------------------------------------------------------------------------------------
def test_the_builders_save_load_and_what_the_python_layer_refuses(tmp_path):
    line = segments.polyline([(0, 0, 0), (1, 0, 0), (1, 2, 0)], 3, (0.5, 0.25, 1.0))
    assert len(line) == 2 and (line["object"] == 3).all() and line["a"][1].tolist() == [1.0, 0.0, 0.0] and line["b"][1].tolist() == [1.0, 2.0, 0.0]
    box = segments.box_edges(1, (-1, -2, -3), (1, 2, 3), (1.0, 1.0, 1.0))
    assert len(box) == 12
    lengths = sorted(np.linalg.norm(box["b"] - box["a"], axis=1).tolist())
    assert lengths == [2.0] * 4 + [4.0] * 4 + [6.0] * 4
    corners = {tuple(c) for c in np.concatenate([box["a"], box["b"]]).tolist()}
    assert len(corners) == 8
    lattice = segments.rod_lattice(0, (0, 0, 0), (2, 2, 2), 2, (1.0, 1.0, 1.0))
    assert len(lattice) == 3 * 2 * 3 * 3 and np.allclose(np.linalg.norm(lattice["b"] - lattice["a"], axis=1), 1.0)
    assert len({(tuple(a), tuple(b)) for a, b in zip(lattice["a"].tolist(), lattice["b"].tolist())}) == len(lattice)
    assert len(segments.rod_lattice(0, (0, 0, 0), (1, 1, 1), (1, 2, 3), (1, 1, 1))) == 1 * 3 * 4 + 2 * 2 * 4 + 3 * 2 * 3
    assert segments.SEGMENT_DTYPE.itemsize == 48 and [segments.SEGMENT_DTYPE.fields[k][1] for k in ("a", "object", "b", "_pad0", "rgb", "_pad1")] == [0, 12, 16, 28, 32, 44]
    lamps = segments.as_particles(box, 5)
    assert len(lamps) == 60 and lamps.dtype == particles.PARTICLE_DTYPE
    assert np.allclose(lamps["rgb"].astype(np.float64).sum(axis=0), np.linalg.norm(box["b"] - box["a"], axis=1).sum())
    assert np.allclose(lamps["pos"][:5, :], box["a"][0] + (box["b"][0] - box["a"][0]) * ((np.arange(5) + 0.5) / 5)[:, None])
    assert len(segments.as_particles(box[:3], [1, 2, 3])) == 6
    path = tmp_path / "rods.bin"
    segments.save(path, box)
    assert path.stat().st_size == 48 * 12 and segments.load(path).tobytes() == box.tobytes()
    path.write_bytes(b"\0" * 49)
    with pytest.raises(ValueError):
        segments.load(path)
    obj = moving_object(0.6)
    with pytest.raises(ValueError):
        segments.project(box, obj, dict(mode="equirect"), 64, 32, 2)
    with pytest.raises(ValueError):
        segments.project(box, obj, dict(mode="equirect"), 64, 32, -1, 0, dict(pieces=3))
    with pytest.raises(ValueError):
        segments.from_arrays([(0, 0, 0)], [(1, 1, 1), (2, 2, 2)], 0, (1, 1, 1))
    with pytest.raises(ValueError):
        segments.polyline([(0, 0, 0)], 0, (1, 1, 1))
    with pytest.raises(ValueError):
        segments.rod_lattice(0, (0, 0, 0), (1, 1, 1), 0, (1, 1, 1))
    with pytest.raises(ValueError):
        segments.as_particles(box, 0)
    box["object"] = 0
    p = segments.project(box, obj, dict(mode="equirect"), 64, 32, -1, 3, dict(pieces=4, inverse_square=True))
    assert p["X"].shape == (12, 5) and p["m"].shape == (12, 4) and p["rgb"].shape == (12, 5, 3) and p["placed"].all()
