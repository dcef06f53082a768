"""events.readout, the numpy restatement of the readout pass (include/rpt.h, rpt_set_readouts; DESIGN.md "Readout pass"), on hand-built
records whose (u, v) is a flat pixel grid — every expectation below is written out, not recomputed by the code under test — and the
non-vacuity of the cases tests/test_gpu_readout.py runs (tests/readout_cases.py), on CPU records.  No GPU."""
import numpy as np
import pytest

import events_oracle as eo
import readout_cases as rc
from relativitypathtracer_amd.events import EVENT_DTYPE, readout, readout_coverage, readout_settings

INF, NAN = float("inf"), float("nan")
RED = dict(on_rgba=(255, 0, 0, 255), off_rgba=(0, 0, 0, 0))


def _grid(W, H, value=0.0, objects=None):
    """(H, W) records whose (u, v) is the pixel's centre in pixels and whose event[0] is `value`; object 0 unless given."""
    ev = np.zeros((H, W), dtype=EVENT_DTYPE)
    y, x = np.mgrid[0:H, 0:W]
    ev["object"] = 0 if objects is None else np.asarray(objects, dtype=np.int32)
    ev["uv"][..., 0], ev["uv"][..., 1] = x + 0.5, y + 0.5
    ev["event"][..., 0] = value
    return ev


def _black(ev, alpha=9):
    img = np.zeros(ev.shape + (4,), dtype=np.uint8)
    img[..., 3] = alpha
    return img


def _art(img):
    """The red channel as text, the top row first: # fully lit, . untouched, ? anything else."""
    return ["".join("#" if p == 255 else "." if p == 0 else "?" for p in row) for row in img[::-1, :, 0]]


# 16 x 16 pixels a cell: every segment boundary of the table is a pixel edge, so a pixel is lit wholly or not at all
GOLDEN_01234 = """
................................................................................
...########........................########........########.....................
..##########..............##.......#########.......#########......##......##....
..##......##..............##..............##..............##......##......##....
..##......##..............##..............##..............##......##......##....
..##......##..............##..............##..............##......##......##....
..##......##..............##..............##..............##......##......##....
..##......##..............##.......#########.......#########......##########....
..##......##..............##......#########........#########.......#########....
..##......##..............##......##......................##..............##....
..##......##..............##......##......................##..............##....
..##......##..............##......##......................##..............##....
..##......##..............##......##......................##..............##....
..##########..............##......#########........#########..............##....
...########........................########........########.....................
................................................................................
""".split()
GOLDEN_56789 = """
................................................................................
...########........########........########........########........########.....
..#########.......#########........#########......##########......##########....
..##..............##......................##......##......##......##......##....
..##..............##......................##......##......##......##......##....
..##..............##......................##......##......##......##......##....
..##..............##......................##......##......##......##......##....
..#########.......#########...............##......##########......##########....
...#########......##########..............##......##########.......#########....
..........##......##......##..............##......##......##..............##....
..........##......##......##..............##......##......##..............##....
..........##......##......##..............##......##......##..............##....
..........##......##......##..............##......##......##..............##....
...#########......##########..............##......##########.......#########....
...########........########........................########........########.....
................................................................................
""".split()


@pytest.mark.parametrize("value, golden", [(1234.0, GOLDEN_01234), (56789.0, GOLDEN_56789)], ids=["01234", "56789"])
def test_the_ten_digits_against_art_drawn_by_hand(value, golden):
    ev = _grid(80, 16, value)
    img, changed = readout(_black(ev), ev, [dict(rate=1.0, offset=0.0, digits=5, decimals=0, rect=(0, 0, 80, 16), **RED)])
    assert _art(img) == golden
    assert changed == sum(row.count("#") for row in golden)
    assert (img[..., 1:3] == 0).all() and (img[..., 3] == 9).all()


# one pixel inside each box of the segment table at 16 pixels a cell: a b c d e f g point
PROBES = ((6, 14), (10, 10), (10, 4), (6, 1), (2, 4), (2, 10), (6, 7), (13, 1))


def _cells(value, digits, decimals=0, rate=1.0, offset=0.0):
    """The masks (a = bit 0 .. g = bit 6, the point bit 7) the cells show for event[0] = value, read off the picture at 16 pixels a cell."""
    ev = _grid(16 * digits, 16, value)
    with np.errstate(all="ignore"):
        img, _ = readout(_black(ev), ev, [dict(rate=rate, offset=offset, digits=digits, decimals=decimals, rect=(0, 0, 16 * digits, 16), **RED)])
    assert set(np.unique(img[..., 0]).tolist()) <= {0, 255}
    return [sum(1 << bit for bit, (x, y) in enumerate(PROBES) if img[y, 16 * k + x, 0] == 255) for k in range(digits)]


MINUS, D = 0x40, (0x3f, 0x06, 0x5b, 0x4f, 0x66, 0x6d, 0x7d, 0x07, 0x7f, 0x6f)


def test_the_minus_sign_takes_the_first_cell():
    assert _cells(-12.5, 5, 1) == [MINUS, D[0], D[1], D[2] | 0x80, D[5]]
    assert _cells(-99.0, 3) == [MINUS, D[9], D[9]]
    assert _cells(-0.25, 3) == [MINUS, D[0], D[0]]              # floorf(|-0.25|) = 0: "-00"
    assert _cells(-0.0, 3) == [D[0], D[0], D[0]]                # -0.0 < 0 is false


def test_overflow_shows_dashes_and_no_point():
    dashes = [MINUS] * 3
    assert _cells(999.0, 3) == [D[9], D[9], D[9]]
    assert _cells(1000.0, 3) == dashes
    assert _cells(-100.0, 3) == dashes                          # the sign leaves two cells
    assert _cells(99.9, 3, 1) == [D[9], D[9] | 0x80, D[9]]
    assert _cells(100.0, 3, 1) == dashes                        # ... and no decimal point
    for v in (NAN, INF, -INF, 2.0e9, -3.0e38):
        assert _cells(v, 3, 1) == dashes, v
    assert _cells(999999999.0, 9) == [MINUS] * 9                # (float)999999999 is 1e9
    assert _cells(1.0e9, 9) == [MINUS] * 9
    assert _cells(999999936.0, 9) == [D[9]] * 6 + [D[9], D[3], D[6]]       # the largest float below 1e9


def test_the_value_is_rate_times_the_clock_plus_the_offset_floored():
    assert _cells(3.99, 2) == [D[0], D[3]]
    assert _cells(3.999, 4, 2) == [D[0], D[3] | 0x80, D[9], D[9]]
    assert _cells(2.0, 3, rate=-3.0, offset=10.5) == [D[0], D[0], D[4]]
    assert _cells(7.0, 4, 3) == [D[7] | 0x80, D[0], D[0], D[0]]


def test_the_decimal_points_cell():
    for decimals in range(1, 7):
        cells = _cells(0.0, 8, decimals)
        assert [k for k, m in enumerate(cells) if m & 0x80] == [8 - 1 - decimals]
    assert not any(m & 0x80 for m in _cells(0.0, 8, 0))


def test_one_digit():
    assert _cells(7.0, 1) == [D[7]]
    assert _cells(-0.5, 1) == [MINUS]
    assert _cells(10.0, 1) == [MINUS]


def test_a_mirrored_rectangle_mirrors_the_picture():
    ev = _grid(80, 16, 1234.0)
    plain, _ = readout(_black(ev), ev, [dict(digits=5, rect=(0, 0, 80, 16), **RED)])
    in_u, _ = readout(_black(ev), ev, [dict(digits=5, rect=(80, 0, 0, 16), **RED)])
    in_v, _ = readout(_black(ev), ev, [dict(digits=5, rect=(0, 16, 80, 0), **RED)])
    assert _art(plain) == GOLDEN_01234
    assert np.array_equal(in_u, plain[:, ::-1]) and np.array_equal(in_v, plain[::-1])


def test_the_footprint_is_zero_at_an_objects_edge_and_at_the_frames():
    """The rectangle begins a quarter of a pixel into column 2 and row 2: of a pixel's four sub-sample columns (its centre -0.375, -0.125,
    +0.125, +0.375) the first falls outside, so 12 of 16 sub-samples are inside — unless the pixel has no right (upper) neighbour of its
    own object, when all 16 sit on its centre."""
    one = [dict(digits=1, rect=(2.25, 0, 66.25, 64))]
    for W, objects, want in ((4, None, 12), (3, None, 16), (4, [[0, 0, 0, 1]] * 2, 16), (4, [[0, 0, 0, -1]] * 2, 16)):
        ev = _grid(W, 2, objects=objects)
        _, n_in, _, _ = readout_coverage(ev, one + [None])
        assert n_in[0, 2] == want and n_in[0, 1] == 0, (W, objects)
    up = [dict(digits=1, rect=(0, 2.25, 64, 66.25))]
    for H, objects, want in ((4, None, 12), (3, None, 16), (4, [[0], [0], [0], [1]], 16)):
        ev = _grid(1, H, objects=objects)
        _, n_in, _, _ = readout_coverage(ev, up + [None])
        assert n_in[2, 0] == want and n_in[1, 0] == 0, (H, objects)
    # both at once: 3 of 4 columns times 3 of 4 rows
    ev = _grid(4, 4)
    _, n_in, _, _ = readout_coverage(ev, [dict(digits=1, rect=(2.25, 2.25, 66.25, 66.25))])
    assert n_in[2, 2] == 9 and n_in[2, 3] == 12 and n_in[3, 2] == 12 and n_in[3, 3] == 16


def test_one_row_and_one_column_frames():
    row = _grid(80, 1, 1234.0)
    row["uv"][..., 1] = 7.5                                     # the row through the middle bars
    img, changed = readout(_black(row), row, [dict(digits=5, rect=(0, 0, 80, 16), **RED)])
    assert _art(img) == [GOLDEN_01234[8]] and changed == GOLDEN_01234[8].count("#")
    col = _grid(1, 16, 8.0)
    col["uv"][..., 0] = 11.5                                    # the column through segments b and c of an 8, right of its bars
    img, changed = readout(_black(col), col, [dict(digits=1, rect=(0, 0, 16, 16), **RED)])
    assert "".join(r for r in _art(img)) == "..############.." and changed == 12


def test_the_two_step_blend_rounds_as_stated_and_leaves_alpha():
    """One cell of 16 x 16 pixels that begins a quarter of a pixel into column 2 and shows an 8.  Pixel (2, 0): 12 sub-samples inside, none
    lit.  Pixel (4, 4): all inside, and three of its four sub-sample columns (cell x 2.125, 2.375, 2.625 of 1.875 ..) in segment e."""
    ev = _grid(20, 16, 8.0)
    before = _black(ev, alpha=77)
    before[..., :3] = (10, 20, 30)
    img, _ = readout(before, ev, [dict(digits=1, rect=(2.25, 0, 18.25, 16), on_rgba=(255, 0, 0, 255), off_rgba=(200, 100, 50, 160))])
    _, n_in, n_on, _ = readout_coverage(ev, [dict(digits=1, rect=(2.25, 0, 18.25, 16))])
    assert (n_in[0, 2], n_on[0, 2]) == (12, 0) and (n_in[4, 4], n_on[4, 4]) == (16, 12)
    # (160 * 12 + 8) // 16 = 120: (200 * 120 + 10 * 135 + 127) // 255 = 99, (100 * 120 + 20 * 135 + 127) // 255 = 58, (50 * 120 + 30 * 135 + 127) // 255 = 39
    assert img[0, 2].tolist() == [99, 58, 39, 77]
    # off with 160: 129, 70, 43; then on with (255 * 12 + 8) // 16 = 191: (255 * 191 + 129 * 64 + 127) // 255 = 223, (70 * 64 + 127) // 255 = 18, 11
    assert img[4, 4].tolist() == [223, 18, 11, 77]
    assert img[0, 0].tolist() == [10, 20, 30, 77] and (img[..., 3] == 77).all()


def test_applying_the_pass_twice_blends_twice():
    ev = _grid(20, 16, 8.0)
    ro = [dict(digits=1, rect=(2.25, 0, 18.25, 16), on_rgba=(255, 0, 0, 128), off_rgba=(200, 100, 50, 160))]
    before = _black(ev)
    once, n1 = readout(before, ev, ro)
    twice, n2 = readout(once, ev, ro)
    assert n1 > 0 and n2 > 0 and not np.array_equal(once, twice)
    assert (before[..., 3] == twice[..., 3]).all()
    # (4, 4) again: off 160 then on (128 * 12 + 8) // 16 = 96, from black: R (200 * 160 + 127) // 255 = 125 -> (255 * 96 + 125 * 159 + 127) // 255 = 174
    assert once[4, 4, 0] == 174
    # ... and from there: (200 * 160 + 174 * 95 + 127) // 255 = 190 -> (255 * 96 + 190 * 159 + 127) // 255 = 214
    assert twice[4, 4, 0] == 214


def test_objects_without_a_display_and_misses_stay():
    objects = np.zeros((16, 48), dtype=np.int32)
    objects[:, 16:32], objects[:, 32:] = 1, -1
    ev = _grid(48, 16, 8.0, objects)
    ro = [dict(digits=3, rect=(0, 0, 48, 16), **RED), None]
    img, changed = readout(_black(ev), ev, ro)
    assert (img[:, 16:, :3] == 0).all() and changed == (img[:, :16, 0] == 255).sum() > 0
    same, none = readout(_black(ev), ev, [None, None])
    assert none == 0 and (same[..., :3] == 0).all()
    assert readout(_black(ev), ev, [])[1] == 0 and readout(_black(ev), ev, None)[1] == 0
    with pytest.raises(ValueError):                             # one entry per object
        readout(_black(ev), ev, ro[:1])


def test_every_refusal():
    good = dict(rate=1.0, offset=0.0, digits=4, decimals=2, rect=(0.1, 0.2, 0.9, 0.8))
    assert readout_settings(**good)["digits"] == 4
    bad = [dict(digits=10), dict(digits=-1), dict(decimals=7, digits=9), dict(decimals=4), dict(decimals=5), dict(rect=(0.5, 0.2, 0.5, 0.8)),
           dict(rect=(0.1, 0.3, 0.9, 0.3)), dict(rate=NAN), dict(rate=INF), dict(offset=-INF), dict(rect=(0.1, NAN, 0.9, 0.8)),
           dict(rect=(0.1, 0.2, INF, 0.8)), dict(rect=(0.1, 0.2, 0.9)), dict(on_rgba=(0, 0, 256, 0)), dict(off_rgba=(0, 0, 0))]
    for change in bad:
        with pytest.raises(ValueError):
            readout_settings(**dict(good, **change))
    assert readout_settings(digits=1, decimals=0)["rect"] == tuple(np.float32(c) for c in (0.1, 0.25, 0.9, 0.75))
    assert readout_settings()["digits"] == 0                    # no display: nothing else is asked of it
    assert readout_settings(digits=0, decimals=9, rect=(0, 0, 0, 0))["digits"] == 0
    ev = _grid(4, 4)
    with pytest.raises(ValueError):
        readout(_black(ev), ev, [dict(good, digits=10)])
    with pytest.raises(ValueError):
        readout(_black(ev), ev[0], [good])


# ---- the GPU cases show something: on CPU records of the same scenes, cameras and sizes -------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("readout"))


@pytest.fixture(scope="module")
def scenes():
    return rc.scenes()


def _kinds(ev, readouts):
    shown, n_in, n_on, value = readout_coverage(ev, readouts)
    obj = ev["object"]
    has = np.array([d is not None and d["digits"] != 0 for d in readouts])
    on_display_object = (obj >= 0) & has[np.clip(obj, 0, len(readouts) - 1)]
    assert np.array_equal(shown, on_display_object)
    kinds = {"every sub-sample lit": shown & (n_on == 16), "some sub-samples lit": shown & (n_on > 0) & (n_on < 16),
             "inside the rectangle and dark": shown & (n_in == 16) & (n_on == 0), "the display's object outside the rectangle": shown & (n_in == 0),
             "an object without a display": (obj >= 0) & ~shown, "a miss": obj < 0}
    return {k: int(m.sum()) for k, m in kinds.items()}, np.unique(value[shown & (n_in > 0)]).size


@pytest.mark.parametrize("name, camera, size", rc.CASES + [("turnaround", "pinhole", s) for s in rc.SIZES[:2]],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_every_gpu_case_has_pixels_of_every_kind(lib, scenes, name, camera, size):
    scene, readouts = scenes[name]
    counts, values = _kinds(rc.cpu_events(lib, scene, *size, camera), readouts)
    assert all(n >= 1 for n in counts.values()), counts
    if name in ("cube", "strip", "many", "turnaround"):         # a moving face: the relativity of simultaneity, pixel by pixel
        assert values >= 2


def test_the_sphere_cases_seam_lies_inside_the_rectangle(lib, scenes):
    scene, readouts = scenes["sphere"]
    ev = rc.cpu_events(lib, scene, 128, 72, "pinhole")
    _, n_in, _, _ = readout_coverage(ev, readouts)
    u, obj = ev["uv"][..., 0], ev["object"]
    seam = (np.abs(u[:, 1:] - u[:, :-1]) > 0.5) & (obj[:, 1:] == 0) & (obj[:, :-1] == 0)
    assert (seam & (n_in[:, :-1] > 0)).sum() >= 5


def test_the_many_objects_display_is_beyond_the_first_64(scenes):
    scene, readouts = scenes["many"]
    assert len(scene.objects()) == 70 == len(readouts) and [k for k, d in enumerate(readouts) if d] == [66]
