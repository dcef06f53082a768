"""events.overlay, the numpy restatement of the overlay pass (include/rpt.h, rpt_set_overlay; DESIGN.md "Overlay pass"), on hand-built
records — every expectation below is written out, not recomputed by the code under test — then its tint against events.delay_map, and
the non-vacuity of the layer settings tests/test_gpu_overlay.py runs (tests/overlay_cases.py).  No GPU."""
import numpy as np
import pytest

import events_oracle as eo
import overlay_cases as oc
from relativitypathtracer_amd.events import EVENT_DTYPE, delay_map, overlay, overlay_settings

INF, NAN = float("inf"), float("nan")


def _records(objects, dist=None, clock=None):
    """(H, W) records from an (H, W) list of object indices (row 0 the bottom row), with `dist` and event[0] where given."""
    obj = np.asarray(objects, dtype=np.int32)
    ev = np.zeros(obj.shape, dtype=EVENT_DTYPE)
    ev["object"] = obj
    if dist is not None:
        ev["dist"] = np.asarray(dist, dtype=np.float32)
    if clock is not None:
        ev["event"][..., 0] = np.asarray(clock, dtype=np.float32)
    return ev


def _black(ev, alpha=9):
    img = np.zeros(ev.shape + (4,), dtype=np.uint8)
    img[..., 3] = alpha
    return img


def _mask(img):
    """Which pixels are no longer black."""
    return (img[..., :3] != 0).any(axis=-1).astype(int)


def test_a_ramp_of_the_clock_draws_one_pixel_lines_between_cells():
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    ev = _records(np.zeros((8, 8)), clock=0.5 * (x + y))           # cell = floor((x + y) / 2) with step 1
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0, clock_rgba=(10, 20, 30, 255))
    want = np.array([[0, 1, 0, 1, 0, 1, 0, 1],
                     [1, 0, 1, 0, 1, 0, 1, 0],
                     [0, 1, 0, 1, 0, 1, 0, 1],
                     [1, 0, 1, 0, 1, 0, 1, 0],
                     [0, 1, 0, 1, 0, 1, 0, 1],
                     [1, 0, 1, 0, 1, 0, 1, 0],
                     [0, 1, 0, 1, 0, 1, 0, 1],
                     [1, 0, 1, 0, 1, 0, 1, 0]])                      # (7, 7) has no neighbour inside the frame, and x + y = 14 is even anyway
    assert np.array_equal(_mask(img), want)
    assert changed == 32
    assert (img[want == 1] == (10, 20, 30, 9)).all() and (img[want == 0] == (0, 0, 0, 9)).all()
    # a ramp along x only: the lines are columns, and the last column has no right neighbour to differ from
    ev = _records(np.zeros((8, 8)), clock=0.5 * x)                  # cells 0 0 1 1 2 2 3 3
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)
    assert np.array_equal(_mask(img), np.array([[0, 1, 0, 1, 0, 1, 0, 0]] * 8)) and changed == 24
    # the step scales the cells: step 2 over the same ramp gives cells 0 0 0 0 1 1 1 1
    img, changed = overlay(_black(ev), ev, -1, clock_step=2.0)
    assert np.array_equal(_mask(img), np.array([[0, 0, 0, 1, 0, 0, 0, 0]] * 8)) and changed == 8


def test_two_objects_side_by_side():
    ev = _records([[0, 0, 1, 1]] * 3, clock=[[0, 0, 5, 5]] * 3)
    img, changed = overlay(_black(ev), ev, -1, outlines=True)
    assert np.array_equal(_mask(img), np.array([[0, 1, 0, 0]] * 3)) and changed == 3       # the left pixel of the pair carries the line
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)                              # a contour never runs between two objects
    assert np.array_equal(_mask(img), np.zeros((3, 4), dtype=int)) and changed == 0


def test_a_miss_next_to_a_hit():
    ev = _records([[-1, 0, 0],
                   [-1, -1, 0]], clock=[[3, 0, 0], [4, 5, 0]], dist=[[0, 2, 2], [0, 0, 2]])
    img, changed = overlay(_black(ev), ev, -1, outlines=True)
    assert np.array_equal(_mask(img), np.array([[1, 1, 0],
                                                [0, 1, 0]])) and changed == 3                # hit against miss counts, from either side
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)                              # a miss is never on a contour, whatever its record holds
    assert changed == 0
    img, changed = overlay(_black(ev), ev, -1, tint=True, tint_t_max=4.0, tint_alpha=255)   # the tint is for hit pixels only
    assert np.array_equal(_mask(img), np.array([[0, 1, 1],
                                                [0, 0, 1]])) and changed == 3
    assert (img[0, 1] == (64, 255, 64, 9)).all()                                            # x = 2 / 4: the green knot


def test_a_non_finite_distance():
    ev = _records([[0, 0, 0, 0]], dist=[[1.0, INF, 3.0, 4.5]])
    img, changed = overlay(_black(ev), ev, -1, delay_step=1.0)
    assert np.array_equal(_mask(img), [[0, 0, 1, 0]]) and changed == 1      # cells 1, none, 3, 4: the infinite one neither is on a line nor makes pixel 0 one
    ev = _records([[0, 0, 0, 0]], dist=[[1.0, NAN, 3.0, 3.0]])
    img, changed = overlay(_black(ev), ev, -1, delay_step=1.0)
    assert changed == 0
    # the tint takes a delay that is not finite as 0, also when it looks for the frame's largest
    ev = _records([[0, 0, 0]], dist=[[INF, 4.0, NAN]])
    for t_max in (4.0, 0.0):
        img, changed = overlay(_black(ev), ev, -1, tint=True, tint_t_max=t_max, tint_alpha=255)
        assert np.array_equal(img[0, :, :3], [[255, 64, 64], [64, 64, 255], [255, 64, 64]]) and changed == 3


def test_a_product_beyond_two_to_the_thirty():
    ev = _records([[0, 0, 0, 0]], clock=[[0.0, 1.0, 2.0 ** 31, 2.0 ** 31 + 512.0]])
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)
    assert np.array_equal(_mask(img), [[1, 0, 0, 0]]) and changed == 1
    # the bound itself: 2^30 - 64 is the largest float below 2^30 and still has a cell, 2^30 has none
    ev = _records([[0, 0, 0, 0]], clock=[[2.0 ** 30 - 128.0, 2.0 ** 30 - 64.0, 2.0 ** 30, 2.0 ** 30 + 128.0]])
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)
    assert np.array_equal(_mask(img), [[1, 0, 0, 0]]) and changed == 1
    ev = _records([[0, 0, 0]], clock=[[-(2.0 ** 30), -(2.0 ** 30) + 64.0, -(2.0 ** 30) + 128.0]])      # the magnitude counts
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)
    assert np.array_equal(_mask(img), [[0, 1, 0]]) and changed == 1
    # the PRODUCT decides, not the scalar: a small step takes a modest value over the bound
    ev = _records([[0, 0, 0]], clock=[[1.0, 2.0, 3.0]])
    img, changed = overlay(_black(ev), ev, -1, clock_step=2.0 ** -30)
    assert changed == 0


def test_a_one_row_frame_and_a_one_column_frame():
    ev = _records([[0, 0, 1, 1, -1]], clock=[[0, 1, 1, 2, 3]])
    img, changed = overlay(_black(ev), ev, -1, outlines=True)
    assert np.array_equal(_mask(img), [[0, 1, 0, 1, 0]]) and changed == 2
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)
    assert np.array_equal(_mask(img), [[1, 0, 1, 0, 0]]) and changed == 2
    ev = _records([[0], [1], [1], [-1], [-1]], clock=[[0], [0], [1], [2], [3]])      # bottom to top
    img, changed = overlay(_black(ev), ev, -1, outlines=True)
    assert np.array_equal(_mask(img), [[1], [0], [1], [0], [0]]) and changed == 2
    img, changed = overlay(_black(ev), ev, -1, clock_step=1.0)
    assert np.array_equal(_mask(img), [[0], [1], [0], [0], [0]]) and changed == 1
    ev = _records([[0]], clock=[[1.5]])                                               # one pixel: no neighbour at all
    assert overlay(_black(ev), ev, -1, outlines=True, clock_step=1.0, delay_step=1.0, lattice_step=1.0)[1] == 0


def test_the_blend_rounds_as_stated_and_leaves_alpha():
    ev = _records([[0, 1]])
    img = np.array([[[0, 255, 100, 77], [1, 2, 3, 4]]], dtype=np.uint8)
    out, changed = overlay(img, ev, -1, outlines=True, outline_rgba=(255, 0, 200, 128))
    # (255 * 128 + 0 * 127 + 127) // 255 = 128;  (0 + 255 * 127 + 127) // 255 = 127;  (200 * 128 + 100 * 127 + 127) // 255 = 150
    assert out[0, 0].tolist() == [128, 127, 150, 77] and out[0, 1].tolist() == [1, 2, 3, 4] and changed == 1
    out, _ = overlay(np.zeros((1, 2, 4), np.uint8), ev, -1, outlines=True, outline_rgba=(255, 255, 255, 1))
    assert out[0, 0].tolist() == [1, 1, 1, 0]                        # (255 + 127) // 255
    out, changed = overlay(img, ev, -1, outlines=True, outline_rgba=(9, 9, 9, 0))
    assert np.array_equal(out, img) and changed == 0                 # weight 0 changes nothing, and nothing is counted
    assert img[0, 0].tolist() == [0, 255, 100, 77]                   # the caller's array is not written


def test_the_tint_ramp_and_its_range():
    ev = _records([[0, 0, 0, 0, 0]], dist=[[0.0, 1.0, 2.0, 4.0, 8.0]])
    want = [[255, 64, 64], [159, 159, 64], [64, 255, 64], [64, 64, 255], [64, 64, 255]]       # x = 0, 1/4, 1/2, 1, clamped
    img, changed = overlay(_black(ev), ev, -1, tint=True, tint_t_max=4.0, tint_alpha=255)
    assert img[0, :, :3].tolist() == want and changed == 5 and (img[..., 3] == 9).all()
    ev4 = ev[:, :4]
    img, _ = overlay(_black(ev4), ev4, -1, tint=True, tint_alpha=255)                          # the frame's own largest delay is 4
    assert img[0, :, :3].tolist() == want[:4]
    img, _ = overlay(_black(ev), ev, 0, tint=True, tint_alpha=255)                             # light delay off: every delay is 0
    assert img[0, :, :3].tolist() == [[255, 64, 64]] * 5
    img, _ = overlay(_black(ev), ev, -1, tint=True, tint_t_max=4.0, tint_alpha=128)
    assert img[0, 1, :3].tolist() == [80, 80, 32]                    # (159 * 128 + 127) // 255, (64 * 128 + 127) // 255


def test_layers_go_on_in_the_stated_order():
    # pixel 0: a clock line, a delay line and a lattice line at once on a tinted pixel; pixel 1: an outline; every layer opaque: the last one wins
    two = _records([[0, 0, 1]], dist=[[1.0, 2.0, 2.0]], clock=[[0.0, 1.0, 1.0]])
    two["event"][0, :, 1] = [0.0, 1.0, 1.0]
    kw = dict(clock_step=1.0, clock_rgba=(0, 255, 255, 255), delay_step=1.0, delay_rgba=(255, 255, 0, 255), lattice_step=(1.0, 0.0, 0.0),
              lattice_rgba=(255, 0, 255, 255), tint=True, tint_t_max=2.0, tint_alpha=255)
    img, _ = overlay(_black(two), two, -1, **kw)
    assert img[0, 0, :3].tolist() == [255, 255, 0]                   # the delay line lies over the clock line, the lattice and the tint
    assert img[0, 1, :3].tolist() == [64, 64, 255]                   # no line here: the tint shows (x = 1)
    img, _ = overlay(_black(two), two, -1, **dict(kw, delay_step=None))
    assert img[0, 0, :3].tolist() == [0, 255, 255]                   # ... the clock line over the lattice
    img, _ = overlay(_black(two), two, -1, **dict(kw, delay_step=None, clock_step=None))
    assert img[0, 0, :3].tolist() == [255, 0, 255]                   # ... the lattice over the tint
    img, _ = overlay(_black(two), two, -1, outlines=True, outline_rgba=(255, 255, 255, 255), **kw)
    assert img[0, 0, :3].tolist() == [255, 255, 0] and img[0, 1, :3].tolist() == [255, 255, 255]      # the outline (pixel 1) over everything
    # a half-weight outline over an opaque clock line: (255 * 128 + 0 + 127) // 255 = 128, (255 * 128 + 255 * 127 + 127) // 255 = 255
    edge = _records([[0, 1]], clock=[[0.0, 0.0]])
    img, _ = overlay(np.array([[[0, 255, 255, 1], [0, 0, 0, 1]]], np.uint8), edge, -1, outlines=True, outline_rgba=(255, 255, 255, 128))
    assert img[0, 0].tolist() == [128, 255, 255, 1]


def test_applying_it_twice_blends_twice():
    ev = _records([[0, 1]])
    once, _ = overlay(np.zeros((1, 2, 4), np.uint8), ev, -1, outlines=True, outline_rgba=(255, 255, 255, 128))
    twice, changed = overlay(once, ev, -1, outlines=True, outline_rgba=(255, 255, 255, 128))
    assert once[0, 0, 0] == 128 and twice[0, 0, 0] == 192 and changed == 1      # (255 * 128 + 128 * 127 + 127) // 255 = 192


def test_a_bad_description_is_refused():
    ev = _records([[0, 1]])
    img = _black(ev)
    with pytest.raises(TypeError):
        overlay_settings(outline=True)
    for kw in (dict(delay_step=0.0), dict(delay_step=-1.0), dict(clock_step=INF), dict(clock_step=NAN), dict(lattice_step=(0.0, 0.0, 0.0)),
               dict(lattice_step=(1.0, -2.0, 0.0)), dict(tint=True, tint_t_max=-1.0), dict(outlines=True, outline_rgba=(1, 2, 3)),
               dict(tint=True, tint_alpha=256)):
        with pytest.raises(ValueError):
            overlay(img, ev, -1, **kw)
    assert overlay_settings()["layers"] == 0 and overlay_settings(lattice_step=0.5)["lattice_step"] == (0.5, 0.5, 0.5)
    assert overlay_settings(outlines=True, delay_step=1, clock_step=1, lattice_step=1, tint=True)["layers"] == 31
    out, changed = overlay(img, ev, -1)
    assert np.array_equal(out, img) and changed == 0                 # no layer: no change


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("overlay"))


@pytest.mark.parametrize("name", ["rulers", "ladder_paradox"])
def test_the_tint_is_delay_map_within_one_lsb(lib, name):
    """float32 (the pass) against float64 (delay_map): at most 1 LSB per channel on the CPU event frames, every hit pixel tinted."""
    scene = eo.load_scene(name, "rest", -1)
    ev = oc.cpu_events(lib, scene, 128, 72, "pinhole")
    hit = ev["object"] >= 0
    img, changed = overlay(np.zeros((72, 128, 4), np.uint8), ev, -1, tint=True, tint_alpha=255)
    want = delay_map(ev, -1, band=0.0)
    diff = np.abs(img[..., :3].astype(int) - want.astype(int))
    print(f"{name}: {int((diff > 0).any(-1).sum())} of {int(hit.sum())} hit pixels differ from delay_map, by at most {int(diff.max())} LSB")
    assert diff.max() <= 1
    assert changed == hit.sum() and (img[~hit] == 0).all()


@pytest.mark.parametrize("size", oc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", oc.CAMERAS)
@pytest.mark.parametrize("name", oc.SCENES)
def test_the_layers_of_the_gpu_tests_are_not_vacuous(lib, name, camera, size):
    """Every line layer tests/test_gpu_overlay.py switches on marks more than 1 % and fewer than 50 % of the scene's hit pixels on the CPU
    event frame — a step so coarse that nothing is drawn, or so fine that everything is, would test nothing.  The tint has no such
    band: by its rule it colours every hit pixel, which is what is asserted for it."""
    W, H = size
    scene = eo.load_scene(name, "rest", -1)
    ev = oc.cpu_events(lib, scene, W, H, camera)
    hit = ev["object"] >= 0
    assert hit.sum() > 300 and (~hit).sum() > 300
    base = np.full((H, W, 4), 7, dtype=np.uint8)
    for layer, kw in oc.layer_settings(name).items():
        img, changed = overlay(base, ev, -1, **kw)
        on = oc.marked(base, img)
        assert changed == on.sum()
        share = float((on & hit).sum()) / float(hit.sum())
        print(f"{name} {camera} {W}x{H} {layer}: {share:.3f} of the hit pixels")
        if layer in ("tint", "all"):
            assert (on[hit]).all()
        else:
            assert 0.01 < share < 0.5, (layer, share)
        if layer != "outlines" and layer != "all":
            assert not on[~hit].any()                                # only outlines may touch a miss pixel
