"""Adaptive anti-aliasing without a GPU: the criterion in numpy (relativitypathtracer_amd/adaptive.py) on hand-made images, the oracle
composite that the GPU test expects (and that each of its cases refines some pixels and leaves some), the reference with the sample
loop against the oracle's own msaa argument, and the calls' argument validation."""
import ctypes as C

import numpy as np
import pytest

import aa_support
import oracle_ffi
from conftest import CONFIGS, load_config
from relativitypathtracer_amd import _ffi
from relativitypathtracer_amd.adaptive import composite, refine_mask

RPT_ERR_ARG = 1


def test_a_single_bright_pixel_marks_itself_and_its_four_neighbours():
    img = np.full((7, 9, 3), 10, np.uint8)
    img[3, 4] = (10, 200, 10)
    want = np.zeros((7, 9), bool)
    for y, x in ((3, 4), (2, 4), (4, 4), (3, 3), (3, 5)):
        want[y, x] = True
    assert np.array_equal(refine_mask(img, 8), want)
    assert np.array_equal(refine_mask(img, 189), want)          # |200 - 10| = 190 > 189
    assert not refine_mask(img, 190).any()                      # "greater than", not "at least"
    rgba = np.concatenate([img, np.random.default_rng(0).integers(0, 255, (7, 9, 1), dtype=np.uint8)], -1)
    assert np.array_equal(refine_mask(rgba, 8), want)           # the fourth byte is not a colour


def test_frame_borders():
    img = np.zeros((4, 5, 3), np.uint8)
    img[0, 0] = (0, 0, 255)
    img[3, 4] = (255, 0, 0)
    want = np.zeros((4, 5), bool)
    for y, x in ((0, 0), (0, 1), (1, 0), (3, 4), (3, 3), (2, 4)):
        want[y, x] = True
    assert np.array_equal(refine_mask(img, 0), want)            # nothing wraps round
    one = np.full((1, 1, 3), 77, np.uint8)
    assert refine_mask(one, -1).all() and not refine_mask(one, 0).any()
    row = np.array([[[0, 0, 0], [9, 0, 0], [9, 0, 0]]], np.uint8)
    assert refine_mask(row, 8).tolist() == [[True, True, False]]
    assert refine_mask(row.transpose(1, 0, 2), 8).tolist() == [[True], [True], [False]]


def test_thresholds_all_none_and_monotone():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (33, 47, 3), dtype=np.uint8)
    flat = np.full((5, 6, 3), 128, np.uint8)
    assert refine_mask(img, -1).all() and refine_mask(flat, -1).all()
    assert not refine_mask(img, 255).any()
    assert not refine_mask(flat, 0).any()
    last = refine_mask(img, -1)
    for t in range(0, 256):
        m = refine_mask(img, t)
        assert not (m & ~last).any(), t                         # a larger threshold never adds a pixel
        last = m
    with pytest.raises(ValueError):
        refine_mask(img, 256)
    with pytest.raises(ValueError):
        refine_mask(img.astype(np.float32), 8)


def test_composite_layouts():
    mask = np.array([[True, False, False], [False, True, True]])
    fine = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    coarse = -fine
    got = composite(mask, fine, coarse)
    assert np.array_equal(got[mask], fine[mask]) and np.array_equal(got[~mask], coarse[~mask])
    pf = np.zeros(6, dtype=oracle_ffi.PIXEL_DTYPE)
    pc = np.zeros(6, dtype=oracle_ffi.PIXEL_DTYPE)
    pf["x"], pc["x"] = 1, 2
    assert composite(mask, pf, pc)["x"].tolist() == [1, 2, 2, 2, 1, 1]
    with pytest.raises(ValueError):
        composite(mask, fine, coarse[:1])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_compared_case_refines_some_pixels_and_leaves_some(name):
    """What tests/test_gpu_adaptive_aa.py compares the plain pinhole with: where(mask_T(oracle(1)), oracle(msaa = n), oracle(1)).  Every
    case with 0 <= T < 255 must refine at least one pixel and leave at least one, or it would prove nothing."""
    W, H = aa_support.PLAIN_SIZE
    scene = load_config(name)
    px1, rgb1, _ = oracle_ffi.render(scene, W, H)
    for n in aa_support.PLAIN_NS:
        pxn, rgbn, _ = oracle_ffi.render(scene, W, H, msaa=n)
        for T in aa_support.PLAIN_THRESHOLDS:
            mask = refine_mask(aa_support.rgb8_of(px1, W, H), T)
            if 0 <= T < 255:
                assert 0 < mask.sum() < W * H, (name, n, T, int(mask.sum()))
            want = composite(mask, pxn, px1)
            assert np.array_equal(want[mask.reshape(-1)], pxn[mask.reshape(-1)]) and np.array_equal(want[~mask.reshape(-1)], px1[~mask.reshape(-1)])
        assert not np.array_equal(pxn["rgba"], px1["rgba"]), (name, n)      # supersampling changes the picture


@pytest.fixture(scope="module")
def aa_oracle(tmp_path_factory):
    return aa_support.build_oracle(tmp_path_factory.mktemp("aa"))


@pytest.mark.parametrize("name", ["shadows", "arch", "cubes"])
def test_the_sample_loop_reference_is_the_oracles_msaa(aa_oracle, name):
    """tests/native/aa_oracle.c with the pinhole's sample directions is the oracle's own msaa frame, bit for bit."""
    W, H = 96, 54
    scene = load_config(name)
    for n in (1, 2, 3):
        px, rgb, hits = aa_support.oracle_supersampled(aa_oracle, scene, W, H, n, aa_support.lens_sample_dirs(W, H, n))
        assert hits.max() <= n * n and 0 < (hits > 0).sum() < W * H
        opx, orgb, _ = oracle_ffi.render(scene, W, H, msaa=n)
        assert np.array_equal(px.view(np.uint8), opx.view(np.uint8)), (name, n)
        assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32)), (name, n)


def test_panorama_sample_directions_are_the_finer_panoramas_pixels():
    W, H, n = 12, 6, 3
    d = aa_support.pano_sample_dirs(W, H, n, h_fov=2.0, v_fov=1.2, yaw=0.3).reshape(H, W, n, n, 3)
    d1 = aa_support.pano_sample_dirs(n * W, n * H, 1, h_fov=2.0, v_fov=1.2, yaw=0.3).reshape(n * H, n * W, 3)
    for (y, x, sy, sx) in ((0, 0, 0, 0), (5, 11, 2, 2), (2, 7, 1, 2), (3, 0, 2, 0)):
        assert np.array_equal(d[y, x, sy, sx], d1[n * y + sy, n * x + sx])


def test_argument_validation_needs_no_device():
    h = _ffi.hip()
    n = C.c_uint64(7)
    assert h.rpt_set_adaptive_aa(None, 2, 8) == RPT_ERR_ARG
    assert h.rpt_last_aa_refined(None, C.byref(n)) == RPT_ERR_ARG and n.value == 7
    assert h.rpt_last_aa_variant(None) == RPT_ERR_ARG
