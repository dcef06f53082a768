"""Glare without a GPU: the taps of rpt_glare_taps against the float64 Gaussian (rule G1), the refusals of rule G0 as
predicates, glare.apply — exact integers in numpy — against the stage of tests/native/glare_oracle.c word for word, and what the stage
must do whatever the numbers: a single source gives the outer product of the taps, flux is lost to truncation only, no layers is the
identity."""
import math

import numpy as np
import pytest

import glare_cases as gl
from relativitypathtracer_amd import glare


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return gl.build_library(tmp_path_factory.mktemp("glare"), "stars")


@pytest.mark.parametrize("sigma", gl.SIGMAS)
def test_the_taps_are_the_rounded_gaussian_and_sum_to_65536(sigma):
    t, R = glare.taps(sigma)
    assert R == min(32, math.ceil(3.0 * sigma)) and len(t) == 2 * R + 1
    assert int(t.sum()) == 65536
    assert np.array_equal(t, t[::-1])
    j = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-j * j / (2.0 * sigma * sigma))
    ideal = 65536.0 * g / g.sum()
    err = np.abs(t.astype(np.float64) - ideal)
    print(sigma, R, float(np.delete(err, R).max()), float(err[R]))
    assert np.delete(err, R).max() <= 0.5 + 1e-6
    # the centre takes what the 2 R roundings left: each is off by at most 0.5, so the centre by at most R
    assert err[R] <= R + 1e-3


def test_the_setters_refusals_as_predicates():
    ok = [[], [(1.0, 0.5)], [(0.5, 0.5), (0.5, 32.0 / 3.0)], [(1e-3, 1.0), (0.2, 2.0), (0.3, 3.0)]]
    for layers in ok:
        w = glare.weights(layers)
        assert sum(w) == 65536 and all(x >= 0 for x in w) and len(w) == len(layers) + 1
    assert glare.weights([(0.5, 0.5), (0.5, 2.5)])[0] == 0
    bad = [[(0.6, 1.0), (0.5, 1.0)],                     # a negative core
           [(float("nan"), 1.0)], [(0.5, float("nan"))],
           [(0.0, 1.0)], [(-0.1, 1.0)],
           [(0.5, 0.49)], [(0.5, 10.7)],                 # sigma outside [0.5, 32/3]
           [(0.1, 1.0)] * 4]                             # more than RPT_GLARE_LAYERS_MAX layers
    for layers in bad:
        with pytest.raises(ValueError):
            glare.weights(layers)
    for sigma in (0.49, 10.7, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            glare.taps(sigma)


@pytest.mark.parametrize("W,H,wrap", gl.MODEL_SIZES, ids=lambda v: str(v))
def test_apply_equals_the_c_stage(lib, W, H, wrap):
    rng = np.random.default_rng(W * 1000 + H)
    acc = gl.random_accumulator(W, H, rng)
    assert (acc > (1 << 44)).any()
    records = np.zeros((H, W, 8), dtype=np.int32)        # 32 B per pixel, the object first: -1 a miss
    hit = rng.random((H, W)) < 0.3
    hit[0, 0] = True                                     # (the 2^50 word is behind an object)
    records[:, :, 0] = np.where(hit, 3, -1)
    assert (acc[hit] != 0).any() and (acc[~hit] != 0).any()
    for name, layers in gl.LAYER_SETS.items():
        for mask in (None, hit):
            want = gl.oracle_stage(lib, acc, layers, None if mask is None else records, wrap)
            got = glare.apply(acc, layers, hit_mask=mask, wrap=wrap)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (name, mask is not None, int((got != want).sum()))
            assert want.any()
    masked = gl.oracle_stage(lib, acc, gl.LAYER_SETS["three"], records, wrap)
    assert not np.array_equal(masked, gl.oracle_stage(lib, acc, gl.LAYER_SETS["three"], None, wrap))


def test_a_single_word_gives_the_outer_product_of_the_taps():
    W, H, x, y, A = 81, 75, 40, 37, (1 << 40) + 12345
    layers = gl.LAYER_SETS["three"]
    acc = np.zeros((H, W, 3), dtype=np.uint64)
    acc[y, x, 1] = A
    got = glare.apply(acc, layers)
    w = glare.weights(layers)
    want = [[0] * W for _ in range(H)]
    want[y][x] = w[0] * A
    for w_k, (_, sigma) in zip(w[1:], layers):
        t, R = glare.taps(sigma)
        t = [int(v) for v in t]
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                want[y + j][x + i] += w_k * ((t[R + j] * ((t[R + i] * A) >> 16)) >> 16)
    want = np.array([[v >> 16 for v in row] for row in want], dtype=np.uint64)
    assert np.array_equal(got[:, :, 1], want)
    assert not got[:, :, 0].any() and not got[:, :, 2].any()


def test_flux_is_lost_to_truncation_only():
    """Away from the frame's edges the stage moves flux and loses none but what its shifts truncate: each layer at most one unit per word
    of h_k, spread over the 2 R + 1 taps of the column stage as at most one each, one more per word of v_k, and the sum one per word."""
    W, H = 120, 110
    rng = np.random.default_rng(5)
    acc = np.zeros((H, W, 3), dtype=np.uint64)
    inner = gl.random_accumulator(W - 80, H - 80, rng)
    inner = np.minimum(inner, np.uint64(1 << 44))
    acc[40:-40, 40:-40] = inner                          # 40 > R: nothing leaves the frame
    for name, layers in gl.LAYER_SETS.items():
        S = glare.apply(acc, layers)
        total_in, total_out = sum(int(v) for v in acc.reshape(-1)), sum(int(v) for v in S.reshape(-1))
        words = W * H * 3
        # per layer and stage at most one unit per word, each carried on with total weight <= 1; then the last shift
        bound = words * (2 * len(layers) + 1)
        print(name, total_in, total_out, total_in - total_out, bound)
        assert total_in - bound <= total_out <= total_in


def test_no_layers_is_the_identity():
    acc = gl.random_accumulator(33, 17, np.random.default_rng(1))
    for layers in (None, []):
        got = glare.apply(acc, layers)
        assert np.array_equal(got, acc) and got is not acc
