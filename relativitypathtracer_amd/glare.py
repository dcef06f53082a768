"""Glare for the point-source passes (Renderer.set_glare, rpt_set_glare) on the host: the integer taps of a layer as the
library computes them, the stage itself in exact integers — the user's preview of what a layer set does to an accumulator, and the
model the tests hold the kernels' C restatement to — and one or two named layer sets.

A layer is (weight, sigma): a separable Gaussian of sigma pixels that carries `weight` of a source's flux; what the layers leave, the
core, stays in the source's own pixel.  The stage is linear and the same for every source, so a brighter source looks bigger only
because more of its tail clears the display's floor."""
import ctypes as C
import math

import numpy as np

from . import _ffi

LAYERS_MAX = 3
RADIUS_MAX = 32
SOURCE_MAX = 1 << 44            # rule G2: a word of the accumulator enters the stage as min(word, 2^44)
SIGMA_MIN, SIGMA_MAX = 0.5, 32.0 / 3.0

# Chosen by eye on the shipped scenes at 1280 x 720, not derived from any optics: "soft" is a tight halo that makes the magnitudes of a
# star field readable; "lens" adds a wide, faint skirt that only the brightest sources lift above the display's floor.
PRESETS = {"soft": [(0.30, 1.2)],
           "lens": [(0.30, 1.2), (0.12, 4.0), (0.04, 32.0 / 3.0)]}


def preset(name):
    """One of the named layer sets ("soft", "lens") as a list of (weight, sigma) for Renderer.set_glare.  They are a matter of taste."""
    if name not in PRESETS:
        raise ValueError(f"glare preset {name!r}: there are {sorted(PRESETS)}")
    return list(PRESETS[name])


def taps(sigma):
    """(the 2 R + 1 integer taps of one layer, R) from rpt_glare_taps — host code, no device: R = min(32, ceil(3 sigma)), the taps sum
    to 65536.  Always through the library, so that no second exp or rounding can disagree with the kernels' taps."""
    out = (C.c_uint32 * (2 * RADIUS_MAX + 1))()
    radius = C.c_int(0)
    if _ffi.hip().rpt_glare_taps(float(sigma), out, C.byref(radius)) != 0:
        raise ValueError(f"glare: sigma is {sigma!r}, not in [0.5, 32/3]")
    R = radius.value
    return np.array(out[RADIUS_MAX - R:RADIUS_MAX + R + 1], dtype=np.uint64), R


def weights(layers):
    """Rule G0: [w_0, w_1, ...], integers that sum to 65536; ValueError for what rpt_set_glare refuses."""
    layers = list(layers)
    if len(layers) > LAYERS_MAX:
        raise ValueError(f"glare has at most {LAYERS_MAX} layers, {len(layers)} were given")
    w = []
    for weight, sigma in layers:
        if not (weight > 0.0 and weight <= 1.0):
            raise ValueError(f"glare: the weight {weight!r} is not in (0, 1]")
        if not (SIGMA_MIN <= sigma <= SIGMA_MAX):
            raise ValueError(f"glare: sigma is {sigma!r}, not in [0.5, 32/3]")
        w.append(int(math.floor(weight * 65536.0 + 0.5)))
    if sum(w) > 65536:
        raise ValueError("glare: the weights sum to more than 1")
    return [65536 - sum(w)] + w


def _shifted(a, j, axis, wrap):
    """b[.., x, ..] = a[.., x + j, ..] along `axis`: zero outside the frame, or modulo the size with `wrap`."""
    if wrap:
        return np.roll(a, -j, axis=axis)
    n = a.shape[axis]
    out = np.zeros_like(a)
    if abs(j) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(j, 0), n + min(j, 0))
    dst[axis] = slice(max(-j, 0), n - max(j, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def apply(acc, layers, hit_mask=None, wrap=False):
    """Rules G2-G5 on an (H, W, 3) uint64 accumulator (unit 2^-24), in exact integers: the (H, W, 3) uint64 sums S the resolve
    tonemaps.  hit_mask: (H, W) bool, the star pass's rule — a masked pixel is no source.  wrap: columns are taken modulo the width (a
    full-circle panorama); rows never wrap.  No layers: the accumulator as it is.  Every intermediate is at most 2^60."""
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"glare.apply: the accumulator is (H, W, 3), not {a.shape}")
    layers = list(layers or [])
    if not layers:
        return a.copy()
    w = weights(layers)
    a = np.minimum(a, np.uint64(SOURCE_MAX))
    if hit_mask is not None:
        a = np.where(np.asarray(hit_mask, dtype=bool)[:, :, None], np.uint64(0), a)
    total = np.uint64(w[0]) * a
    for w_k, (_, sigma) in zip(w[1:], layers):
        t, R = taps(sigma)
        h = np.zeros_like(a)
        for j in range(-R, R + 1):
            h += t[R + j] * _shifted(a, j, 1, wrap)
        h >>= np.uint64(16)
        v = np.zeros_like(a)
        for j in range(-R, R + 1):
            v += t[R + j] * _shifted(h, j, 0, False)
        v >>= np.uint64(16)
        total += np.uint64(w_k) * v
    return total >> np.uint64(16)
