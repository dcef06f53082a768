"""The criterion of adaptive anti-aliasing (include/rpt.h, rpt_set_adaptive_aa) in numpy: which pixels of a one-sample frame the
refine pass renders again, and the frame that results.  Host code, no device needed: a user previews what a threshold selects, the
tests state the feature with it —

    adaptive(n, T) = composite(refine_mask(one-sample frame, T), supersampled(n), one-sample frame)
"""
from __future__ import annotations

import numpy as np


def refine_mask(rgb8: np.ndarray, threshold: int) -> np.ndarray:
    """(H, W) bool: True where the largest absolute difference of the pixel's 8-bit R, G, B to those of any of its four neighbours
    (x +- 1, y +- 1; neighbours outside the frame are ignored) is GREATER than `threshold`.  rgb8: (H, W, 3 or 4) uint8 (a fourth
    channel is ignored).  threshold -1 selects every pixel, 255 none."""
    img = np.asarray(rgb8)
    if img.ndim != 3 or img.shape[2] not in (3, 4) or img.dtype != np.uint8:
        raise ValueError(f"refine_mask takes an (H, W, 3 or 4) uint8 image, not {img.dtype} {img.shape}")
    if not -1 <= int(threshold) <= 255:
        raise ValueError("the threshold is -1 (every pixel) .. 255 (none)")
    c = img[:, :, :3].astype(np.int16)
    d = np.zeros(c.shape[:2], dtype=np.int16)
    dx = np.abs(c[:, 1:] - c[:, :-1]).max(axis=2)          # between columns x and x + 1
    dy = np.abs(c[1:] - c[:-1]).max(axis=2)                # between rows y and y + 1
    d[:, 1:] = np.maximum(d[:, 1:], dx)
    d[:, :-1] = np.maximum(d[:, :-1], dx)
    d[1:] = np.maximum(d[1:], dy)
    d[:-1] = np.maximum(d[:-1], dy)
    return d > int(threshold)


def composite(mask: np.ndarray, fine: np.ndarray, coarse: np.ndarray) -> np.ndarray:
    """where(mask, fine, coarse) pixel by pixel: `fine` and `coarse` are frames of the mask's H x W pixels in any layout whose leading
    axes are the mask's (flattened or not) — structured 16-B pixels, (H, W, 3) floats, (H W, 16) bytes."""
    mask = np.asarray(mask, dtype=bool)
    fine, coarse = np.asarray(fine), np.asarray(coarse)
    if fine.shape != coarse.shape or fine.dtype != coarse.dtype:
        raise ValueError("fine and coarse must have the same shape and dtype")
    for m in (mask, mask.reshape(-1)):
        if fine.shape[:m.ndim] == m.shape:
            return np.where(m.reshape(m.shape + (1,) * (fine.ndim - m.ndim)), fine, coarse)
    raise ValueError(f"a frame of shape {fine.shape} does not start with the mask's {mask.shape}")
