"""numpy reference of the per-face census (include/ts_mesh.h: ts2d_mesh_census_add): integer sums with np.add.at.

A pixel is counted iff 0 <= face_idx < F and (no mask or mask > 0); a counted pixel adds 1 to word 0 of its face's row and, with a target,
q(c) = rint(clip(nan -> 0, 0, 1) * 65536) (float32 product, exact; round to nearest even) per channel to words 1..3."""
from __future__ import annotations

import numpy as np


def q16(c):
    """Q16 fixed point of target values, as int64."""
    c = np.asarray(c, np.float32)
    return np.rint(np.clip(np.nan_to_num(c, nan=0), 0, 1).astype(np.float32) * np.float32(65536)).astype(np.int64)


def counted(face_idx, F, pixel_mask=None):
    """(H, W) bool: the pixels the census counts."""
    fi = np.asarray(face_idx, np.int64)
    ok = (fi >= 0) & (fi < F)
    if pixel_mask is not None:
        ok &= np.asarray(pixel_mask, np.float32).reshape(fi.shape) > 0  # a NaN mask value is not > 0
    return ok


def census_add(acc, face_idx, target=None, pixel_mask=None):
    """Adds one view to `acc` ((F, 4) int64 {pixels, sum_r, sum_g, sum_b}) in place and returns it."""
    assert acc.dtype == np.int64 and acc.ndim == 2 and acc.shape[1] == 4
    ok = counted(face_idx, acc.shape[0], pixel_mask)
    f = np.asarray(face_idx, np.int64)[ok]
    np.add.at(acc[:, 0], f, 1)
    if target is not None:
        q = q16(target)
        for c in range(3):
            np.add.at(acc[:, 1 + c], f, q[c][ok])
    return acc


def census(F, face_idx, target=None, pixel_mask=None):
    return census_add(np.zeros((F, 4), np.int64), face_idx, target, pixel_mask)


def mean_color(acc, fallback):
    """float32(float64(sum) / (float64(pixels) * 65536)) where pixels > 0, else the fallback row."""
    n = acc[:, :1].astype(np.float64)
    with np.errstate(all="ignore"):
        mean = (acc[:, 1:].astype(np.float64) / (n * 65536.0)).astype(np.float32)
    return np.where(n > 0, mean, np.asarray(fallback, np.float32))
