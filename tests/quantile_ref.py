"""The project's quantile(p) rule restated in NumPy (shared by
test_quantile_host.py and test_gpu_quantile.py): Statistics.quantile(x, p),
Julia's default definition (type 7, alpha = beta = 1), as include/bldp.h states
it.  For a block x of n >= 2 values and a Float64 p in [0, 1]:

1. v[1..n] = x in isless order (the integer image of the float: -0.0 < 0.0);
2. in Float64, every operation rounded once: m = 1 + p * (1 - 1 - 1),
   aleph = n * p + m, j = clamp(trunc(aleph), 1, n - 1), g = clamp(aleph - j, 0, 1);
3. a = v[j], b = v[j + 1];
4. both finite: d = b - a rounded once in the element type (Float32 for Float32
   data), r = Float64(a) + g * Float64(d);
5. else r = (1 - g) * Float64(a) + g * Float64(b) (0 * Inf = NaN included);
6. the result is r in the element type; 7. a block holding a NaN gives NaN.

Other element types take the same steps in Float64.  NumPy's scalar and array
Float64 arithmetic rounds every operation once (no fused multiply-add)."""
from __future__ import annotations

import numpy as np

from mad_ref import blocks, key, window


def rank_weight(n, p):
    """(j, g): the 1-based lower rank and the weight of the next."""
    p = np.float64(p)
    m = np.float64(1.0) + p * (np.float64(1.0) - np.float64(1.0) - np.float64(1.0))
    aleph = np.float64(n) * p + m
    j = int(min(max(np.trunc(aleph), 1.0), float(n - 1)))
    g = float(min(max(aleph - np.float64(j), np.float64(0.0)), np.float64(1.0)))
    return j, g


def neighbours(R, p):
    """(a, b, g) along axis 0 of blocks R: the two order statistics and the weight."""
    j, g = rank_weight(R.shape[0], p)
    S = np.take_along_axis(R, np.argsort(key(R), axis=0, kind="stable"), axis=0)
    return S[j - 1], S[j], g


def quantile_blocks(R, p):
    """Along axis 0: Float32 of Float32 blocks, Float64 of Float64 ones."""
    a, b, g = neighbours(R, p)
    g = np.float64(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a  # rounded once, in the element type
        assert d.dtype == R.dtype
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        lerp = a64 + g * d.astype(np.float64)
        mix = (np.float64(1.0) - g) * a64 + g * b64
        r = np.where(np.isfinite(a) & np.isfinite(b), lerp, mix).astype(R.dtype)
    return np.where(np.isnan(R).any(axis=0), R.dtype.type(np.nan), r)


def quantile_ref(a, n, p, win=None, axis=0):
    """fqavfunc (axis 0) or tavfunc (axis 2) quantile(p) of every n values:
    Float32 data in Float32, anything else in Float64; n <= 1 is the window."""
    a = np.asarray(a)
    if n <= 1:
        return np.asfortranarray(window(a, win))
    R = blocks(a, n, win, axis)
    if R.dtype != np.float32:
        R = R.astype(np.float64)
    return np.asfortranarray(np.moveaxis(quantile_blocks(R, p), 0, axis))
