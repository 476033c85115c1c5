"""The project's "mad" rule restated in NumPy (shared by test_mad_host.py and
test_gpu_mad.py).  For a block x of n >= 2 values of element type Float32:

1. c = median(x): isless order (the integer image of the float: -0.0 < 0.0),
   the middle element of an odd block, a/2 + b/2 in Float32 (two roundings) of
   an even one, NaN when the block holds a NaN;
2. d = |x - c|, the difference rounded once to Float32;
3. m = median(d) by the same rule (NaN wins: a NaN c, or Inf - Inf);
4. result = Float32(Float64(m) * MAD_CONSTANT).

Other element types take the same steps in Float64 and the result is the
Float64 product.  The constant is StatsBase's mad_constant
(1 / quantile(Normal(), 3/4)) as the issue states it."""
from __future__ import annotations

import numpy as np

MAD_CONSTANT = 1.4826022185056018


def window(a, win):
    if win is None:
        return a
    return a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1]) for k in range(3)])]


def blocks(a, n, win=None, axis=0):
    """(n, blocks along `axis`, the other axes...) of the window of a."""
    w = np.moveaxis(np.asarray(window(a, win)), axis, 0)
    assert w.shape[0] % n == 0
    return np.asfortranarray(w).reshape((n, w.shape[0] // n) + w.shape[1:], order="F")


def key(x):
    """isless order of the floats as unsigned order (NaN aside)."""
    ut = np.uint32 if x.dtype == np.float32 else np.uint64
    u = np.ascontiguousarray(x).view(ut)
    top = ut(1) << ut(8 * x.dtype.itemsize - 1)
    return np.where(u & top != 0, ~u, u | top)


def median(R):
    """Along axis 0, in R's element type."""
    n, half = R.shape[0], R.dtype.type(0.5)
    S = np.take_along_axis(R, np.argsort(key(R), axis=0, kind="stable"), axis=0)
    with np.errstate(invalid="ignore"):
        r = S[n // 2] if n % 2 else S[n // 2 - 1] * half + S[n // 2] * half
    assert r.dtype == R.dtype
    return np.where(np.isnan(R).any(axis=0), R.dtype.type(np.nan), r)


def mad_blocks(R):
    """Along axis 0: Float32 of Float32 blocks, Float64 of Float64 ones."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(R - median(R)[None])
    assert d.dtype == R.dtype
    m = median(d)
    with np.errstate(over="ignore"):  # (floatmax * 1.48 is Inf in Float32)
        return (m.astype(np.float64) * MAD_CONSTANT).astype(R.dtype)


def mad_ref(a, n, win=None, axis=0):
    """fqavfunc (axis 0) or tavfunc (axis 2) "mad" of every n values: Float32
    data in Float32, anything else in Float64; n <= 1 is the window itself."""
    a = np.asarray(a)
    if n <= 1:
        return np.asfortranarray(window(a, win))
    R = blocks(a, n, win, axis)
    if R.dtype != np.float32:
        R = R.astype(np.float64)
    return np.asfortranarray(np.moveaxis(mad_blocks(R), 0, axis))


def median_ref(a, n, win=None, axis=0):
    return np.asfortranarray(np.moveaxis(median(blocks(a, n, win, axis)), 0, axis))
