"""The project's "outliers" rule restated in NumPy on top of mad_ref.py (shared
by test_outliers_host.py and test_gpu_outliers.py).  For a block x of n >= 2
Float32 values:

1. c = median(x) (mad_ref.median: BLDP_OP_MEDIAN's bits);
2. d = |x - c|, the difference rounded once to Float32;
3. s = Float32(Float64(median(d)) * MAD_CONSTANT) (BLDP_OP_MAD's bits);
4. thr = Float32(nsigma * Float64(s)), one Float64 product rounded once;
5. sample i is flagged when d_i > thr, a strict Float32 compare;
6. a NaN c or s flags nothing;
7. count = the flagged samples of the block (uint32);
8. mask = the flags (uint8), dense over the window."""
from __future__ import annotations

import numpy as np

from mad_ref import MAD_CONSTANT, blocks, median, window


def outlier_blocks(R, nsigma):
    """Along axis 0 of Float32 blocks: (c, s, thr, d, flags)."""
    assert R.dtype == np.float32
    c = median(R)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(R - c[None])
        assert d.dtype == np.float32
        m = median(d)
        s = (m.astype(np.float64) * MAD_CONSTANT).astype(np.float32)
        thr = (np.float64(nsigma) * s.astype(np.float64)).astype(np.float32)
        flags = d > thr[None]  # (False against a NaN d or thr)
    flags &= ~(np.isnan(c) | np.isnan(s))[None]
    return c, s, thr, d, flags


def outliers_ref(a, n, nsigma, win=None, axis=0):
    """med, mad, count (uint32) and mask (uint8, the window's shape) of every
    block of n values along ``axis`` (0 or 2) of the window of a."""
    a = np.asarray(a)
    assert n >= 2 and axis in (0, 2) and a.dtype == np.float32
    R = blocks(a, n, win, axis)
    c, s, _, _, flags = outlier_blocks(R, nsigma)
    count = flags.sum(axis=0).astype(np.uint32)
    w = window(a, win)
    moved = np.moveaxis(w, axis, 0).shape  # the window with `axis` first
    mask = np.moveaxis(flags.reshape(moved, order="F"), 0, axis).astype(np.uint8)
    back = lambda p: np.asfortranarray(np.moveaxis(p, 0, axis))  # noqa: E731
    return back(c), back(s), back(count), np.asfortranarray(mask)
