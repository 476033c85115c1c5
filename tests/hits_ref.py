"""NumPy restatement of the hits rule (include/bldp.h) for one window.

``window`` is the selected (nc, ni, nt) Float32 window (for a band: the vcat of
the banks' windows along the channels), ``mask`` anything that broadcasts to it:
a byte that is not 0 flags the sample.  The flagged samples in Julia's
column-major ``findall`` order: ``total``, their 0-based linear indices
k = c + nc*(i + ni*t) and their values, the lists cut to ``cap``."""
from __future__ import annotations

import numpy as np


def hits_ref(window, mask, cap=None):
    """(total, idx int64, val float32) of the window's flagged samples."""
    window = np.asarray(window, dtype=np.float32)
    wshape = window.shape
    m = np.broadcast_to(np.asarray(mask) != 0, wshape)
    idx = np.flatnonzero(m.reshape(-1, order="F"))
    val = window.reshape(-1, order="F")[idx]
    total = idx.size
    if cap is not None:
        idx, val = idx[:cap], val[:cap]
    return int(total), idx.astype(np.int64), val


def snr_ref(value, median_b, mad_b):
    """(Float64(value) - Float64(median_b)) / Float64(mad_b), element by element."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.asarray(value, np.float32).astype(np.float64)
                - np.asarray(median_b, np.float32).astype(np.float64)) \
            / np.asarray(mad_b, np.float32).astype(np.float64)
