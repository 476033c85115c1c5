"""NumPy restatement of the masked reduce's rule (include/bldp.h) for one window.

``a`` is the selected (nc, ni, nt) Float32 window, ``mask`` anything that
broadcasts to it: a byte of 0 keeps the sample, any other value drops it.  For
every F x T block: the Float64 sum of the kept samples (selected, never
multiplied: a flagged NaN or Inf does not reach the sum), the exact count of
kept samples, and the Float32 mean ``np.float32(sum) / np.float32(kept)``."""
from __future__ import annotations

import numpy as np


def masked_blocks(a, F, T):
    """(nco, ni, nto, F*T) view-like array: the samples of every block."""
    nc, ni, nt = a.shape
    F, T = max(int(F), 1), max(int(T), 1)
    assert nc % F == 0 and nt % T == 0
    b = a.reshape(nc // F, F, ni, nt // T, T)          # [co, k, i, to, tt]
    return b.transpose(0, 2, 3, 1, 4).reshape(nc // F, ni, nt // T, F * T)


def masked_ref(a, mask, F=1, T=1):
    """(sum Float64, kept int64, mean Float32) of every block, each (nc/F, ni, nt/T)."""
    a = np.asarray(a, dtype=np.float32)
    flagged = np.broadcast_to(np.asarray(mask) != 0, a.shape)
    x = masked_blocks(a, F, T)
    keep = ~masked_blocks(flagged, F, T)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(keep, x.astype(np.float64), 0.0).sum(axis=-1)   # np.where selects
    kept = keep.sum(axis=-1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = s.astype(np.float32) / kept.astype(np.float32)
    return s, kept, mean
