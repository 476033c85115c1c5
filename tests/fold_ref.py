"""NumPy restatement of the fold / unfold rule (include/bldp.h) for one window.

``a`` is the selected (nc, ni, nt) Float32 window; selected channel c has fine
index k = c mod nfpc and coarse index j = c div nfpc; T spectra make a time
block.  In Julia terms the fold is
``dropdims(sum(reshape(A, nfpc, J, ni, T, nto); dims=(2,4)); dims=(2,4))``.
``mask`` is None or anything that broadcasts to the window: a byte of 0 keeps the
sample, any other value drops it (selected, never multiplied)."""
from __future__ import annotations

import numpy as np


def fold_blocks(a, nfpc, T):
    """[j, k, i, t', tt] view of the window (NumPy splits an axis slowest first)."""
    nc, ni, nt = a.shape
    assert nfpc >= 1 and T >= 1 and nc % nfpc == 0 and nt % T == 0
    return a.reshape(nc // nfpc, nfpc, ni, nt // T, T)


def fold_ref(a, nfpc, T=None, mask=None):
    """(sum Float64, kept int64, sum Float32, mean Float32), each (nfpc, ni, nt/T).
    The Float64 sum rounded once is the ``sum``; the Float64 quotient rounded once
    is the ``mean`` (NaN where nothing is kept)."""
    a = np.asarray(a, dtype=np.float32)
    T = max(a.shape[2], 1) if T is None else max(int(T), 1)
    flag = np.zeros(a.shape, bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0,
                                                                        a.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(fold_blocks(flag, nfpc, T), 0, fold_blocks(a, nfpc, T).astype(np.float64))
        s = x.sum(axis=(0, 4))
        kept = (~fold_blocks(flag, nfpc, T)).sum(axis=(0, 4)).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return s, kept, s.astype(np.float32), (s / kept.astype(np.float64)).astype(np.float32)


def fold_abs(a, nfpc, T=None, mask=None):
    """The Float64 sum of |x| over the kept samples of every block (the tolerance's)."""
    a = np.asarray(a, dtype=np.float32)
    keep = np.ones(a.shape, bool) if mask is None else ~np.broadcast_to(np.asarray(mask) != 0,
                                                                         a.shape)
    with np.errstate(invalid="ignore"):
        return fold_ref(np.where(keep, np.abs(a), 0).astype(np.float32), nfpc, T)[0]


def unfold_ref(a, prof, nfpc, T=None, how="divide"):
    """NumPy's Float32 ``/`` or ``-`` of the window and prof[c mod nfpc, i, t div T]."""
    a = np.asarray(a, dtype=np.float32)
    prof = np.asarray(prof, dtype=np.float32)
    nc, ni, nt = a.shape
    T = max(nt, 1) if T is None else max(int(T), 1)
    assert prof.shape == (nfpc, ni, nt // T)
    p = prof[np.arange(nc) % nfpc][:, :, np.arange(nt) // T]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (a / p if how == "divide" else a - p).astype(np.float32)
