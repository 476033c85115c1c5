"""The NumPy restatement of the dedoppler rule (include/bldp.h), for the CPU and
the GPU tests: loops over the drifts and the spectra of a block on whole (nc, ni)
slabs, every add a Float32 add in the order t = 0 .. T-1 from +0.0."""
from __future__ import annotations

import numpy as np


def off(d, t, T):
    """off(d, t): the straight line from 0 to d over T spectra, rounded to the
    nearest channel, halves away from zero; integers only."""
    s = (d > 0) - (d < 0)
    return s * ((2 * abs(d) * t + (T - 1)) // (2 * (T - 1)))


def offsets(D, T):
    """(2D + 1, T) int64: row k is the path of drift k - D."""
    return np.array([[off(d, t, T) for t in range(T)] for d in range(-D, D + 1)], dtype=np.int64)


def scan_order(D):
    """The drifts in the order best / drift scan them."""
    out = [0]
    for m in range(1, D + 1):
        out += [-m, m]
    return out


def key(x):
    """isless order as unsigned order; every NaN the greatest (argext's key)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    k = np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(x), np.uint64(0xFFFFFFFF), k)


def dedoppler_ref(w, D, T, seg=None):
    """(sums (nc, ni, nb, 2D + 1), best (nc, ni, nb), drift (nc, ni, nb) int32) of
    the window ``w`` (nc, ni, nt), Float32."""
    w = np.asarray(w, dtype=np.float32)
    nc, ni, nt = w.shape
    assert T >= 2 and nt % T == 0 and D >= 0
    nb, K = nt // T, 2 * D + 1
    seg = nc if not seg else seg
    tab = offsets(D, T)
    c = np.arange(nc)
    sums = np.zeros((nc, ni, nb, K), dtype=np.float32, order="F")
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(nb):
            for k in range(K):
                acc = np.zeros((nc, ni), dtype=np.float32)
                for t in range(T):
                    src = c + tab[k, t]
                    ok = (src >= 0) & (src < nc)
                    ok &= np.where(ok, src, 0) // seg == c // seg
                    acc[ok] = acc[ok] + w[src[ok], :, b * T + t]   # Float32 + Float32
                sums[:, :, b, k] = acc
    best = sums[..., D].copy(order="F")
    drift = np.zeros((nc, ni, nb), dtype=np.int32, order="F")
    bk = key(best)
    for d in scan_order(D)[1:]:
        v = sums[..., d + D]
        kv = key(v)
        up = kv > bk   # strictly: the first NaN, else the first of the greatest
        best[up], drift[up], bk[up] = v[up], d, kv[up]
    return sums, best, drift


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
