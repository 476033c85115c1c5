"""The statement of getmoments and the tolerances of its planes (helpers of
tests/test_moments_host.py and tests/test_gpu_moments.py; not a test module).

For every (channel, IF) row v of the window over its n selected spectra:

    m    = mean(v)                   Float32, Base.sum's pairwise sum / n
    z    = v[i] - m; z2 = z * z      Float32
    cm2 += z2; cm3 += z2 * z; cm4 += z2 * z2   Float32 products, Float64 sums
    mean     = Float64(m)
    var      = cm2 / n               uncorrected: what both StatsBase recipes form
    skewness = (cm3 / n) / sqrt((cm2 / n)^3)
    kurtosis = (cm4 / n) / (cm2 / n)^2 - 3

mean is oracle.mean_f32 widened (the same bits on every path), skewness is
skewness_ref.skew_statement under assert_skewness and kurtosis oracle.kurtosis
under conftest.assert_kurtosis, tolerances unchanged.  var, against NumPy's
cm2 / n of the statement, with u = 2^-24 and e = 2^-53:

  regs     the recipe in its own order: the same bits.
  mid, twopass
           the same non-negative Float64 terms added in another order: each
           order is within (nt - 1) e of the exact sum, relative to it, so the
           two are within nt e of each other (to first order) -- the sum bounds
           itself, no scale is needed.
  leaf     z and z^2 exact in Float64 where the recipe rounds both to Float32:
           a square term moves by at most 3u (2u from z, 1u from the product),
           skewness_ref's bound on a square term, held with its 5%: 3u 1.05.
NaN and +-Inf positions (and the infinities' signs) equal the statement's.
"""
from __future__ import annotations

import numpy as np

from conftest import assert_kurtosis, same_bits
from skewness_ref import (E64, U32, _seq_sum, assert_positions, assert_skewness, block_win,
                          skew_statement)

PLANES = ("mean", "var", "skewness", "kurtosis")
VAR_LEAF_TOL = 3.0 * U32 * 1.05


def var_sum_tol(nt: int) -> float:
    return max(int(nt), 1) * E64


def var_statement(orc, a, win=None):
    """cm2 / n of every (channel, IF) row of the window, (nc, ni) float64."""
    a = np.asfortranarray(np.asarray(a, dtype=np.float32))
    w = orc.np_window(a, win)
    nc, ni, nt = w.shape
    if nt == 0:
        return np.full((nc, ni), np.nan)
    rows = w.reshape((nc * ni, nt), order="F")
    m = orc.mean_f32(a, win).reshape(nc * ni, order="F")[:, None]
    with np.errstate(all="ignore"):
        z = (rows - m).astype(np.float32)
        z2 = (z * z).astype(np.float32)
        v = _seq_sum(z2) / nt
    return v.reshape((nc, ni), order="F")


def moments_statement(orc, a, win=None):
    """dict of the four planes of the statement, each (nc, ni) float64, and "A",
    the scale of skewness_ref's bound."""
    a = np.asfortranarray(np.asarray(a, dtype=np.float32))
    nc, ni, nt = orc.window_shape(a.shape, win)
    if nt == 0:
        nan = np.full((nc, ni), np.nan)
        return {k: nan.copy() for k in PLANES + ("A",)}
    s, A = skew_statement(orc, a, win)
    return {"mean": orc.mean_f32(a, win).astype(np.float64), "var": var_statement(orc, a, win),
            "skewness": s, "A": A, "kurtosis": orc.kurtosis(a, win)}


def moments_statement_blocks(orc, a, win, M):
    """The statement of every block alone: each plane (nc, ni, nt / M)."""
    nt = orc.window_shape(a.shape, win)[2]
    assert nt % M == 0
    r = [moments_statement(orc, a, block_win(a.shape, win, M, b)) for b in range(nt // M)]
    return {k: np.stack([x[k] for x in r], axis=2) for k in r[0]}


def assert_var(got, want, path: str, nt: int, msg="") -> None:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert_positions(got, want, (msg, "var"))
    if path == "regs":
        assert same_bits(got, want), (msg, "var bits")
        return
    assert path in ("mid", "twopass", "leaf"), path
    tol = VAR_LEAF_TOL if path == "leaf" else var_sum_tol(nt)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    lim = tol * np.abs(want[fin])
    print(f"var {path} nt={nt} {msg}: worst error / bound = "
          f"{float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0:.3g}")
    bad = err > lim
    assert not bad.any(), (msg, path, nt, float(err.max()), float((err[bad] / lim[bad]).max()))


def assert_moments(got: dict, want: dict, path: str, nt: int, msg="") -> None:
    """Every plane of `got` (name -> (nc, ni) array, absent or None = not
    asked for) against the statement `want` in the class of `path`."""
    for name in PLANES:
        g = got.get(name)
        if g is None:
            continue
        g = np.asarray(g)
        assert g.dtype == np.float64 and g.shape == want[name].shape, (msg, name, g.shape)
        if name == "mean":
            assert same_bits(g, want["mean"]), (msg, "mean bits")
        elif name == "var":
            assert_var(g, want["var"], path, nt, msg)
        elif name == "skewness":
            assert_skewness(g, want["skewness"], want["A"], path, nt, msg)
        else:
            assert_positions(g, want["kurtosis"], (msg, "kurtosis"))
            assert_kurtosis(g, want["kurtosis"], path, nt, (msg, "kurtosis"))
