"""The statement of getskewness and the tolerances of its paths (helpers of
tests/test_skewness_host.py and tests/test_gpu_skewness.py; not a test module).

The rule, StatsBase.skewness as remembered (neither Julia nor StatsBase is on
the machines this suite runs on), for every (channel, IF) row v of the window
over its n selected spectra:

    m   = mean(v)          Float32: Base.sum(v) / n, getkurtosis' pairwise sum
    z   = v[i] - m         Float32
    z2  = z * z            Float32
    cm2 += z2              Float64 accumulator, in index order
    cm3 += z2 * z          Float32 product, Float64 accumulator, in index order
    skewness = (cm3 / n) / sqrt((cm2/n) * (cm2/n) * (cm2/n))      Float64

A signed sum has no relative bound on itself, so every bound is scaled by the
absolute third moment as the recipe forms it,

    A = (sum |fl(z2 * z)| / n) / (cm2/n)^1.5  >=  |skewness|.

With u = 2^-24 (Float32) and e = 2^-53 (Float64):

  regs     the recipe in its own order: the same bits.
  mid, twopass
           the recipe's terms added in another order: |d cm3| <= (nt - 1) e A3
           and cm2 within (nt - 1) e relative, so |d s| <= 2.5 nt e A; held at
           3 nt e A (the half covers the final sqrt and division).
  leaf     z, z^2 and z^3 exact in Float64 where the recipe rounds z, z2 and
           z2 * z to Float32: a cube term moves by at most 5u (3u from z, 1u
           per product), a square term by 3u, so |d s| <= (5 + 1.5 * 3) u A =
           9.5 u A; held at 9.5 u 1.05 A (5% for second-order terms, as
           KURT_LEAF_TOL).
NaN and +-Inf positions (and the infinities' signs) equal the statement's on
every path.
"""
from __future__ import annotations

import numpy as np

from conftest import same_bits

U32 = 2.0 ** -24
E64 = 2.0 ** -53
SKEW_LEAF_TOL = 9.5 * U32 * 1.05


def skew_sum_tol(nt: int) -> float:
    return 3.0 * max(int(nt), 1) * E64


def _seq_sum(x: np.ndarray) -> np.ndarray:
    """Float64 sum of each row in index order (np.add.accumulate is a
    sequential loop; ndarray.sum is pairwise)."""
    if x.shape[1] == 0:
        return np.zeros(x.shape[0], dtype=np.float64)
    return np.add.accumulate(x.astype(np.float64), axis=1)[:, -1]


def skew_statement(orc, a, win=None):
    """(skewness, A) of every (channel, IF) row of the window, both (nc, ni)
    float64: the rule above with oracle.mean_f32 as m."""
    a = np.asfortranarray(np.asarray(a, dtype=np.float32))
    w = orc.np_window(a, win)
    nc, ni, nt = w.shape
    rows = w.reshape((nc * ni, nt), order="F")
    if nt == 0:
        nan = np.full((nc, ni), np.nan)
        return nan, nan.copy()
    m = orc.mean_f32(a, win).reshape(nc * ni, order="F")[:, None]
    with np.errstate(all="ignore"):
        z = (rows - m).astype(np.float32)
        z2 = (z * z).astype(np.float32)
        z3 = (z2 * z).astype(np.float32)
        cm2 = _seq_sum(z2) / nt
        cm3 = _seq_sum(z3) / nt
        den = np.sqrt(cm2 * cm2 * cm2)
        s = cm3 / den
        A = (_seq_sum(np.abs(z3)) / nt) / den
    return s.reshape((nc, ni), order="F"), A.reshape((nc, ni), order="F")


def block_win(shape, win, M, b):
    w = list(win) if win is not None else [0, shape[0], 1, 0, shape[1], 1, 0, shape[2], 1]
    w[6] += b * M * w[8]
    w[7] = M
    return w


def skew_statement_blocks(orc, a, win, M):
    """(skewness, A), both (nc, ni, nt / M): the statement of every block alone."""
    nt = orc.window_shape(a.shape, win)[2]
    assert nt % M == 0
    r = [skew_statement(orc, a, block_win(a.shape, win, M, b)) for b in range(nt // M)]
    return np.stack([x[0] for x in r], axis=2), np.stack([x[1] for x in r], axis=2)


def assert_positions(got, want, msg="") -> None:
    """NaN positions, and the positions and signs of the infinities."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, "NaN positions")
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf), (msg, "Inf positions")
    assert np.array_equal(got[inf], want[inf]), (msg, "Inf signs")


def assert_skewness(got, want, A, path: str, nt: int, msg="") -> None:
    """GPU skewness against the statement at the tolerance of the path that
    ran ("regs" the same bits, "mid" / "twopass" skew_sum_tol(nt) * A, "leaf"
    SKEW_LEAF_TOL * A); non-finite positions equal everywhere."""
    got, want, A = (np.asarray(x, np.float64) for x in (got, want, A))
    assert_positions(got, want, msg)
    if path == "regs":
        assert same_bits(got, want), (msg, "bits")
        return
    assert path in ("mid", "twopass", "leaf"), path
    tol = SKEW_LEAF_TOL if path == "leaf" else skew_sum_tol(nt)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    lim = tol * A[fin]
    print(f"skewness {path} nt={nt} {msg}: worst error / bound = "
          f"{float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0:.3g}")
    bad = err > lim
    assert not bad.any(), (msg, path, nt, float(err.max()), float((err / lim)[bad].max()))
