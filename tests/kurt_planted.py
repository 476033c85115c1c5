"""Planted rows for the case table of tests/kurt_cases.py, and their statements
(helpers of tests/test_kurt_planted_host.py and tests/test_gpu_kurt_cases.py;
not a test module).

Every (channel, IF, bank) row of a case's window is one of four kinds, by the
channel's index in the window, so that four channels hold each kind:

  c % 4 == 0  power     integrated BL power as tests/test_gpu_kurtosis.py's
                        power_rows draws it: gamma with mean/sigma R of sqrt(2),
                        30, 300, 3000 or 30000 around 1e9 (sqrt(2): 1e8) times a scallop.
                        There one ulp of Julia's Float32 mean moves the result.
  c % 4 == 1  position  a constant level L with a single spike 2 L at one
                        spectrum (in every block, for tblock).  A skipped spike
                        leaves a constant row, whose every moment ratio is NaN;
                        a spike counted twice halves the kurtosis.  Row after row
                        takes the next of positions(): the ends of the window,
                        both sides of every wave boundary of the case's first
                        kernel, of the leaf, tile and time-chunk boundaries of
                        its tree, and of its batch ends; for blocks the same
                        within a block.  Windows of more than one tree block
                        (> 2048 spectra), which have few rows, start the list
                        at the first leaf's end, a time chunk's start, the
                        root's split and the last block's start.
  c % 4 == 2  negated   minus the power row two channels below (same IF and
                        bank): the kurtosis is that row's, the skewness flips.
  c % 4 == 3  ulp       1e9 plus a few ulps, or a second power row.

R, L, the spike's place and the draws differ by channel, IF and bank, so a row
read in another row's place shows (a position row by its mean and variance
only: a lone spike's ratios depend on the count of spectra alone).  Windows of fewer than four channels rotate
the kinds with the (IF, bank) row.  Everything of the array outside the window
is NaN: reading it poisons the row.

L < 2000 and the spike L above it keep z^2, z^3 and z^4 normal Float32 numbers;
z of the other spectra is L - m exactly.  statements() asserts that every
expected value is finite.
"""
from __future__ import annotations

import numpy as np

import kurt_cases as kc
from conftest import KURT_LEAF_TOL, kurt_sum_tol
from moments_ref import VAR_LEAF_TOL, moments_statement, moments_statement_blocks, var_sum_tol
from skewness_ref import (SKEW_LEAF_TOL, block_win, skew_statement, skew_statement_blocks,
                          skew_sum_tol)

POWER, POSITION, NEGATED, ULP = 0, 1, 2, 3
RS = (np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0)
MAX_POSITIONS = 96


# ---- Julia's pairwise-sum tree, restated from kurtosis.hip -------------------
def pw_level(n: int) -> int:
    K = 0
    while ((n + (1 << K) - 1) >> K) > 2048:
        K += 1
    return K


def pw_node(n: int, L: int, j: int):
    lo, ln = 0, n
    for l in range(L - 1, -1, -1):
        left = (ln + 1) >> 1
        if (j >> l) & 1:
            lo, ln = lo + left, ln - left
        else:
            ln = left
    return lo, ln


def pw_leaf(n: int, K: int, slot: int):
    lo, ln = pw_node(n, K, slot >> 1)
    if ln > 1024:
        left = (ln + 1) >> 1
        return (lo + left, ln - left) if slot & 1 else (lo, left)
    return (lo + ln, 0) if slot & 1 else (lo, ln)


def _cdiv(a, b):
    return -(-a // b)


def _span(lo, ln, sym):
    """Spectra of one leaf (or block, or short window) [lo, lo + ln) a kernel can
    get wrong: its ends, and both sides of the boundaries its first kernel splits
    it at."""
    p = [lo, lo + ln - 1, lo + 1, lo + ln - 2]
    name = kc.kernel(sym)
    args = sym[sym.index("<") + 1:-1].split(",") if "<" in sym else []
    if name in ("k_kurt_regs", "k_kurtb_regs"):
        p += list(range(lo, lo + ln))  # (<= 32: every spectrum)
    elif name == "k_kurt_mid":
        p += [lo + ((w * ln) >> 2) - d for w in (1, 2, 3) for d in (1, 0)]
    elif name == "k_kurt_mid2":
        nw = int(args[1])
        p += [lo + (w * ln) // nw - d for w in range(1, nw) for d in (1, 0)]
    elif name in ("k_kurt_leaf", "k_kurtb_stream"):
        B = int(args[1])  # the first spectrum, then batches of B and a tail
        nb = (ln - 1) // B
        p += [lo + B, lo + B + 1, lo + 1 + nb * B - 1, lo + 1 + nb * B]
    elif name == "k_kurt_tile":
        Q = int(args[0])
        for w in (1, 2, 15):  # waves, and the lane groups' pieces of the first wave
            p += [lo + (w * ln) // 16 - 1, lo + (w * ln) // 16]
        cnt = ln // 16
        p += [lo + cnt // Q - 1, lo + cnt // Q]
    elif name == "k_kurt_leafsum":
        p += [lo + 8, lo + 9, lo + 1 + ((ln - 1) // 8) * 8 - 1, lo + 1 + ((ln - 1) // 8) * 8]
    return [t for t in p if lo <= t < lo + ln]


def positions(case) -> list:
    """Spectra (of the window; of a block for tblock) that take a spike, in the
    order the position rows use them."""
    w = kc.window(case)
    nc, ni, nt = w[1], w[4], w[7]
    n = case.tblock if case.tblock else nt
    if n == 0:
        return []
    p = [0, n - 1, 1, n - 2]
    front = []  # long windows have few rows: their first position rows take boundaries
    if n <= 1024 or kc.path(case) in ("regs", "mid"):
        p += _span(0, n, case.first)
    else:
        K = pw_level(n)
        nslot = 2 << K
        for s in (0, 1, 2, 3, nslot // 2 - 1, nslot // 2, nslot - 2, nslot - 1):
            lo, ln = pw_leaf(n, K, s)
            if ln > 0:
                p += _span(lo, ln, case.first)
        for L in range(1, min(K, 4) + 1):  # the tree's upper nodes
            lo, ln = pw_node(n, L, 1)
            p += [lo - 1, lo]
        if K >= 1:  # the first leaf's end, the root's split, the last block's start
            front += [pw_leaf(n, K, 1)[0] - 1, pw_node(n, 1, 1)[0], pw_node(n, K, (1 << K) - 1)[0],
                      pw_leaf(n, K, 1)[0]]
    if kc.path(case) == "twopass" and not case.tblock:  # plan_kurtosis' time chunks
        ts = 1
        while ts < 4 and n >= 32 * ts:
            ts *= 2
        tiles = _cdiv(_cdiv(nc, 64), 4 // ts) * ni * case.nbank
        nchunk = max(1, min(_cdiv(kc.NUM_CUS * 8, tiles), n // (16 * ts))) if tiles < kc.NUM_CUS * 8 else 1
        rpc = max(1, _cdiv(n, nchunk))
        for j in (1, 2, _cdiv(n, rpc) - 1):
            p += [j * rpc - 1, j * rpc, j * rpc + ts - 1, j * rpc + ts]
        if front and nchunk > 1:
            front.insert(1, rpc)  # the second chunk's first spectrum
    p = front + p
    out = []
    for t in p:
        if 0 <= t < n and t not in out:
            out.append(t)
    return out[:MAX_POSITIONS]


def kind_of(c: int, g: int, nc: int) -> int:
    return (c + (g if nc < 4 else 0)) % 4


def _power(rng, R, c, nt):
    bp = 0.2 + 0.8 * np.sin(np.pi * ((c % 64) + 0.5) / 64) ** 2
    # (R = sqrt(2) around 1e8: a 6 sigma draw around 1e9 has z^4 above Float32's largest)
    top = 1e9 if R >= 30.0 else 1e8
    return rng.gamma(R * R, top / (R * R) * bp, nt).astype(np.float32)


def level_of(c: int, g: int) -> np.float32:
    return np.float32(1000 + 8 * ((c + 5 * g) % 120))


def build(case):
    """(banks, kinds, spikes): the case's banks, (nchan, nif, ntime) Fortran
    float32 arrays; kinds[c, i, b] of the window's rows; spikes[c, i, b] the
    spectrum (of the window, or of every block) of a position row's spike, -1
    elsewhere."""
    w = kc.window(case)
    c0, nc, cs, i0, ni, is_, t0, nt, ts = w
    rng = np.random.default_rng(kc.seed_of(case))
    pos = positions(case)
    M = case.tblock if case.tblock else nt
    nb = nt // M if M else 0
    kinds = np.zeros((nc, ni, case.nbank), np.int8)
    spikes = np.full((nc, ni, case.nbank), -1, np.int64)
    banks = []
    npos = 0
    ulp = np.spacing(np.float32(1e9))
    for b in range(case.nbank):
        a = np.full((case.ntime, case.nif, case.nchan), np.nan, np.float32)  # (C order: rows contiguous)
        for i in range(ni):
            g = i + ni * b
            rows = np.empty((nc, nt), np.float32)
            for c in range(nc):
                k = kind_of(c, g, nc)
                kinds[c, i, b] = k
                if nt == 0:
                    continue
                if k == POWER:
                    rows[c] = _power(rng, RS[(c // 4 + g) % 5], c, nt)
                elif k == POSITION:
                    L = level_of(c, g)
                    rows[c] = L
                    q = pos[npos % len(pos)]
                    npos += 1
                    spikes[c, i, b] = q
                    rows[c, q::M] = 2 * L  # (one spike in the window; one per block for tblock)
                elif k == NEGATED:
                    if c >= 2 and kind_of(c - 2, g, nc) == POWER:
                        rows[c] = -rows[c - 2]
                    else:
                        rows[c] = -_power(rng, RS[(c + g) % 5], c, nt)
                elif (c // 4 + g) % 2 == 0:
                    rows[c] = np.float32(1e9) + ulp * rng.integers(-3, 4, nt).astype(np.float32)
                else:
                    rows[c] = _power(rng, RS[(c // 4 + g + 2) % 5], c, nt)
            if nt:
                a[t0:t0 + nt * ts:ts, i0 + i * is_, c0:c0 + nc * cs:cs] = rows.T
        banks.append(np.asfortranarray(a.transpose(2, 1, 0)))
    assert nb * M == nt
    return banks, kinds, spikes


def planes_of(order: int) -> tuple:
    return {4: ("kurtosis",), 3: ("skewness",), 0: ("mean", "var", "skewness", "kurtosis")}[order]


def statements(orc, case, banks, finite=True) -> list:
    """Per bank the statement's planes of the case's order (and "A" with a
    skewness): (nc, ni) arrays, (nc, ni, nt / tblock) for tblock.  Every value
    is finite (a window of no spectra: every one NaN), which `finite` asserts."""
    win, M = case.window, case.tblock
    out = []
    for a in banks:
        if case.order == 4:
            if M:
                nt = kc.window(case)[7]
                k = np.stack([orc.kurtosis(a, block_win(a.shape, win, M, b)) for b in range(nt // M)],
                             axis=2)
            else:
                k = orc.kurtosis(a, win)
            w = {"kurtosis": k}
        elif case.order == 3:
            s, A = skew_statement_blocks(orc, a, win, M) if M else skew_statement(orc, a, win)
            w = {"skewness": s, "A": A}
        else:
            w = moments_statement_blocks(orc, a, win, M) if M else moments_statement(orc, a, win)
        for name, v in w.items():
            if not finite:
                continue
            if kc.window(case)[7] == 0:
                assert np.isnan(v).all(), (kc.case_id(case), name)
            else:
                assert np.isfinite(v).all(), (kc.case_id(case), name, "not finite")
        out.append(w)
    return out


def class_bound(case, name: str, want: dict) -> np.ndarray:
    """The bound of plane `name` in the case's tolerance class, element by
    element (what conftest.assert_kurtosis, skewness_ref.assert_skewness and
    moments_ref.assert_var allow): 0 where the class is "the same bits"."""
    path = kc.path(case)
    n = case.tblock if case.tblock else kc.window(case)[7]
    v = np.asarray(want[name], np.float64)
    if path == "regs" or name == "mean":
        return np.zeros(v.shape)
    leaf = path == "leaf"
    if name == "kurtosis":
        return (KURT_LEAF_TOL if leaf else kurt_sum_tol(n)) * np.abs(v + 3.0)
    if name == "skewness":
        return (SKEW_LEAF_TOL if leaf else skew_sum_tol(n)) * np.asarray(want["A"], np.float64)
    return (VAR_LEAF_TOL if leaf else var_sum_tol(n)) * np.abs(v)
