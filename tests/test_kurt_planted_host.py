"""The planted rows of tests/kurt_planted.py do their job, on the statement alone.

For a handful of cases of tests/kurt_cases.py (one per path and block form):
every row kind lies within the first four channels, the position rows take
the window's (or a block's) ends, and three mutants of the window (a planted
spectrum dropped, one counted twice, two adjacent (bank, IF) rows swapped)
move the statement off its unmutated value by more than the bound of the
case's tolerance class, which is what tests/test_gpu_kurt_cases.py allows a
kernel.  No GPU: the statements are the oracle's and NumPy's.
"""
from __future__ import annotations

import numpy as np
import pytest

import kurt_cases as kc
import kurt_planted as kp

SYMS = ("k_kurt_regs<16,false,4>", "k_kurt_regs<32,true,3>", "k_kurt_mid2<32,8,3>",
        "k_kurt_mid<48,0>", "k_kurt_leaf<1,16>", "k_kurt_tile<2,false>", "k_kurt_fold<4>",
        "k_kurtb_regs<32,false,3>", "k_kurtb_stream<4,4,0>", "k_kurtb_scatter")
CASES = [c for c in kc.CASES if c.sym in SYMS]


def moved(name, want, mut, bound, at):
    """Whether plane `name` of the mutant's statement left the class bound at `at`."""
    a, b = want[name][at], mut[name][at]
    nan = np.isnan(a) != np.isnan(b)
    with np.errstate(invalid="ignore"):
        return nan | (np.abs(a - b) > bound[at])


def test_the_handful_is_there():
    assert sorted(c.sym for c in CASES) == sorted(SYMS)


def test_every_case_holds_two_rows_and_every_kind():
    """At least two (bank, IF) rows, and the four row kinds among them."""
    for c in kc.CASES:
        w = kc.window(c)
        if w[7] == 0:  # (the NaN fill of a window of no spectra)
            continue
        groups = w[4] * c.nbank
        kinds = {kp.kind_of(ch, g, w[1]) for ch in range(w[1]) for g in range(groups)}
        assert groups >= 2 and kinds == {0, 1, 2, 3}, kc.case_id(c)


def test_positions_hold_the_ends_and_the_boundaries():
    for c in kc.CASES:
        w = kc.window(c)
        n = c.tblock if c.tblock else w[7]
        if n == 0:
            continue
        p = kp.positions(c)
        assert len(p) == len(set(p)) and all(0 <= t < n for t in p), kc.case_id(c)
        assert {0, n - 1, 1, n - 2} <= set(p) if n >= 4 else p[0] == 0, kc.case_id(c)
        if n <= 2048:
            assert p[:4] == [0, n - 1, 1, n - 2][:len(p)], kc.case_id(c)
        else:  # few rows: the first of them take the tree's boundaries
            K = kp.pw_level(n)
            assert p[0] == kp.pw_leaf(n, K, 1)[0] - 1 and kp.pw_node(n, 1, 1)[0] in p[:3], kc.case_id(c)
        if kc.path(c) == "regs":
            assert sorted(p) == list(range(n)), kc.case_id(c)
        if kc.kernel(c.first) == "k_kurt_mid":
            assert {(n >> 2) - 1, n >> 2, (3 * n >> 2) - 1, 3 * n >> 2} <= set(p), kc.case_id(c)
        if n > 2048:  # the first leaves of the tree, both sides
            lo, ln = kp.pw_leaf(n, kp.pw_level(n), 1)
            assert {lo - 1, lo} <= set(p) and 512 <= ln <= 1024, kc.case_id(c)


@pytest.mark.parametrize("case", CASES, ids=kc.case_id)
def test_mutants_leave_the_class(orc, case):
    banks, kinds, spikes = kp.build(case)
    w = kc.window(case)
    c0, nc, cs, i0, ni, is_, t0, nt, ts = w
    M = case.tblock
    # every kind within four channels of the first row; rows differ by IF and bank
    assert sorted(kinds[:4, 0, 0]) == [0, 1, 2, 3]
    win = [np.asarray(orc.np_window(a, case.window)) for a in banks]
    flat = [x[:, i, :] for x in win for i in range(ni)]
    for u in range(len(flat)):
        for v in range(u + 1, len(flat)):
            assert not (flat[u] == flat[v]).all(axis=1).any(), (u, v)
    n_pos = int((kinds == kp.POSITION).sum())
    assert len(set(spikes[kinds == kp.POSITION])) == min(n_pos, len(kp.positions(case)))
    want = kp.statements(orc, case, banks)
    names = kp.planes_of(case.order)

    def remade(b, edit):
        a = banks[b].copy(order="F")
        edit(a)
        return kp.statements(orc, case, [a], finite=False)[0]  # (a mutant may give NaN)

    # a position row of bank 0: its spike dropped, then counted twice
    c, i = [int(x[0]) for x in np.nonzero(kinds[:, :, 0] == kp.POSITION)]
    q = int(spikes[c, i, 0])
    q2 = q + 1 if q + 1 < (M or nt) else q - 1
    at = (c, i, 0) if M else (c, i)
    cell = (c0 + c * cs, i0 + i * is_)
    L = kp.level_of(c, i)
    assert banks[0][cell + (t0 + q * ts,)] == 2 * L and banks[0][cell + (t0 + q2 * ts,)] == L
    bound = {name: kp.class_bound(case, name, want[0]) for name in names}

    def drop(a):
        a[cell + (t0 + q * ts,)] = L

    def twice(a):
        a[cell + (t0 + q2 * ts,)] = 2 * L

    for edit in (drop, twice):
        mut = remade(0, edit)
        for name in names:
            assert moved(name, want[0], mut, bound[name], at), (edit.__name__, name)
    # two adjacent (bank, IF) rows swapped: IFs 0 and 1 of bank 0
    assert ni >= 2

    def swap(a):
        sl0 = (slice(None), i0, slice(None))
        sl1 = (slice(None), i0 + is_, slice(None))
        t = a[sl0].copy()
        a[sl0] = a[sl1]
        a[sl1] = t

    mut = remade(0, swap)
    # (a lone spike's skewness and kurtosis depend on the count of spectra alone,
    # not on its level or place: a position row tells rows apart by mean and var)
    told = kinds[:, 0, 0] != kp.POSITION
    for name in names:
        for i in (0, 1):
            at = (slice(None), i)
            m = moved(name, want[0], mut, bound[name], at)
            assert (m if name in ("mean", "var") else m[told]).all(), ("swap", name, i)
            assert np.array_equal(mut[name][:, i], want[0][name][:, 1 - i], equal_nan=True)

