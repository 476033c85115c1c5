"""The planted signed data of tests/reduce_signed_ref.py, checked on the host:
its reference against the oracles, and that it sees the wrong reducers it was
made for.

The wrong reducers, as NumPy models over the F x T blocks, each for the op it
would sit in (the kernels are instantiated per op, so `max` losing an element
says nothing about `sum`):

  max0 / min0   max / min started from 0 instead of -Inf / +Inf
  skip(p)       in-block position p left out
  lastrow       the last spectrum of a time block left out
  swap          blocks 2k and 2k + 1 written to each other's slot

What the planted data sees (asserted below, for a case of every kernel):
max0 in every block of the all-negative set, min0 in every block of the
all-positive set; skip(p) and lastrow in every block through sum and mean on
the all-negative and all-positive sets, and through max (min) in every set in
the blocks whose +P (-P') plant they drop, which over a case's blocks is every
position; swap in every swapped pair through max and min in every set.

What the suite's 0..255 data (synth kind 1) misses at 4098 groups x 1 IF x 16
spectra, F = 1024, T = 16, the largest test_reduce_interleaved_integer_exact
shape (test_old_data_is_blind): max0 and min0 in every block (no value is
negative, and every block holds a 0); skip(p), lastrow and swap in every block
for max and for min (255 and 0 occur about 64 times in each block of 16384, so
no single element, row or block decides them).  Only sum and mean see those
three there.
"""
from __future__ import annotations

import numpy as np
import pytest

import reduce_cases as rc
import reduce_signed_ref as ref


# -- the reference ----------------------------------------------------------------------------

SMALL = [  # (shape, window, F, T, nbank)
    ((8, 1, 4), None, 1, 1, 1),
    ((8, 1, 4), None, 2, 1, 2),
    ((24, 2, 6), None, 3, 2, 1),
    ((64, 1, 8), None, 4, 4, 3),
    ((70, 2, 9), (1, 64, 1, 0, 2, 1, 1, 8, 1), 16, 8, 1),
    ((65, 3, 7), (0, 60, 1, 1, 2, 1, 0, 6, 1), 5, 3, 2),
    ((120, 1, 12), (0, 60, 2, 0, 1, 1, 0, 6, 2), 12, 3, 1),
    ((256, 2, 16), None, 64, 16, 1),
    ((1030, 1, 5), (3, 1024, 1, 0, 1, 1, 0, 4, 1), 512, 2, 2),
    ((2048, 1, 3), None, 1024, 3, 1),
    ((42, 2, 10), (0, 42, 1, 0, 2, 1, 2, 8, 1), 7, 4, 1),
    ((36, 1, 40), None, 6, 8, 2),
]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "%dx%dx%d-F%d-T%d-b%d" % (c[0] + c[2:]))
def test_reference_agrees_with_the_oracles(orc, case):
    shape, window, F, T, nbank = case
    u = ref.planted(shape, window, F, T, nbank, seed=F + T)
    sets = ref.offsets(u, F, T)
    sets["special"] = ref.special(u, shape, window, F, T)
    for name in ref.SETS:
        for op in ref.OPS:
            want = ref.reference(u if name == "special" else sets[name], window, F, T, op,
                                 fix=sets[name] if name == "special" else None)
            for oracle in (orc.reduce, orc.np_reduce):
                got = np.concatenate([oracle(a, F, T, op, window) for a in sets[name]], axis=0)
                assert ref.mismatch(got, want, op, 1) is None, (case, name, op, oracle.__name__)


def test_planted_data_is_what_it_says():
    shape, window, F, T, nbank = (70, 2, 40), (1, 64, 1, 0, 2, 1, 0, 40, 1), 8, 4, 2
    u = ref.planted(shape, window, F, T, nbank, seed=1)
    B, P, C = ref.params(F, T)
    n, per = F * T, 8 * 2 * 10
    assert per * nbank >= n
    seen_plus, seen_minus = set(), set()
    for b in range(nbank):
        R = ref.blocks(u[b], window, F, T)
        assert R.dtype == np.float32 and np.array_equal(R, np.rint(R))
        R2 = R.transpose(0, 3, 1, 2, 4).reshape(n, per, order="F")  # (p, j)
        j = np.arange(per) + b * per
        plus, minus = ref.positions(n, j)
        vp, vm = ref.plant_values(P, j)
        assert np.array_equal(R2.argmax(axis=0), plus) and np.array_equal(R2.max(axis=0), vp)
        assert np.array_equal(R2.argmin(axis=0), minus) and np.array_equal(R2.min(axis=0), -vm)
        assert ((R2 == R2.max(axis=0)).sum(axis=0) == 1).all()  # attained once
        assert ((R2 == R2.min(axis=0)).sum(axis=0) == 1).all()
        rest = np.sort(np.abs(R2), axis=0)[:-2]
        assert rest.max() <= B
        seen_plus |= set(plus.tolist())
        seen_minus |= set(minus.tolist())
    assert seen_plus == seen_minus == set(range(n))
    assert ref.positions(n, 0)[0] == 0 and ref.positions(n, 0)[1] == n - 1
    sets = ref.offsets(u, F, T)
    assert max(a.max() for a in sets["neg"]) < 0 < min(a.min() for a in sets["pos"])
    assert min(a.min() for a in u) < 0 < max(a.max() for a in u)
    for F, T in ((65536, 8), (4096, 128), (1, 1), (12, 8)):
        B, P, C = ref.params(F, T)
        assert C > P + 7 + B and P > B and F * T * (C + P + 7 + B) < 2 ** 24


# -- the wrong reducers -----------------------------------------------------------------------

def flat(a, window, F, T):
    """Blocks as (p, j): position p = f + F t down, block j = co + nco (i + ni to) across."""
    R = ref.blocks(a, window, F, T)
    return R.transpose(0, 3, 1, 2, 4).reshape(F * T, -1, order="F")


def right(R2, op):
    if op in ("sum", "mean"):
        return R2.sum(axis=0, dtype=np.int64)
    return R2.max(axis=0) if op == "max" else R2.min(axis=0)


def without(R2, op, drop):
    """op over each block without the positions where `drop` (n,) is set."""
    ident = {"sum": 0, "mean": 0, "max": -np.inf, "min": np.inf}[op]
    return right(np.where(drop[:, None], np.float32(ident), R2), op)


def skip_all(R2, op):
    """(p, j): op over block j without position p, for every p."""
    if op in ("sum", "mean"):
        return R2.sum(axis=0, dtype=np.int64)[None, :] - R2.astype(np.int64)
    f = np.maximum if op == "max" else np.minimum
    ident = np.float32(-np.inf if op == "max" else np.inf)
    pad = np.full((1, R2.shape[1]), ident, np.float32)
    before = np.concatenate([pad, f.accumulate(R2, axis=0)[:-1]])
    after = np.concatenate([f.accumulate(R2[::-1], axis=0)[::-1][1:], pad])
    return f(before, after)


def swapped(out):
    o = out.copy()
    m = len(o) // 2 * 2
    o[0:m:2], o[1:m:2] = out[1:m:2], out[0:m:2]
    return o


def detections(R2, F, T):
    """{(model, op): bool per block (skip: per (p, block))}: the outputs the wrong reducer changes."""
    n = F * T
    d = {("max0", "max"): np.maximum(right(R2, "max"), 0) != right(R2, "max"),
         ("min0", "min"): np.minimum(right(R2, "min"), 0) != right(R2, "min")}
    last = np.arange(n) >= n - F
    for op in ("sum", "max", "min"):  # (mean: sum's, divided)
        ok = right(R2, op)
        d["skip", op] = skip_all(R2, op) != ok[None, :]
        d["lastrow", op] = without(R2, op, last) != ok
        d["swap", op] = swapped(ok) != ok
    return d


def sample_cases():
    """The smallest case of every kernel (k_reduce_rowt: of every G4)."""
    best = {}
    for c in rc.CASES:
        g = rc.group(c)
        size = c.nchan * c.nif * c.ntime * c.nbank
        if c.F * c.T <= 4096 and (g not in best or size < best[g][0]):
            best[g] = (size, c)
    assert set(best) == set(rc.GROUPS)
    return [best[g][1] for g in sorted(best)]


@pytest.mark.parametrize("case", sample_cases(), ids=rc.case_id)
def test_planted_data_sees_the_wrong_reducers(case):
    shape, window, F, T = (case.nchan, case.nif, case.ntime), case.window, case.F, case.T
    n = F * T
    banks = ref.planted(shape, window, F, T, case.nbank, seed=rc.seed_of(case))
    sets = ref.offsets(banks, F, T)
    per = flat(banks[0], window, F, T).shape[1]
    j = np.arange(per * case.nbank)
    plus, minus = ref.positions(n, j)
    pp = np.arange(n)[:, None]
    det = {}
    for name in ("neg", "mixed", "pos"):
        R2 = np.concatenate([flat(a, window, F, T) for a in sets[name]], axis=1)
        det[name] = detections(R2, F, T)
    pairs = np.arange(len(j)) < len(j) // 2 * 2  # the blocks a swap touches
    assert det["neg"]["max0", "max"].all() and det["pos"]["min0", "min"].all()
    for name in ("neg", "pos"):
        assert det[name]["skip", "sum"].all() and det[name]["lastrow", "sum"].all()
    if n > 1:
        for name in ("neg", "mixed", "pos"):
            d = det[name]
            assert d["skip", "max"][pp == plus[None, :]].all()
            assert d["skip", "min"][pp == minus[None, :]].all()
            assert d["lastrow", "max"][plus >= n - F].all()
            assert d["lastrow", "min"][minus >= n - F].all()
            assert d["swap", "max"][pairs].all() and d["swap", "min"][pairs].all()
        if len(j) >= n:  # every position is some block's maximum and some block's minimum
            assert set(plus.tolist()) == set(minus.tolist()) == set(range(n))


def test_old_data_is_blind(orc):
    """The 0..255 data of the GPU suite under the same models (the module's docstring)."""
    nco, ni, nt, F, T = 4098, 1, 16, 1024, 16
    a = orc.synth(nco * F, ni, nt, 1024, nco + F, 1)
    assert a.min() == 0 and a.max() == 255
    R2 = flat(a, None, F, T)
    n = F * T
    assert not (np.maximum(right(R2, "max"), 0) != right(R2, "max")).any()
    assert not (np.minimum(right(R2, "min"), 0) != right(R2, "min")).any()
    last = np.arange(n) >= n - F
    for op in ("max", "min"):
        ok = right(R2, op)
        # skip(p) changes block j only where p holds the one extreme of its kind
        once = (R2 == ok[None, :]).sum(axis=0) == 1
        assert not once.any()
        assert not (without(R2, op, last) != ok).any()
        assert not (swapped(ok) != ok).any()
    ok = right(R2, "sum")
    assert (without(R2, "sum", last) != ok).all() and (swapped(ok) != ok).mean() > 0.99
