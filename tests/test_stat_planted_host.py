"""CPU: the planted blocks of tests/stat_planted.py are what they claim to be,
the references the GPU module compares against agree with two other statements
of the same rules on them, and the blocks would tell a wrong select.

The generators assert their own claims with the select model (`select_trace`)
when they build a block; here every class is built over a range of block
lengths and ranks, the model's select is held to a plain sort, and
`quantile_ref`, `mad_ref`, `median_ref` and `outliers_ref` are compared bit for
bit with the model's results (histograms, no sort) and with `alt_*` (a sort by
Python struct-packed keys).  Then each wrong select is switched into the MODEL
(never the library): dropping the low byte, taking rank q for q + 1, ordering
-0.0 equal to +0.0, `>=` for `>` in the flag rule, and losing a slot's ranks from
the fifth slot on.  Each must change the bits of some result on some block of
the class aimed at it.
"""
from __future__ import annotations

import numpy as np
import pytest

import stat_cases as sc
import stat_planted as sp
from conftest import same_bits
from mad_ref import mad_ref, median_ref
from outliers_ref import outliers_ref
from quantile_ref import quantile_ref, rank_weight

NS = (2, 3, 4, 5, 8, 17, 33, 64, 65, 100, 257, 1028)
NSIGMAS = (0.0, 5.0, 1e300)


def spread_probs(n, L):
    """L lower ranks spread over a block of n (tools/stat_cases_gen.py's)."""
    return tuple((k * (n - 1) // L + 0.5) / (n - 1) for k in range(L))


def rank_probs(n, q):
    """Probabilities whose lower rank is q: the middle of the pair and its two ends."""
    ps = [(q + 0.5) / (n - 1), q / (n - 1), min((q + 1) / (n - 1), 1.0)]
    assert sp.lower_rank(n, ps[0]) == q
    return tuple(ps)


def planted(n):
    """[(class, q, ps, block)] of every class a block of n allows, for the
    median's ranks, both clamp ends and the ranks of 8 spread probabilities."""
    rng = np.random.default_rng(n)
    out = []
    qs = sorted({(n - 1) // 2, 0, n - 2})
    for q in qs:
        pair = (q, q + 1)
        for name, gen in list(sp.ORDER_CLASSES.items()) + list(sp.RANK_FREE.items()):
            v = gen(n, q, pair, rng)
            if v is not None:
                out.append((name, q, rank_probs(n, q), rng.permutation(v)))
    if n >= 9:
        ps = spread_probs(n, 8)
        ranks = sp.rank_set(n, ps)
        for name, gen in sp.SLOT_CLASSES.items():
            v = gen(n, ranks[0], ranks, rng)
            if v is not None:
                out.append((name, ranks[0], ps, rng.permutation(v)))
    return out


@pytest.fixture(scope="module")
def blocks():
    return {n: planted(n) for n in NS}


def test_every_class_is_built_and_holds_its_claim(blocks):
    """(the claims are the generators' own assertions: building is the test)"""
    seen = {}
    for n, rows in blocks.items():
        for name, q, ps, v in rows:
            assert v.dtype == np.float32 and v.shape == (n,), (name, n)
            seen.setdefault(name, set()).add(n)
    assert set(seen) == set(sp.ORDER_CLASSES) | set(sp.RANK_FREE) | set(sp.SLOT_CLASSES)
    # what needs a minimum n is skipped below it, and only there
    assert seen["all256"] == {n for n in NS if n >= 256}
    assert seen["slots_five"] == seen["slots_all"] == {n for n in NS if n >= 9}
    assert min(seen["tie_last_finite"]) <= 5 and seen["split3_ulp"] == set(NS)
    assert seen["many_digits"] == {n for n in NS if n >= 3}
    # sixteen ranks need 17 values
    assert len(sp.rank_set(17, spread_probs(17, 8))) == 16 > len(sp.rank_set(16, spread_probs(16, 8)))


def test_the_select_model_is_a_select(blocks):
    for n, rows in blocks.items():
        for name, q, ps, v in rows:
            keys = sp.f2key(v)
            ranks = sp.rank_set(n, ps)
            tr = sp.select_trace(keys, ranks)
            srt = np.sort(keys)
            assert list(tr.key) == srt[list(ranks)].tolist(), (name, n)
            for r, k, selc, tie in zip(ranks, tr.key, tr.selc, tr.tie):
                first = int(np.searchsorted(srt, k, side="left"))
                assert selc == int((srt == k).sum()) and tie == r - first, (name, n, r)
            assert tr.slots[0] == 1 and all(1 <= s <= len(ranks) for s in tr.slots)
            for k in range(4):  # the prefixes are the keys' leading bytes
                assert [p >> (24 - 8 * k) for p in tr.prefix[k]] == \
                    [kk >> (24 - 8 * k) for kk in tr.key]
    assert sp.key2f(sp.f2key(np.float32([-0.0, 0.0, -np.inf, 1e-45]))).tobytes() == \
        np.float32([-0.0, 0.0, -np.inf, 1e-45]).tobytes()


def results(v, ps, wrong=None):
    """Every result of a block from the model, as raw bits."""
    n = v.size
    out = {"median": sp.model_median(v, wrong), "mad": sp.model_mad(v, wrong)}
    for p in ps:
        out["quantile %r" % p] = sp.model_quantile(v, p, wrong)
    out["quantiles"] = sp.model_quantiles(v, ps, wrong)
    for ns in NSIGMAS:
        c, s, cnt, f = sp.model_outliers(v, ns, wrong)
        out["outliers %g" % ns] = np.concatenate([np.float32([c, s]).view(np.uint32), [cnt], f])
    return {k: np.asarray(x).tobytes() for k, x in out.items()}


def test_the_references_agree_with_two_other_statements(blocks):
    for n, rows in blocks.items():
        for name, q, ps, v in rows:
            a = np.asfortranarray(v.reshape(n, 1, 1))
            msg = (name, n, q)
            med, mad = median_ref(a, n)[0, 0, 0], mad_ref(a, n)[0, 0, 0]
            assert same_bits(med, sp.model_median(v)) and same_bits(med, sp.alt_median(v)), msg
            assert same_bits(mad, sp.model_mad(v)) and same_bits(mad, sp.alt_mad(v)), msg
            planes = sp.model_quantiles(v, ps)
            for k, p in enumerate(ps):
                want = quantile_ref(a, n, p)[0, 0, 0]
                assert same_bits(want, sp.model_quantile(v, p)), (msg, p)
                assert same_bits(want, sp.alt_quantile(v, p)), (msg, p)
                assert same_bits(want, planes[k]), (msg, p)
            for ns in NSIGMAS:
                c, s, cnt, mask = outliers_ref(a, n, ns)
                for other in (sp.model_outliers(v, ns), sp.alt_outliers(v, ns)):
                    assert same_bits(c[0, 0, 0], other[0]) and same_bits(s[0, 0, 0], other[1]), msg
                    assert cnt[0, 0, 0] == other[2] and (mask[:, 0, 0] == other[3]).all(), (msg, ns)
    # the time axis takes the same blocks
    v = blocks[17][0][3]
    a = np.asfortranarray(v.reshape(1, 1, 17))
    assert same_bits(quantile_ref(a, 17, 0.3, axis=2)[0, 0, 0], sp.alt_quantile(v, 0.3))
    assert same_bits(mad_ref(a, 17, axis=2)[0, 0, 0], sp.alt_mad(v))


# the wrong select, and the class of blocks aimed at it
WRONG = {"low_byte": "split3_ulp", "same_rank": "tie_last_finite", "zeros_equal": "split0_zeros",
         "ge_flag": "zero_majority", "lost_slot": "slots_five"}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_a_wrong_select_changes_the_bits(blocks, wrong):
    aimed, caught = WRONG[wrong], []
    for n, rows in blocks.items():
        for name, q, ps, v in rows:
            if name != aimed:
                continue
            right, bad = results(v, ps), results(v, ps, wrong)
            diff = sorted(k for k in right if right[k] != bad[k])
            if diff:
                caught.append((n, q, diff))
    assert caught, (wrong, aimed)
    print("%s: caught on %d blocks of %s, first %r" % (wrong, len(caught), aimed, caught[0]))
    # on every block length the class exists at.  (The order of the zeros shows in
    # the median of an odd block alone, which is the element itself: middle(),
    # quantile_mix and |x - c| all pass -0.0 through a sum that gives +0.0.)
    lengths = {n for n, rows in blocks.items() if any(r[0] == aimed for r in rows)}
    if wrong == "zeros_equal":
        lengths = {n for n in lengths if n % 2}
        assert all(d[0] == "median" for _, _, d in caught)
    assert {n for n, _, _ in caught} == lengths, (wrong, caught)


def test_the_table_carries_every_class():
    """Rows of the table, built: every class is planted somewhere, every
    order-statistic row carries the pass-0 .. pass-3 splits, the quantiles rows
    with sixteen ranks carry the slot classes, var / std rows the moments' data."""
    seen = set()
    rows = [c for c in sc.CASES if c.note == "ranks"][::4] + sc.CASES[::12]
    for c in rows:
        banks, carried = sp.build(c)
        assert len(banks) == c.nbank and all(
            b.shape == (c.nchan, c.nif, c.ntime) and b.dtype == np.float32 and b.flags.f_contiguous
            for b in banks), sc.case_id(c)
        names = set(carried)
        seen |= names
        if sc.kind(c) in ("var", "std"):
            assert names == set(sp.MOMENT_CLASSES), sc.case_id(c)
            assert all(np.isfinite(b).all() and np.abs(b).max() <= 1e9 for b in banks)
        elif c.n >= 2:
            assert names >= set(sp.PAIRS), (sc.case_id(c), sorted(names))
            if sc.kind(c) == "quantiles" and c.plan[8] == 16:
                assert names >= set(sp.SLOT_CLASSES), (sc.case_id(c), sorted(names))
        assert sp.build(c)[0][0] is banks[0]  # (cached: one array for every user)
    assert seen == set(sp.ALL_CLASSES), sorted(set(sp.ALL_CLASSES) - seen)
    # a quantile row is run at its own p and at both clamp ends
    c = next(c for c in sc.CASES if sc.kind(c) == "quantile")
    assert sp.quantile_probs(c)[1:] == (0.0, 1.0)
    assert rank_weight(c.n, 0.0)[0] - 1 == 0 and rank_weight(c.n, 1.0)[0] - 1 == c.n - 2
