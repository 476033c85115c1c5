"""Blocks built by key structure for the order-statistic kernels, and a CPU
model of their select that proves each block is what it claims to be.

The selects of stats.hip and tstats.hip are MSB-first radix selects over the
order-preserving uint32 image of the float, 8 bits a pass.  What they execute
depends on the bits of the data: the pass at which two ranks' prefixes part,
how many distinct prefixes (slots) a rank set occupies, how many digits a wave
meets, whether the next rank is the same key again or the smallest above.
`select_trace` is that select in plain NumPy (histograms, no sort); every
generator below asserts its claim with it.  `build(case)` fills the window of
a row of tests/stat_cases.py with such blocks: the first and the last blocks
of the window cycle through the classes the row's block length and ranks
allow (`carried(case)` names them), the others hold noise and small-integer
ties.

The model also restates the results (median, mad, quantile, outliers) from the
selected keys, with the wrong selects of tests/test_stat_planted_host.py
switched in by name, and `alt_*` state them a third time from a sort by Python
struct-packed keys.
"""
from __future__ import annotations

import struct
import zlib
from collections import namedtuple

import numpy as np

import stat_cases as sc
from mad_ref import MAD_CONSTANT
from quantile_ref import rank_weight

F32 = np.float32
NAN = F32(np.nan)
INF = F32(np.inf)
U32 = np.uint32


def f2key(x):
    """isless order of Float32 as unsigned order (a NaN's key lies above +Inf's)."""
    u = np.ascontiguousarray(x, dtype=F32).view(U32)
    return np.where(u >> U32(31) != 0, ~u, u | U32(0x80000000)).astype(U32)


def key2f(k):
    k = np.asarray(k, dtype=U32)
    return np.where(k >> U32(31) != 0, k & U32(0x7fffffff), ~k).astype(U32).view(F32)


def bits(u):
    return np.asarray(u, dtype=U32).view(F32)


def key_of(x):
    """The key of one value, as an int."""
    return int(f2key(np.array([x], dtype=F32))[0])


# ---------------------------------------------------------------------------
# the select

Trace = namedtuple("Trace", "prefix slots count key selc tie")


def select_trace(keys, ranks, wrong=None):
    """The radix select of the sorted 0-based `ranks` among `keys`.  Per pass k:
    prefix[k][r], the key bits of rank r fixed after the pass; slots[k], the
    distinct prefixes entering it; count[k][r], the keys in the bin selected.
    key[r] is the selected key, selc[r] how many keys equal it and tie[r] the
    rank inside that tie run (what the time-split form's last pass leaves).
    wrong="lost_slot": from the fifth slot on a slot's ranks are not settled (a
    wave that scans one slot only); wrong="low_byte": three passes."""
    keys = np.asarray(keys, dtype=U32)
    ranks = [int(r) for r in ranks]
    assert ranks == sorted(ranks) and 0 <= ranks[0] and ranks[-1] < keys.size
    pre, rem = [0] * len(ranks), list(ranks)
    prefix, slots, count = [], [], []
    for ps in range(3 if wrong == "low_byte" else 4):
        shift = 24 - 8 * ps
        mask = 0 if ps == 0 else (0xffffffff << (shift + 8)) & 0xffffffff
        heads = sorted(set(pre))
        slots.append(len(heads))
        hist = {}
        for h in heads:
            sel = keys[(keys & U32(mask)) == U32(h)]
            hist[h] = np.bincount(((sel >> U32(shift)) & U32(255)).astype(np.int64), minlength=256)
        cnt = []
        for r in range(len(ranks)):
            if wrong == "lost_slot" and heads.index(pre[r]) >= 4:
                cnt.append(0)
                continue
            h = hist[pre[r]]
            cum = np.cumsum(h)
            d = int(np.searchsorted(cum, rem[r], side="right"))
            cnt.append(int(h[d]))
            rem[r] -= int(cum[d] - h[d])
            pre[r] |= d << shift
        prefix.append(tuple(pre))
        count.append(tuple(cnt))
    return Trace(prefix, slots, count, tuple(pre), count[-1], tuple(rem))


def next_key(keys, tr, r=0, wrong=None):
    """The key of the rank after ranks[r] by the time-split form's rule: the
    same key again while the tie run lasts, else the smallest key above."""
    if wrong == "same_rank" or tr.tie[r] + 1 < tr.selc[r]:
        return tr.key[r]
    return int(np.asarray(keys, dtype=U32)[np.asarray(keys, dtype=U32) > U32(tr.key[r])].min())


# ---------------------------------------------------------------------------
# the results, from the model's keys

def _keys(x, wrong):
    x = np.asarray(x, dtype=F32)
    if wrong == "zeros_equal":
        x = x + F32(0.0)  # (-0.0 + 0.0 is +0.0)
    return f2key(x)


def _pair(x, q, wrong):
    """The values of ranks q and q + 1 (q itself where it is the last)."""
    keys = _keys(x, wrong)
    tr = select_trace(keys, [q], wrong)
    ka = tr.key[0]
    kb = ka if q + 1 >= keys.size else next_key(keys, tr, 0, wrong)
    if wrong is None and q + 1 < keys.size:  # the two ranks selected side by side: the same keys
        assert select_trace(keys, [q, q + 1]).key == (ka, kb)
    a, b = key2f([ka, kb])
    return a, b


def mix(a, b, g):
    """quantile_ref's join of two neighbours with weight g."""
    g = np.float64(g)
    with np.errstate(invalid="ignore", over="ignore"):
        if np.isfinite(a) and np.isfinite(b):
            return F32(np.float64(a) + g * np.float64(F32(b - a)))
        return F32((np.float64(1.0) - g) * np.float64(a) + g * np.float64(b))


def middle(a, b):
    with np.errstate(invalid="ignore"):
        return F32(F32(a * F32(0.5)) + F32(b * F32(0.5)))


def model_median(x, wrong=None):
    x = np.asarray(x, dtype=F32)
    if np.isnan(x).any():
        return NAN
    n = x.size
    a, b = _pair(x, (n - 1) // 2, wrong)
    return a if n % 2 else middle(a, b)


def model_quantile(x, p, wrong=None):
    x = np.asarray(x, dtype=F32)
    if np.isnan(x).any():
        return NAN
    j, g = rank_weight(x.size, p)
    a, b = _pair(x, j - 1, wrong)
    return mix(a, b, g)


def model_quantiles(x, ps, wrong=None):
    """Every plane from ONE select of the distinct ranks, as k_quantiles_select."""
    x = np.asarray(x, dtype=F32)
    if np.isnan(x).any():
        return np.full(len(ps), NAN)
    jg = [rank_weight(x.size, p) for p in ps]
    ranks = sorted({j - 1 for j, _ in jg} | {j for j, _ in jg})
    tr = select_trace(_keys(x, wrong), ranks, wrong)
    val = dict(zip(ranks, key2f(tr.key)))
    return np.array([mix(val[j - 1], val[j - 1 if wrong == "same_rank" else j], g) for j, g in jg],
                    dtype=F32)


def model_mad(x, wrong=None):
    x = np.asarray(x, dtype=F32)
    c = model_median(x, wrong)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(x - c)
        return F32(np.float64(model_median(d, wrong)) * MAD_CONSTANT)


def model_outliers(x, nsigma, wrong=None):
    """(median, mad, count, flags)"""
    x = np.asarray(x, dtype=F32)
    c, s = model_median(x, wrong), model_mad(x, wrong)
    with np.errstate(invalid="ignore", over="ignore"):
        thr = F32(np.float64(nsigma) * np.float64(s))
        d = np.abs(x - c)
        f = d >= thr if wrong == "ge_flag" else d > thr
    if np.isnan(c) or np.isnan(s):
        f = np.zeros(x.size, bool)
    return c, s, np.uint32(f.sum()), f.astype(np.uint8)


# ---------------------------------------------------------------------------
# a third statement: a sort by Python struct-packed keys

def struct_key(v):
    u = struct.unpack(">I", struct.pack(">f", v))[0]
    return (~u & 0xffffffff) if u >> 31 else (u | 0x80000000)


def struct_sorted(x):
    return [F32(v) for v in sorted(np.asarray(x, dtype=F32).tolist(), key=struct_key)]


def alt_median(x):
    x = np.asarray(x, dtype=F32)
    if any(v != v for v in x.tolist()):
        return NAN
    s, n = struct_sorted(x), x.size
    return s[n // 2] if n % 2 else middle(s[n // 2 - 1], s[n // 2])


def alt_quantile(x, p):
    x = np.asarray(x, dtype=F32)
    if any(v != v for v in x.tolist()):
        return NAN
    s = struct_sorted(x)
    j, g = rank_weight(x.size, p)
    return mix(s[j - 1], s[j], g)


def alt_mad(x):
    x = np.asarray(x, dtype=F32)
    c = alt_median(x)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.array([abs(F32(v - c)) for v in x], dtype=F32)
        return F32(np.float64(alt_median(d)) * MAD_CONSTANT)


def alt_outliers(x, nsigma):
    x = np.asarray(x, dtype=F32)
    c, s = alt_median(x), alt_mad(x)
    with np.errstate(invalid="ignore", over="ignore"):
        thr = F32(np.float64(nsigma) * np.float64(s))
        f = np.array([bool(abs(F32(v - c)) > thr) for v in x])
    if c != c or s != s:
        f[:] = False
    return c, s, np.uint32(f.sum()), f.astype(np.uint8)


# ---------------------------------------------------------------------------
# the generators: gen(n, q, ranks, rng) -> the block in sorted order, or None
# where n (or the rank) does not allow the class.  q is the lower of the two
# ranks a result joins, ranks the whole sorted rank set of the call.

def _below(a, k):
    return [F32(a - F32(0.5) * F32(j)) for j in range(k, 0, -1)]


def _above(b, k):
    return [F32(b + F32(0.5) * F32(j)) for j in range(1, k + 1)]


def _first_split(tr):
    """The pass at which the two ranks of a trace part, or None."""
    for k, pre in enumerate(tr.prefix):
        if pre[0] != pre[1]:
            return k
    return None


PAIRS = {"split0_sign": (F32(-1.5), F32(2.5), 0),
         "split0_zeros": (F32(-0.0), F32(0.0), 0),
         "split1": (F32(bits(0x3f800000)), F32(bits(0x3f810000)), 1),
         "split2": (F32(bits(0x3f800000)), F32(bits(0x3f800100)), 2),
         "split3_ulp": (F32(bits(0x3f800000)), F32(bits(0x3f800001)), 3),
         "split_never": (F32(1.0), F32(1.0), None)}


def gen_split(name):
    a, b, want = PAIRS[name]

    def gen(n, q, ranks, rng):
        if not 0 <= q <= n - 2:
            return None
        v = np.array(_below(a, q) + [a, b] + _above(b, n - q - 2), dtype=F32)
        tr = select_trace(f2key(v), [q, q + 1])
        assert _first_split(tr) == want and key2f(tr.key).tobytes() == v[q:q + 2].tobytes(), name
        return v
    return gen


def gen_tie(where, above):
    """Rank q first in (0), inside (1) or last in (2) a run of three equal keys
    whose upper neighbour is finite, +Inf or a NaN key."""
    def gen(n, q, ranks, rng):
        s = q - where
        if s < 0 or s + 3 > n - 1:
            return None
        top = n - s - 3
        up = {"finite": _above(F32(4.0), top), "inf": [INF] * top, "nan": [NAN] * top}[above]
        v = np.array(_below(F32(4.0), s) + [F32(4.0)] * 3 + up, dtype=F32)
        keys = f2key(v)
        tr = select_trace(keys, [q])
        assert tr.selc[0] == 3 and tr.tie[0] == where and tr.key[0] == key_of(4.0)
        assert next_key(keys, tr) == key_of(v[q + 1]) == int(keys[q + 1])
        return v
    return gen


def gen_one_digit(n, q, ranks, rng):
    """Three top bytes shared: the 64 lanes of a wave on one counter through pass 2."""
    v = np.sort(bits(U32(0x40490f00) | rng.integers(0, 256, n).astype(U32)))
    assert len(set((f2key(v) >> U32(8)).tolist())) == 1
    return v


def gen_two_digits(n, q, ranks, rng):
    top = rng.choice(np.array([0x3f, 0x40], dtype=U32), n)
    top[:2] = (0x3f, 0x40)
    v = bits((top << U32(24)) | rng.integers(0, 1 << 24, n).astype(U32))
    assert len(set((f2key(v) >> U32(24)).tolist())) == 2 and np.isfinite(v).all()
    return v


def gen_many_digits(n, q, ranks, rng):
    if n < 3:
        return None
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    v[:3] = (F32(-3.0), F32(1e-20), F32(5e10))
    assert len(set((f2key(v) >> U32(24)).tolist())) >= 3
    return v


def gen_all256(n, q, ranks, rng):
    """Every top byte of the key, from -Inf through subnormals of both signs to +Inf."""
    if n < 256:
        return None
    tb = np.concatenate([np.arange(256), rng.integers(0, 256, n - 256)]).astype(U32)
    low = rng.integers(0, 1 << 24, n).astype(U32)
    low[tb == 0x00] |= U32(0x7fffff)            # (-Inf and the finite keys above it; below is NaN)
    low[tb == 0xff] &= U32(0x7fffff)            # (up to +Inf: 0x7f800000)
    keys = (tb << U32(24)) | low
    keys[0] = U32(0x007fffff)                   # -Inf
    keys[255] = U32(0xff800000)                 # +Inf
    keys[0x7f] = U32(0x7f800000) | (keys[0x7f] & U32(0x3fffff))  # a negative subnormal
    keys[0x80] = U32(0x80000001) | (keys[0x80] & U32(0x7fffff))  # a positive subnormal
    v = key2f(keys)
    assert not np.isnan(v).any() and len(set((f2key(v) >> U32(24)).tolist())) == 256
    tiny = np.finfo(F32).tiny
    sub = (v != 0) & (np.abs(v) < tiny)
    assert (v == -INF).any() and (v == INF).any() and (sub & (v < 0)).any() and (sub & (v > 0)).any()
    return v


def _grouped(n, group_of_rank, ranks, rng):
    """Sorted keys whose top byte is 0x90 + the group of the largest rank <= the
    position (group 0 below the first rank), the low 24 bits ascending within a group."""
    grp = np.zeros(n, dtype=np.int64)
    for k, r in enumerate(ranks):
        grp[r:] = group_of_rank(k)
    low = rng.integers(0, 1 << 24, n).astype(np.int64)
    order = np.lexsort((low, grp))
    keys = ((U32(0x90) + grp[order].astype(U32)) << U32(24)) | low[order].astype(U32)
    return key2f(keys)


def gen_slots_one(n, q, ranks, rng):
    """Every rank in one slot through pass 2; they part at pass 3."""
    if len(ranks) < 3:
        return None
    v = bits(U32(0x40490f00) | (np.arange(n) * 256 // n).astype(U32))
    tr = select_trace(f2key(v), ranks)
    assert tr.slots == [1, 1, 1, 1] and len(set(tr.prefix[2])) == 1
    assert len(set(tr.key)) == len(set(f2key(v)[list(ranks)].tolist()))
    if n <= 256:
        assert len(set(tr.key)) == len(ranks)
    return v


def gen_slots_all(n, q, ranks, rng):
    """A slot per rank from pass 0: neighbouring ranks lie across a slot boundary."""
    if len(ranks) < 3:
        return None
    v = _grouped(n, lambda k: k + 1, ranks, rng)
    tr = select_trace(f2key(v), ranks)
    assert tr.slots[0] == 1 and tr.slots[1:] == [len(ranks)] * 3
    for a, b, pa, pb in zip(ranks, ranks[1:], tr.prefix[0], tr.prefix[0][1:]):
        assert pa != pb and (b != a + 1 or pa < pb)
    return v


def gen_slots_five(n, q, ranks, rng):
    """Five slots from pass 0 (a wave scans a second one), of unequal numbers of ranks."""
    nr = len(ranks)
    if nr < 6:
        return None
    v = _grouped(n, lambda k: 1 + k * 5 // nr, ranks, rng)
    tr = select_trace(f2key(v), ranks)
    sizes = [tr.prefix[0].count(p) for p in sorted(set(tr.prefix[0]))]
    assert tr.slots[1] == 5 and len(set(sizes)) > 1
    return v


def gen_dev_pairs(n, q, ranks, rng):
    """Deviations that tie in pairs: c +- d."""
    c = F32(10.0)
    half = [F32(0.5) * F32(j) for j in range(1, n // 2 + 1)]
    v = np.array([c - d for d in half] + ([c] if n % 2 else []) + [c + d for d in half], dtype=F32)
    d = np.sort(np.abs(v - alt_median(v)))
    assert (d[n % 2::2] == d[n % 2 + 1::2]).all() and (n < 4 or alt_mad(v) > 0)
    return v


def gen_zero_majority(n, q, ranks, rng):
    """More than half the block at the centre: mad = 0 and a threshold of 0."""
    k = n // 2 + 1
    v = np.array([F32(3.0)] * k + _above(F32(3.0), n - k), dtype=F32)
    c, s, cnt, f = alt_outliers(v, 5.0)
    assert c == F32(3.0) and s == 0 and cnt == n - k and (f == (v != c)).all()
    return v


def gen_inf_half(n, q, ranks, rng):
    """Half or more +Inf: the median is Inf, |Inf - Inf| is NaN, mad is NaN."""
    k = (n + 1) // 2
    v = np.array(_below(F32(2.0), n - k) + [INF] * k, dtype=F32)
    c, s, cnt, f = alt_outliers(v, 5.0)
    assert c == INF and np.isnan(s) and cnt == 0
    return v


def gen_half_ties(n, q, ranks, rng):
    """An even block whose two middle values are subnormals with an inexact half:
    a/2 + b/2 with each half rounded first is not the once-rounded (a + b)/2 that
    a fused multiply-add of either half gives (1 and 2, or 2 and 5, units of 2^-149)."""
    if n % 2:
        return None
    a, b = ((1, 2), (2, 5))[int(rng.integers(2))]
    a, b = F32(bits(a)), F32(bits(b))
    h = n // 2 - 1
    v = np.array(_below(F32(-1.0), h) + [a, b] + _above(F32(1.0), h), dtype=F32)
    two = middle(a, b)
    for fused in (F32(np.float64(a) * 0.5 + np.float64(F32(b * F32(0.5)))),
                  F32(np.float64(b) * 0.5 + np.float64(F32(a * F32(0.5))))):
        if fused != two:
            break
    else:
        raise AssertionError("no fused form differs")
    assert alt_median(v) == two and two in (F32(bits(1)), F32(bits(3)))
    return v


def gen_nan(n, q, ranks, rng):
    v = (rng.standard_normal(n) * 1e3).astype(F32)
    v[int(rng.integers(n))] = NAN
    return v


ORDER_CLASSES = {name: gen_split(name) for name in PAIRS}
for _w, _wn in enumerate(("first", "inside", "last")):
    for _a in ("finite", "inf", "nan"):
        ORDER_CLASSES["tie_%s_%s" % (_wn, _a)] = gen_tie(_w, _a)
RANK_FREE = {"one_digit": gen_one_digit, "two_digits": gen_two_digits,
             "many_digits": gen_many_digits, "all256": gen_all256,
             "dev_pairs": gen_dev_pairs, "zero_majority": gen_zero_majority,
             "inf_half": gen_inf_half, "nan_block": gen_nan, "half_ties": gen_half_ties}
SLOT_CLASSES = {"slots_one": gen_slots_one, "slots_all": gen_slots_all,
                "slots_five": gen_slots_five}
# var / std: the data of test_gpu_stats.py and test_gpu_tstat.py (finite, of
# moderate size), and the constant block the files promise an exact 0.0 for
MOMENT_CLASSES = {
    "noise": lambda n, q, ranks, rng: noise(n, rng),
    "ties": lambda n, q, ranks, rng: rng.integers(0, 8, n).astype(F32),
    "gamma": lambda n, q, ranks, rng: rng.gamma(2.0, 50.0, n).astype(F32),
    "const": lambda n, q, ranks, rng: np.full(n, F32(3.0000001)),
    "const_big": lambda n, q, ranks, rng: np.full(n, F32(1e9)),
}
ALL_CLASSES = (tuple(ORDER_CLASSES) + tuple(RANK_FREE) + tuple(SLOT_CLASSES) +
               tuple(MOMENT_CLASSES))


def noise(n, rng):
    """Signed normals with some zeros of both signs: finite and of moderate size,
    what the Float32 bound of var / std is stated for (a block of subnormals
    underflows in Float32 whatever the kernel does)."""
    a = (rng.standard_normal(n) * 1e3).astype(F32)
    hit = rng.random(n) < 0.05
    a[hit] = rng.choice(np.array([0.0, -0.0], F32), int(hit.sum()))
    return a


def lower_rank(n, p):
    return rank_weight(n, p)[0] - 1


def rank_set(n, ps):
    """The sorted distinct ranks {j - 1, j} of quantiles(ps) on blocks of n."""
    low = {lower_rank(n, p) for p in ps}
    return tuple(sorted(low | {q + 1 for q in low}))


def quantile_probs(case):
    """The probabilities a quantile row is run with: its own and both clamp ends."""
    return (sc.probs(case)[0], 0.0, 1.0)


def combos(case):
    """[(class name, generator, q, ranks)] a row's blocks cycle through."""
    n, op = case.n, sc.kind(case)
    if op in ("var", "std"):
        return [(name, g, 0, ()) for name, g in MOMENT_CLASSES.items()]
    if n < 2:
        return [("noise", MOMENT_CLASSES["noise"], 0, ())]
    med = ((n - 1) // 2, n // 2)
    if op == "quantile":
        q0 = lower_rank(n, sc.probs(case)[0])
        ranks, own, ends = (q0, q0 + 1), [q0], [q for q in (0, n - 2) if q != q0]
    elif op == "quantiles":
        ranks = rank_set(n, sc.probs(case))
        low = sorted({lower_rank(n, p) for p in sc.probs(case)})
        own, ends = sorted({low[0], low[-1]}), []
    else:
        ranks, own, ends = tuple(sorted(set(med))), [med[0]], []
    out = [(name, g, q, ranks) for q in own for name, g in ORDER_CLASSES.items()]
    out += [(name, ORDER_CLASSES[name], q, ranks) for q in ends for name in PAIRS]
    out += [(name, g, own[0], ranks) for name, g in RANK_FREE.items()]
    if op == "quantiles":
        out += [(name, g, own[0], ranks) for name, g in SLOT_CLASSES.items()]
    return out


def block_index(case):
    """Per block of the window, in the order build() plants them: the index
    arrays (channels, IF, spectra) of its n elements in the array."""
    w = sc.window(case)
    c = w[0] + w[2] * np.arange(w[1])
    i = w[3] + w[5] * np.arange(w[4])
    t = w[6] + w[8] * np.arange(w[7])
    n = max(case.n, 1)
    if case.axis == 0:
        return [(c[j * n:(j + 1) * n], ii, tt) for tt in t for ii in i for j in range(w[1] // n)]
    return [(cc, ii, t[b * n:(b + 1) * n]) for b in range(w[7] // n) for ii in i for cc in c]


_BUILT = {}


def build(case):
    """(banks, carried): the row's Fortran-ordered Float32 arrays, one per bank,
    and the class names planted, with their block counts.  The same arrays on
    every call (they are cached: do not write into them)."""
    cid = sc.case_id(case)
    if cid in _BUILT:
        return _BUILT[cid]
    seed = zlib.crc32(cid.encode())
    rng = np.random.default_rng(seed)
    shape = (case.nchan, case.nif, case.ntime)
    todo = combos(case)
    idx = block_index(case)
    nblk = len(idx)
    edge = 2 * len(todo)
    banks, carried, turn = [], {}, 0
    for bank in range(case.nbank):
        a = np.asfortranarray((rng.standard_normal(shape) * 1e3).astype(F32))
        tie_rows = rng.random(shape[1:]) < 0.5  # whole (IF, spectrum) rows of small integers
        a[:, tie_rows] = rng.integers(0, 8, (shape[0], int(tie_rows.sum()))).astype(F32)
        for b in range(nblk):
            if edge <= b < nblk - edge:
                continue
            for _ in range(len(todo)):
                name, gen, q, ranks = todo[turn % len(todo)]
                turn += 1
                v = gen(max(case.n, 1), q, ranks, np.random.default_rng(seed + 7919 * turn))
                if v is not None:
                    break
            else:
                continue
            cc, ii, tt = idx[b]
            a[cc, ii, tt] = rng.permutation(v)
            carried[name] = carried.get(name, 0) + 1
        banks.append(a)
    _BUILT[cid] = (banks, carried)
    return _BUILT[cid]


def carried(case):
    """The classes the row's arrays carry."""
    return tuple(sorted(build(case)[1]))
