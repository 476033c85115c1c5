"""Planted signed data for the Float32 reduce, and a plain NumPy reference.

`planted` fills banks with small integers in which every output block has one
known maximum and one known minimum; `offsets` shifts them to all-negative,
mixed and all-positive values; `special` adds NaN, +-Inf and signed zeros.  All
sums are exact in Float32 in any order (checked here), so `reference` (int64
sums, integer max / min, converted once) is compared bit for bit.

Blocks are numbered j = co + nco (i + ni (to + nto bank)); position p of a block
is element (f, t) of its F x T channels x spectra, p = f + F t.
"""
from __future__ import annotations

import math

import numpy as np

OPS = ("sum", "mean", "max", "min")
SETS = ("neg", "mixed", "pos", "special")
EXACT = 2 ** 24  # integers below it are Float32 values, and so are their partial sums


def params(F, T):
    """(B, P, C): base values in [-B, B], plants +-(P .. P + 6), offset C with
    F T (C + P + 7 + B) < 2^24, so that every partial sum of every set is an
    integer below 2^24 in magnitude: exact in Float32 in any order."""
    n = F * T
    for B, P in ((1, 3), (1, 2)):
        C = P + 7 + B + 1
        if n * (C + P + 7 + B) < EXACT:
            return B, P, C
    raise AssertionError("F T = %d: no exact planted data" % n)


def window_shape(shape, window):
    return tuple(shape) if window is None else (window[1], window[4], window[7])


def _axes(shape, window):
    if window is None:
        return [np.arange(n) for n in shape]
    return [window[3 * k] + window[3 * k + 2] * np.arange(window[3 * k + 1]) for k in range(3)]


def stride_of(n):
    """The walk's stride: the integer nearest 0.618 n, from there upward, that is coprime to n."""
    s = max(1, int(0.618 * n))
    while math.gcd(s, n) != 1:
        s += 1
    return s


def positions(n, j):
    """In-block positions of the +P_j and the -P'_j plant of block(s) j in
    blocks of n elements: p = j s mod n for a stride s coprime to n, and the
    position before it (mod n).  Block 0 holds both ends, 0 and n - 1; n
    consecutive blocks hold every position once, for either plant; the two
    never meet.  (n = 1: one element, +P_j in even blocks and -P'_j in odd
    ones.)"""
    j = np.asarray(j, np.int64)
    plus = (j * stride_of(n)) % n
    return plus, (plus + n - 1) % n


def plant_values(P, j):
    j = np.asarray(j, np.int64)
    return P + j % 7, P + (j + 3) % 7


def _coords(shape, window, F, T, j, p):
    """Array index (c, i, t) of position p of block j of one bank (j without the bank term)."""
    nc, ni, nt = window_shape(shape, window)
    nco = nc // F
    ax = _axes(shape, window)
    co, i, to = j % nco, (j // nco) % ni, j // (nco * ni)
    return ax[0][co * F + p % F], ax[1][i], ax[2][to * T + p // F]


def planted(shape, window, F, T, nbank, seed):
    """nbank Fortran-order Float32 arrays of `shape`: uniform integers in
    [-B, B], in every block of the window one +P_j and one -P'_j (positions,
    plant_values), and outside the window +-(P + 7 + B) in turn, which would
    show in any block that read them."""
    B, P, C = params(F, T)
    nc, ni, nt = window_shape(shape, window)
    assert nc % F == 0 and nt % T == 0
    per = (nc // F) * ni * (nt // T)
    n = F * T
    rng = np.random.default_rng(seed)
    banks = []
    for b in range(nbank):
        base = rng.integers(-B, B + 1, size=(nc, ni, nt), dtype=np.int8)
        a = np.empty(shape, np.float32, order="F")
        if window is not None:
            flat = a.reshape(-1, order="F")  # (a view: `a` is Fortran-contiguous)
            flat[0::2], flat[1::2] = P + 7 + B, -(P + 7 + B)
        view(a, window)[...] = base
        j = np.arange(per, dtype=np.int64)
        plus, minus = positions(n, j + b * per)
        vp, vm = plant_values(P, j + b * per)
        if n == 1:
            a[_coords(shape, window, F, T, j, plus)] = np.where((j + b * per) % 2 == 0, vp, -vm)
        else:
            a[_coords(shape, window, F, T, j, plus)] = vp
            a[_coords(shape, window, F, T, j, minus)] = -vm
        banks.append(a)
    assert n * (C + P + 7 + B) < EXACT
    return banks


def offsets(banks, F, T):
    """{"neg": u - C, "mixed": u, "pos": u + C}"""
    C = np.float32(params(F, T)[2])
    return {"neg": [u - C for u in banks], "mixed": banks, "pos": [u + C for u in banks]}


# the special set: what goes where, by block (spread over the case's blocks)
ROLES = ("nan", "+inf", "-inf", "zeros", "negzeros", "nan", "nan")


def special_blocks(nblocks):
    """{block: role}: three NaN blocks, a +Inf, a -Inf, a +0.0 block with one
    -0.0 and a -0.0 block with one +0.0, as far as the case has blocks."""
    out = {}
    for k, role in enumerate(ROLES):
        j = (k * nblocks) // len(ROLES) if nblocks >= len(ROLES) else k
        if j < nblocks and j not in out:
            out[j] = role
    return out


def special(banks, shape, window, F, T):
    """The mixed set with special_blocks' changes, each at its block's +P_j
    position (-Inf at the -P'_j one).  Blocks of one element take no zero
    role: Julia's fqav returns F = T = 1 unchanged, so its sign is not a
    reduction's."""
    nc, ni, nt = window_shape(shape, window)
    per = (nc // F) * ni * (nt // T)
    n = F * T
    out = [u.copy(order="F") for u in banks]
    for j, role in special_blocks(per * len(banks)).items():
        a, jj = out[j // per], np.int64(j % per)
        plus, minus = positions(n, j)
        at = _coords(shape, window, F, T, jj, plus)
        if role in ("zeros", "negzeros"):
            if n == 1:
                continue
            fill, one = (0.0, -0.0) if role == "zeros" else (-0.0, 0.0)
            allp = np.arange(n)
            a[_coords(shape, window, F, T, jj, allp)] = np.float32(fill)
            a[at] = np.float32(one)
        elif role == "-inf":
            a[_coords(shape, window, F, T, jj, minus if n > 1 else plus)] = -np.inf
        else:
            a[at] = np.nan if role == "nan" else np.inf
    return out


def view(a, window):
    """The window of `a` (a view where its steps are positive)."""
    if window is None:
        return a
    if min(window[2::3]) > 0:
        return a[tuple(slice(window[3 * k], window[3 * k] + window[3 * k + 1] * window[3 * k + 2],
                             window[3 * k + 2]) for k in range(3))]
    return a[np.ix_(*_axes(a.shape, window))]


def blocks(a, window, F, T):
    """The window of `a` as (F, nco, ni, T, nto)."""
    w = view(a, window)
    nc, ni, nt = w.shape
    return np.asfortranarray(w).reshape((F, nc // F, ni, T, nt // T), order="F")


def _reduce_int(R, op):
    """(nco, ni, nto) Float32 of integer-valued blocks R: int64 sums, converted once."""
    n = R.shape[0] * R.shape[3]
    if op in ("sum", "mean"):
        s = R.sum(axis=(0, 3), dtype=np.int64)
        assert np.abs(s).max(initial=0) < EXACT
        # (mean: the double quotient of two integers below 2^24 is further than
        # 2^-53 relative from every Float32 rounding boundary it does not sit
        # on, so rounding it again gives Float32(s / n))
        return (s if op == "sum" else s / np.float64(n)).astype(np.float32)
    return (R.max(axis=(0, 3)) if op == "max" else R.min(axis=(0, 3))).astype(np.float32)


def _reduce_special(v, op):
    """One block's values (any special ones) by Julia's rules: NaN propagates,
    -0.0 < +0.0, sums start from +0.0."""
    if np.isnan(v).any():
        return np.float32(np.nan)
    if op in ("sum", "mean"):
        s = v.astype(np.float64).sum() + 0.0
        return np.float32(s if op == "sum" else s / v.size)
    m = v.max() if op == "max" else v.min()
    if m == 0:
        neg = np.signbit(v[v == 0])
        m = np.float32(-0.0) if (neg.all() if op == "max" else neg.any()) else np.float32(0.0)
    return np.float32(m)


def references(banks, window, F, T, fix=None):
    """{op: the stitched (nbank nco, ni, nto) Float32 result over the banks}.
    fix: the banks whose non-integer blocks (special_blocks) are recomputed by
    _reduce_special; `banks` are then the integer banks they were made of."""
    Rs = [blocks(u, window, F, T) for u in banks]
    res = {op: np.asfortranarray(np.concatenate([_reduce_int(R, op) for R in Rs], axis=0))
           for op in OPS}
    return res if fix is None else patched(res, fix, window, F, T)


def patched(refs, fix, window, F, T):
    """references() of the integer banks, with the blocks that special() changed in `fix` redone."""
    refs = {op: r.copy(order="F") for op, r in refs.items()}
    nco, ni, nto = refs["sum"].shape
    nco //= len(fix)
    per = nco * ni * nto
    for j in special_blocks(per * len(fix)):
        b, jj = divmod(j, per)
        co, i, to = jj % nco, (jj // nco) % ni, jj // (nco * ni)
        v = view(fix[b], window)[co * F:(co + 1) * F, i, to * T:(to + 1) * T].ravel()
        for op in OPS:
            refs[op][b * nco + co, i, to] = _reduce_special(v, op)
    return refs


def reference(banks, window, F, T, op, fix=None):
    return references(banks, window, F, T, fix)[op]


def pow2(n):
    return n & (n - 1) == 0


# mean: every kernel ends with finish(): s / a.div, a Float32 division of the
# block's sum by (float)(F T).  Both operands are exact here (s and F T below
# 2^24), and the library is compiled without fast-math, where HIP's Float32
# division is correctly rounded (v_div_scale / v_div_fmas / v_div_fixup): the
# result is Float32(s / (F T)) itself.  Time-chunked plans divide once, in the
# finalize kernel, after summing exact partials.  So 0 ulp everywhere, a power
# of two or not; MEAN_ULP is where a looser division would have to be admitted
# (the approximate one, rcp and a multiply, is within 2).
MEAN_ULP = 0


def ulps(got, want):
    """Distance in Float32 steps (finite values of equal sign or zero)."""
    g = np.asarray(got, np.float32).view(np.int32).astype(np.int64)
    w = np.asarray(want, np.float32).view(np.int32).astype(np.int64)
    g = np.where(g < 0, -(g & 0x7FFFFFFF), g)
    w = np.where(w < 0, -(w & 0x7FFFFFFF), w)
    return np.abs(g - w)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def mismatch(got, want, op, n):
    """None where `got` is right, else a short description.  Bit for bit; a
    mean over n elements, n not a power of two, within MEAN_ULP."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    if same_bits(got, want):
        return None
    if op == "mean" and not pow2(n) and MEAN_ULP:
        fin = np.isfinite(want)
        if same_bits(np.where(fin, 0, got), np.where(fin, 0, want)) and \
                ulps(got[fin], want[fin]).max(initial=0) <= MEAN_ULP:
            return None
    bad = np.argwhere(~((got == want) & (np.signbit(got) == np.signbit(want)) |
                        (np.isnan(got) & np.isnan(want))))
    k = tuple(bad[0])
    return "%d of %d outputs differ, first at %s: got %r, expected %r" % (
        len(bad), got.size, k, got[k], want[k])
