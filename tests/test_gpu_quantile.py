"""GPU: fqavfunc / tavfunc ("quantile", p) of Float32 windows (csrc/stats.hip,
csrc/tstats.hip with the quantile selector) against the rule restated in NumPy
(quantile_ref.py), bit for bit: every step of the rule (the isless order, the
Float64 index and weight, the once-rounded Float32 difference, the Float64
product and sum rounded to Float32) is exactly specified, so no tolerance
applies.  NaN results compare as NaN (conftest.same_bits).

Every block size is run on data with whole blocks planted with: a NaN, a
minority, exactly half and a majority of +Inf, some -Inf, +-floatmax
alternating (the difference overflows), subnormals with odd significands,
+-0.0, one value, and the integers 0..3 (heavy ties: the upper rank is "the
same key again" in the split form)."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits
from mad_ref import mad_ref, median_ref
from quantile_ref import quantile_ref, rank_weight

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NPLANT = 11
BELOW_ONE = float(np.nextafter(1.0, 0.0))


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def put(eng, a):
    return eng.fb_from_numpy(a, device="cuda:0")


# ---------------------------------------------------------------------------
# data: B blocks of n values as the columns of an (n, B) matrix

def make_blocks(n, B, seed):
    assert B >= NPLANT
    rng = np.random.default_rng(seed)
    M = rng.gamma(2.0, 5e8, (n, B)).astype(np.float32)
    M[:, 1::2] = (rng.standard_normal((n, (B + 0) // 2)) * 1e3).astype(np.float32)

    def some(k):  # k places of a block
        return rng.permutation(n)[:k]

    j = iter(range(B - 1, -1, -1))  # planted from the last block down
    M[some(1), next(j)] = np.nan
    M[some((n - 1) // 2), next(j)] = np.inf  # a minority
    M[some(n // 2), next(j)] = np.inf        # half
    M[some(n // 2 + 1), next(j)] = np.inf    # a majority
    M[some((n + 2) // 3), next(j)] = -np.inf
    M[:, next(j)] = rng.permutation(np.where(np.arange(n) % 2, FMAX, -FMAX).astype(np.float32))
    sub = (2 * rng.integers(0, 1 << 22, n) + 1).astype(np.uint32)  # odd significands
    sub |= rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    M[:, next(j)] = sub.view(np.float32)
    M[:, next(j)] = rng.choice(np.float32([0.0, -0.0]), n)
    M[:, next(j)] = np.float32(1234.5)
    M[:, next(j)] = rng.integers(0, 4, n).astype(np.float32)
    k = next(j)  # both infinities in one block
    M[some(1), k] = np.inf
    M[some(1), k] = -np.inf
    return M


def chan_array(F, nco, ni, nt, seed):
    """(F * nco, ni, nt): the blocks along the channels."""
    M = make_blocks(F, nco * ni * nt, seed)
    return np.asfortranarray(M.reshape((F * nco, ni, nt), order="F"))


def time_array(T, nc, ni, nb, seed):
    """(nc, ni, T * nb): the blocks along time."""
    M = make_blocks(T, nc * ni * nb, seed).reshape((T, nb, nc, ni), order="F")
    return np.asfortranarray(np.transpose(M, (2, 3, 1, 0)).reshape((nc, ni, nb * T)))


def exact_p(n):
    """A p = k / (n - 1) whose aleph = n p + 1 - p is the exact integer k + 1, the
    highest such rank above the first: g == 0 with 2 <= j <= n - 1 and no clamp
    (n = 2: only p = 0 does that, at j = 1)."""
    if n == 2:
        return 0.0
    for k in range(n - 2, 0, -1):
        p = k / (n - 1)
        j, g = rank_weight(n, p)
        if g == 0.0 and j == k + 1:
            return p
    raise AssertionError(n)


def full_ps(n):
    """0, 1, the middle and two others; g == 0 at an interior rank; j at each
    clamp end (trunc(aleph) = 1 from the smallest p, = n clamped to n - 1)."""
    return (0.0, 1.0, 0.5, 0.25, 0.9, exact_p(n), 1e-300, BELOW_ONE)


def short_ps(n):
    return (0.25, 1.0, exact_p(n))


def test_probabilities_do_what_they_are_there_for():
    for n in (2, 3, 5, 64, 100, 4100, 31, 272, 1024):
        j, g = rank_weight(n, exact_p(n))
        assert g == 0.0 and (2 <= j <= n - 1 if n > 2 else j == 1)
        assert rank_weight(n, 1e-300) == (1, 0.0)
        assert rank_weight(n, 1.0) == (n - 1, 1.0)
        assert rank_weight(n, BELOW_ONE)[0] == n - 1
    a = chan_array(8, NPLANT, 1, 1, 8)
    want = quantile_ref(a, 8, 0.5)
    assert np.isnan(want).sum() >= 1 and np.isinf(want).sum() >= 3 and (want == 1234.5).sum() == 1
    assert np.isnan(quantile_ref(a, 8, 1.0)).sum() >= 2  # (g == 1 next to an infinite a)


# ---------------------------------------------------------------------------
# the channel axis, every form

SORT_F = [2, 3, 4, 5, 7, 8, 16, 33, 63, 64]
SELECT_F = [65, 68, 100, 1024, 4095, 4096]
STREAM_F = [4097, 4100, 8192]
FULL_F = (64, 100, 4100)  # one size per form takes every probability
PATH_OF = {**{F: "median_sort" for F in SORT_F}, **{F: "median_select" for F in SELECT_F},
           **{F: "median_stream" for F in STREAM_F}}


def chan_shape(F):
    nco = max(2, min(512, 32768 // F))  # >= 12 blocks, <= 3072; 200k values at most
    return F, nco, 2, 3


def chan_windows(F, nco):
    nch = F * nco
    rest = [0, 2, 1, 0, 3, 1]
    return [None,                                    # float4 loads where 4 divides F
            [0, F * (nco // 2), 2] + rest,           # channel step 2: one dword per element
            [nch - 1, nch, -1] + rest,               # reversed
            [3, F * (nco - 2), 1] + rest]            # from channel 3: off a 16-byte boundary


@pytest.mark.parametrize("F", SORT_F + SELECT_F + STREAM_F)
def test_fqav_quantile_bits(eng, F):
    _, nco, ni, nt = chan_shape(F)
    a = chan_array(F, nco, ni, nt, F)
    x = put(eng, a)
    med = eng.plan(x, F, 1, "median")
    for p in full_ps(F) if F in FULL_F else short_ps(F):
        plan = eng.quantile_plan(x, F, p)
        assert plan["path"] == PATH_OF[F] == med["path"], (F, p)
        assert plan["rank"] == rank_weight(F, p)[0] - 1
        assert {**plan, "rank": 0} == {k if k != "workspace_bytes" else "rank": v
                                       for k, v in med.items()}
        assert plan == eng.plan(x, F, 1, ("quantile", p))
        for w in chan_windows(F, nco):
            got = eng.fb_to_numpy(eng.quantile(x, F, p, 0, w))
            want = quantile_ref(a, F, p, w)
            assert got.dtype == np.float32 and got.shape == want.shape
            assert same_bits(got, want), (F, p, w)


# ---------------------------------------------------------------------------
# the time axis, both forms

REGS_T = [2, 3, 5, 8, 16, 31, 32]
SPLIT_T = [33, 64, 100, 272, 1024]
FULL_T = (16, 100)


def time_shape(T, nc):
    return T, nc, 2, max(8, min(128, 8192 // T))


@pytest.mark.parametrize("T", REGS_T + SPLIT_T)
def test_tav_quantile_bits(eng, pkg, T):
    import torch

    path = "regs_median" if T <= 32 else "split_median"
    for nc in (8, 6):  # float4 columns, and one dword per lane
        _, _, ni, nb = time_shape(T, nc)
        a = time_array(T, nc, ni, nb, 100 * T + nc)
        x = put(eng, a)
        med = eng.tstat_plan(x, T, "median")
        w = [nc - 1, nc, -1, 0, ni, 1, T, T * (nb // 2), 1]  # channels reversed, half the blocks
        for p in full_ps(T) if T in FULL_T else short_ps(T):
            plan = eng.quantile_plan(x, T, p, 2)
            assert plan["path"] == path == med["path"], (T, nc, p)
            assert plan["passes"] == (1 if T <= 32 else 5)  # (the split form's fifth pass, always)
            assert plan["channels_per_lane"] == (4 if nc == 8 else 1)
            assert plan["rank"] == rank_weight(T, p)[0] - 1
            assert {**plan, "rank": 0, "passes": med["passes"]} == \
                {k if k != "workspace_bytes" else "rank": v for k, v in med.items()}
            want = quantile_ref(a, T, p, axis=2)
            got = eng.fb_to_numpy(eng.quantile(x, T, p, 2))
            assert got.dtype == np.float32 and same_bits(got, want), (T, nc, p)
            assert same_bits(eng.fb_to_numpy(eng.tstat(x, T, ("quantile", p), w)),
                             quantile_ref(a, T, p, w, axis=2)), (T, nc, p)
        p = 0.25
        want = quantile_ref(a, T, p, axis=2)
        # a strided out: the middle slot of a three-bank product
        big = eng.fb_empty(3 * nc, ni, nb, device="cuda:0")
        big.fill_(-7.0)
        r = eng.quantile(x, T, p, 2, out=big[nc:2 * nc])
        torch.cuda.synchronize()
        h = eng.fb_to_numpy(big)
        assert same_bits(h[nc:2 * nc], want) and (h[:nc] == -7.0).all() and (h[2 * nc:] == -7.0).all()
        assert r.data_ptr() == big[nc:2 * nc].data_ptr()
        # two stages: fqavfunc "sum", then tavfunc quantile of its result on the device
        s1 = eng.fb_to_numpy(eng.reduce(x, 2, 1, "sum"))
        r = pkg.worker.getdata(x, fqavby=2, fqavfunc="sum", tavby=T, tavfunc=pkg.quantile(p))
        assert isinstance(r, torch.Tensor) and r.is_cuda
        assert same_bits(eng.fb_to_numpy(r), quantile_ref(s1, T, p, axis=2)), (T, nc)


# ---------------------------------------------------------------------------
# the rule's special cases, and fqav's n <= 1

def test_special_cases_and_copy(eng, pkg):
    inf = np.inf
    rows = np.float32([[1, inf], [-inf, 1], [-FMAX, FMAX], [np.nan, 1], [0.0, -0.0], [1, 3]])
    a = np.asfortranarray(rows.reshape((12, 1, 1)))
    t = np.asfortranarray(rows.reshape((6, 1, 2)))
    for run in (lambda p: eng.fb_to_numpy(eng.quantile(put(eng, a), 2, p))[:, 0, 0],
                lambda p: eng.fb_to_numpy(eng.quantile(put(eng, t), 2, p, 2))[:, 0, 0]):
        lo, mid, hi = run(0.0), run(0.5), run(1.0)
        assert np.isnan(lo[0]) and mid[0] == inf and hi[0] == inf   # g == 0 next to an infinite b
        assert lo[1] == -inf and mid[1] == -inf and np.isnan(hi[1])  # g == 1 next to an infinite a
        assert np.isnan(lo[2]) and mid[2] == inf and hi[2] == inf    # d = b - a overflows Float32
        assert np.isnan([lo[3], mid[3], hi[3]]).all()                # NaN wins
        for z in (lo[4], mid[4], hi[4]):                             # -0.0 + g * 0.0
            assert z == 0.0 and not np.signbit(z)
        assert (lo[5], mid[5], hi[5]) == (1.0, 2.0, 3.0)
    five = np.asfortranarray(np.float32([4, 1, 5, 3, 2]).reshape((5, 1, 1)))
    assert eng.fb_to_numpy(eng.quantile(put(eng, five), 5, 0.25))[0, 0, 0] == 2.0
    assert eng.quantile_plan(put(eng, five), 5, 0.25)["rank"] == 1  # j = 2, g = 0
    # quantile(0.5) of an even block is a + 0.5 (b - a), not middle(a, b) = a/2 + b/2:
    # two subnormals with odd significands differ in the last bit
    sub = np.asfortranarray(np.uint32([1, 2]).view(np.float32).reshape((2, 1, 1)))
    q = eng.fb_to_numpy(eng.quantile(put(eng, sub), 2, 0.5))
    m = eng.fb_to_numpy(eng.reduce(put(eng, sub), 2, 1, "median"))
    assert same_bits(q, quantile_ref(sub, 2, 0.5)) and same_bits(m, median_ref(sub, 2))
    assert q.view(np.uint32)[0, 0, 0] == 2 and m.view(np.uint32)[0, 0, 0] == 1
    # fqav(A, n <= 1) is A whatever f is: the ABI copies the window
    x = put(eng, a)
    assert same_bits(eng.fb_to_numpy(eng.quantile(x, 1, 0.3)), a)
    assert same_bits(eng.fb_to_numpy(eng.reduce(x, 1, 1, pkg.quantile(0.3))), a)
    for n in (1, 0):  # (the tstat copy is the reduce's F = T = 1 sum for every op: values)
        assert np.array_equal(eng.fb_to_numpy(eng.quantile(put(eng, t), n, 0.3, 2))[4:], t[4:])
        assert same_bits(eng.fb_to_numpy(eng.quantile(put(eng, t), n, 0.3, 2)),
                         eng.fb_to_numpy(eng.tstat(put(eng, t), n, "median")))
    copy = eng.tstat_plan(x, 1, "median")
    assert copy.pop("workspace_bytes") == 0 and copy["path"] == "copy"
    assert eng.quantile_plan(x, 1, 0.3, 2) == {**copy, "rank": -1}
    assert pkg.fqav(x, 1, pkg.quantile(0.3)) is x
    with pytest.raises(TypeError, match="tavby"):
        eng.reduce(x, 2, 2, pkg.quantile(0.3))
    with pytest.raises(TypeError):
        eng.band_reduce_multi([x, x], 2, 1, pkg.quantile(0.3))
    with pytest.raises(TypeError, match="quantile"):
        eng.PreparedReduce(x, 2, 1, pkg.quantile(0.3))
    with pytest.raises(ValueError, match="quantile"):
        eng.quantile(x, 2, 1.5)
    with pytest.raises(pkg.DimensionMismatch):
        eng.quantile(x, 5, 0.5)


# ---------------------------------------------------------------------------
# exact properties

PROP = [("F", 64), ("F", 100), ("F", 4100), ("T", 16), ("T", 100)]


def run(eng, axis, a, n, op):
    x = put(eng, a)
    return eng.fb_to_numpy(eng.reduce(x, n, 1, op) if axis == "F" else eng.tstat(x, n, op))


@pytest.mark.parametrize("axis,n", PROP)
def test_permuting_a_block_changes_nothing(eng, pkg, axis, n):
    ax = 0 if axis == "F" else 2
    a = chan_array(n, 6, 2, 3, n) if axis == "F" else time_array(n, 8, 2, 6, n)
    rng = np.random.default_rng(n + 1)
    for p in (0.25, exact_p(n)):
        base = run(eng, axis, a, n, pkg.quantile(p))
        assert same_bits(base, quantile_ref(a, n, p, axis=ax))
        idx = (np.arange(a.shape[ax]) // n) * n + np.tile(rng.permutation(n), a.shape[ax] // n)
        b = np.asfortranarray(np.take(a, idx, axis=ax))
        assert same_bits(run(eng, axis, b, n, pkg.quantile(p)), base), (axis, n, p)


def one_binade(shape, seed):
    """Float32 data in [2^30, 2^31): every difference of two of them is exact
    (Sterbenz' lemma)."""
    rng = np.random.default_rng(seed)
    a = np.ldexp(rng.uniform(1.0, 2.0, shape), 30).astype(np.float32)
    top = np.nextafter(np.float32(2.0 ** 31), np.float32(0))
    return np.asfortranarray(np.minimum(a, top))


@pytest.mark.parametrize("axis,n", PROP + [("F", 2), ("T", 2), ("T", 1024)])
def test_the_ends_are_min_and_max(eng, pkg, axis, n):
    """quantile(0) = v[1] + 0 * d is the min op's result bit for bit on every
    block holding no NaN and no infinity whose d = v[2] - v[1] stays finite:
    random data of both signs (no zeros, |x| < 1e10).  quantile(1) = v[n-1] +
    1 * d with d = v[n] - v[n-1] rounded to Float32 is v[n], the max op's
    result, where that difference is exact; where it rounds, the rule as written
    returns Float32(v[n-1] + d), which need not be v[n] (quantile_ref of
    [1, 2^24 + 2] at p = 1 is 2^24: test_quantile_host.py).  So the upper end is
    compared on data in one binade, whose differences are exact, and the
    blocks where the rule departs from min / max (an infinite neighbour,
    +-floatmax whose d overflows, +-0.0 where -0.0 + 0 * 0.0 is +0.0, an
    inexact d at p = 1) are left to the bit-for-bit comparisons above."""
    rng = np.random.default_rng(n)
    shape = (n * 6, 2, 3) if axis == "F" else (8, 2, n * 6)
    a = rng.gamma(2.0, 5e8, shape).astype(np.float32)
    a[::3] = (rng.standard_normal(a[::3].shape) * 1e3).astype(np.float32)
    a = np.asfortranarray(a)
    assert np.isfinite(a).all() and (a != 0).all()
    for p, op, data in ((0.0, "min", a), (0.0, "min", one_binade(shape, n)),
                        (1.0, "max", one_binade(shape, n))):
        x = put(eng, data)
        ext = eng.reduce(x, n, 1, op) if axis == "F" else eng.reduce(x, 1, n, op)
        got = run(eng, axis, data, n, pkg.quantile(p))
        assert same_bits(got, eng.fb_to_numpy(ext)), (axis, n, p)


@pytest.mark.parametrize("axis,n", PROP)
def test_monotone_in_p(eng, pkg, axis, n):
    """The rule is monotone in p wherever b - a is exact: r = a + g (b - a) is
    then the exact interpolation rounded once to Float64 and once to Float32,
    both monotone, and consecutive ranks meet at v[j + 1].  (Where the Float32
    difference rounds up, a + g d can pass b by that rounding error just below
    g = 1, so the property is no consequence of the rule on data spanning
    binades.)  Data in one binade, [2^30, 2^31): Sterbenz' lemma makes every
    difference exact."""
    a = one_binade((n * 6, 2, 3) if axis == "F" else (8, 2, n * 6), n + 3)
    ps = sorted({0.0, 1e-300, 0.1, 0.25, 1 / 3, 0.5, exact_p(n), 0.75, 0.9, 0.99, BELOW_ONE, 1.0})
    res = [run(eng, axis, a, n, pkg.quantile(p)) for p in ps]
    for p, lo, hi in zip(ps[1:], res, res[1:]):
        assert (lo <= hi).all(), (axis, n, p)
    assert (res[0] < res[-1]).all()


@pytest.mark.parametrize("axis,n", PROP + [("F", 4), ("T", 1024)])
def test_median_and_mad_are_untouched(eng, pkg, axis, n):
    """The kernels are the median's with a selector: median and mad give the
    same bits before and after a quantile call on the same tensor, and they
    are the NumPy restatement's (mad_ref.py)."""
    ax = 0 if axis == "F" else 2
    a = chan_array(n, 6, 2, 3, n + 7) if axis == "F" else time_array(n, 8, 2, 6, n + 7)
    x = put(eng, a)

    def call(op):
        return eng.fb_to_numpy(eng.reduce(x, n, 1, op) if axis == "F" else eng.tstat(x, n, op))

    med, mad = call("median"), call("mad")
    q = call(pkg.quantile(0.25))
    assert same_bits(q, quantile_ref(a, n, 0.25, axis=ax))
    assert same_bits(call("median"), med) and same_bits(med, median_ref(a, n, axis=ax))
    assert same_bits(call("mad"), mad) and same_bits(mad, mad_ref(a, n, axis=ax))
    assert same_bits(eng.fb_to_numpy(x), a)  # the input is read only


# ---------------------------------------------------------------------------
# layers

def test_engine_layers(eng, pkg):
    import torch

    banks = [chan_array(64, 16, 2, 3, 20 + k) for k in range(2)]
    xs = [put(eng, b) for b in banks]
    for F, p in ((64, 0.25), (256, 0.9)):
        q = pkg.quantile(p)
        want = [quantile_ref(b, F, p) for b in banks]
        band = eng.fb_to_numpy(eng.band_quantile(xs, F, p))
        assert same_bits(band, np.concatenate(want, axis=0)), F
        assert same_bits(eng.fb_to_numpy(eng.band_reduce(xs, F, 1, q)), band)
        # a pageable host array through the GPU, and fqav on both kinds
        assert same_bits(eng.quantile_host(banks[0], F, p), want[0])
        assert same_bits(eng.reduce_host(banks[0], F, 1, q), want[0])
        assert same_bits(pkg.fqav(banks[0], F, q), want[0])
        r = pkg.fqav(xs[0], F, q)
        assert isinstance(r, torch.Tensor) and r.is_cuda and same_bits(eng.fb_to_numpy(r), want[0])
    win = [5, 512, 1, 1, 1, 1, 0, 2, 2]
    assert same_bits(eng.quantile_host(banks[0], 64, 0.25, 0, win),
                     quantile_ref(banks[0], 64, 0.25, win))
    t = time_array(48, 12, 2, 4, 9)
    for T in (16, 48):
        assert same_bits(eng.quantile_host(t, T, 0.75, 2), quantile_ref(t, T, 0.75, axis=2)), T
        assert same_bits(eng.tstat_host(t, T, pkg.quantile(0.75)), quantile_ref(t, T, 0.75, axis=2))
    win = [1, 8, 1, 1, 1, 1, 191, 96, -2]  # a reversed time range
    assert same_bits(eng.quantile_host(t, 16, 0.75, 2, win), quantile_ref(t, 16, 0.75, win, axis=2))
    tb = [t, time_array(48, 12, 2, 4, 10)]
    for T in (16, 48):
        band = eng.fb_to_numpy(eng.band_quantile([put(eng, b) for b in tb], T, 0.75, 2))
        assert same_bits(band, np.concatenate([quantile_ref(b, T, 0.75, axis=2) for b in tb], axis=0))
        assert same_bits(eng.fb_to_numpy(eng.band_tstat([put(eng, b) for b in tb], T,
                                                        pkg.quantile(0.75))), band)
    with pytest.raises(TypeError, match="Float32"):
        eng.reduce(xs[0].to(torch.int16), 4, 1, pkg.quantile(0.5))


def test_getdata_files_and_getband(eng, pkg, orc, tmp_path):
    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    lo, hi = pkg.quantile(0.25), pkg.quantile(0.75)
    data = chan_array(8, 8, 2, 40, 4)  # (64, 2, 40)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    bs = str(tmp_path / "bs.rawspec.0002.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=64), data)
    pkg.fbh5.write_bslz4(bs, dict(foff=-1.0, nfpc=64), data, (8, 1, 64),
                         lambda blk: orc.np_bslz4_encode(blk, 512, lz4=orc.lz4_compress))
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    for src in (fil, raw, bs):
        got = W.getdata(src, fqavby=8, fqavfunc=lo)
        assert got.dtype == np.float32 and same_bits(got, quantile_ref(data, 8, 0.25)), src
        assert same_bits(W.getdata(src, idxs, 16, lo), quantile_ref(data, 16, 0.25, win)), src
        assert same_bits(W.getdata(src, tavby=8, tavfunc=hi),
                         quantile_ref(data, 8, 0.75, axis=2)), src
        assert same_bits(W.getdata(src, idxs, tavby=16, tavfunc=hi),
                         quantile_ref(data, 16, 0.75, win, axis=2)), src
        with pytest.raises(TypeError, match="tavby"):
            W.getdata(src, fqavby=8, fqavfunc=lo, tavby=2)
        with pytest.raises(ValueError, match="quantile"):
            W.getdata(src, fqavby=8, fqavfunc=("quantile", 1.5))
    s1 = quantile_ref(data, 4, 0.25)
    assert same_bits(W.getdata(raw, fqavby=4, fqavfunc=lo, tavby=8, tavfunc=hi),
                     quantile_ref(s1, 8, 0.75, axis=2))
    want = quantile_ref(data, 8, 0.25)
    band = pkg.GBT.getband([0, 0], [fil, raw], fqavby=8, fqavfunc=lo)
    assert same_bits(band, np.concatenate([want, want], axis=0))
    staged = pkg.GBT.getband([0, 0], [fil, bs], fqavby=8, fqavfunc=lo, staged=True)
    assert same_bits(staged, np.concatenate([want, want], axis=0))
    s1 = eng.fb_to_numpy(eng.reduce(put(eng, data), 4, 1, "max"))
    tw = quantile_ref(s1, 8, 0.75, axis=2)
    band = pkg.GBT.getband([0, 0], [fil, bs], fqavby=4, fqavfunc="max", tavby=8, tavfunc=hi)
    assert same_bits(band, np.concatenate([tw, tw], axis=0))
    parts = pkg.GBT.getdata([0, 0], [fil, bs], fqavby=8, fqavfunc=lo)
    assert all(same_bits(p, want) for p in parts)
    # the device path keeps the product on the GPU
    r = W.getdata_device(fil, fqavby=8, fqavfunc=lo)
    assert same_bits(eng.fb_to_numpy(r), want)
