"""GPU: fqavfunc / tavfunc "mad" of Float32 windows (csrc/stats.hip,
csrc/tstats.hip with MAD set) against the rule restated in NumPy (mad_ref.py),
bit for bit: every step of the rule (the two medians, the once-rounded
difference, the Float64 product rounded to Float32) is exactly specified, so
no tolerance applies.  NaN results compare as NaN (conftest.same_bits).

Every block size is run on data with whole blocks planted with: a NaN, a
minority, exactly half and a majority of +Inf, +-floatmax (the differences
overflow), subnormals with odd significands, +-0.0, one value, and the
integers 0..3 (heavy ties)."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits
from mad_ref import MAD_CONSTANT, mad_ref, median_ref

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NPLANT = 10


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
    M[some((n - 1) // 2), next(j)] = np.inf  # a minority: finite
    M[some(n // 2), next(j)] = np.inf        # half (even n): the median is Inf, Inf - Inf
    M[some(n // 2 + 1), next(j)] = np.inf    # a majority: NaN
    M[:, next(j)] = rng.permutation(np.where(np.arange(n) % 2, FMAX, -FMAX).astype(np.float32))
    M[:, next(j)] = rng.permutation(np.resize(np.float32([FMAX, FMAX, 3e38, 1.0]), n))
    sub = (2 * rng.integers(0, 1 << 22, n) + 1).astype(np.uint32)  # odd significands
    sub |= rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    M[:, next(j)] = sub.view(np.float32)
    M[:, next(j)] = rng.choice(np.float32([0.0, -0.0]), n)
    M[:, next(j)] = np.float32(1234.5)
    M[:, next(j)] = rng.integers(0, 4, n).astype(np.float32)
    return M


def chan_array(F, nco, ni, nt, seed):
    """(F * nco, ni, nt): the blocks along the channels."""
    M = make_blocks(F, nco * ni * nt, seed)
    return np.asfortranarray(M.reshape((F * nco, ni, nt), order="F"))


def time_array(T, nc, ni, nb, seed):
    """(nc, ni, T * nb): the blocks along time."""
    M = make_blocks(T, nc * ni * nb, seed).reshape((T, nb, nc, ni), order="F")
    return np.asfortranarray(np.transpose(M, (2, 3, 1, 0)).reshape((nc, ni, nb * T)))


def check_planted(want):
    """The planted blocks did what they are there for."""
    w = want.ravel()
    assert np.isnan(w).sum() >= 2 and (w == 0).sum() >= 2 and not np.signbit(w[w == 0]).any()


def test_restatement_on_planted_blocks():
    for n in (2, 5, 8):
        a = chan_array(n, NPLANT, 1, 1, n)
        want = mad_ref(a, n)
        check_planted(want)
        t = time_array(n, 2, 1, 5, n)
        check_planted(mad_ref(t, n, axis=2))
        assert same_bits(np.sort(mad_ref(t, n, axis=2).ravel()), np.sort(want.ravel()))


# ---------------------------------------------------------------------------
# the channel axis, every form

SORT_F = [2, 3, 4, 5, 7, 8, 16, 33, 63, 64]
SELECT_F = [65, 68, 100, 1024, 4095, 4096]
STREAM_F = [4097, 4100, 8192]
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
def test_fqav_mad_bits(eng, F):
    _, nco, ni, nt = chan_shape(F)
    a = chan_array(F, nco, ni, nt, F)
    x = put(eng, a)
    plan = eng.plan(x, F, 1, "mad")
    assert plan["path"] == PATH_OF[F] and plan == eng.plan(x, F, 1, "median")
    assert plan["float4_per_lane"] == (1 if F % 4 == 0 else 0)
    for w in chan_windows(F, nco):
        got = eng.fb_to_numpy(eng.reduce(x, F, 1, "mad", w))
        want = mad_ref(a, F, w)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert same_bits(got, want), (F, w)
        if w is None:
            check_planted(want)


# ---------------------------------------------------------------------------
# the time axis, both forms

REGS_T = [2, 3, 16, 31, 32]
SPLIT_T = [33, 34, 64, 100, 1024]


def time_shape(T, nc):
    return T, nc, 2, max(8, min(128, 8192 // T))


@pytest.mark.parametrize("T", REGS_T + SPLIT_T)
def test_tav_mad_bits(eng, pkg, T):
    import torch

    path = "regs_median" if T <= 32 else "split_median"
    passes = 2 if T <= 32 else (8 if T % 2 else 10)
    for nc in (8, 6):  # float4 columns, and one dword per lane
        _, _, ni, nb = time_shape(T, nc)
        a = time_array(T, nc, ni, nb, 100 * T + nc)
        x = put(eng, a)
        plan = eng.tstat_plan(x, T, "mad")
        assert plan["path"] == path and plan["passes"] == passes, (T, nc, plan)
        assert plan["channels_per_lane"] == (4 if nc == 8 else 1)
        med = eng.tstat_plan(x, T, "median")
        assert {**plan, "passes": med["passes"]} == med  # the median's plan but for the passes
        want = mad_ref(a, T, axis=2)
        got = eng.fb_to_numpy(eng.tstat(x, T, "mad"))
        assert got.dtype == np.float32 and same_bits(got, want), (T, nc)
        check_planted(want)
        # a window: channels reversed (dword loads), the spectra of half the blocks from the second
        w = [nc - 1, nc, -1, 0, ni, 1, T, T * (nb // 2), 1]
        assert same_bits(eng.fb_to_numpy(eng.tstat(x, T, "mad", w)), mad_ref(a, T, w, axis=2))
        # a strided out: the middle slot of a three-bank product
        big = eng.fb_empty(3 * nc, ni, nb, device="cuda:0")
        big.fill_(-7.0)
        r = eng.tstat(x, T, "mad", out=big[nc:2 * nc])
        torch.cuda.synchronize()
        h = eng.fb_to_numpy(big)
        assert same_bits(h[nc:2 * nc], want) and (h[:nc] == -7.0).all() and (h[2 * nc:] == -7.0).all()
        assert r.data_ptr() == big[nc:2 * nc].data_ptr()
        # a band of three banks
        banks = [a, time_array(T, nc, ni, nb, 100 * T + nc + 1), a[::-1].copy(order="F")]
        band = eng.fb_to_numpy(eng.band_tstat([put(eng, b) for b in banks], T, "mad"))
        assert same_bits(band, np.concatenate([mad_ref(b, T, axis=2) for b in banks], axis=0))
        # two stages: fqavfunc "sum", then tavfunc "mad" of its result on the device
        s1 = eng.fb_to_numpy(eng.reduce(x, 2, 1, "sum"))
        r = pkg.worker.getdata(x, fqavby=2, fqavfunc="sum", tavby=T, tavfunc="mad")
        assert isinstance(r, torch.Tensor) and r.is_cuda
        assert same_bits(eng.fb_to_numpy(r), mad_ref(s1, T, axis=2)), (T, nc)


# ---------------------------------------------------------------------------
# the rule's special cases, and fqav's n <= 1

def test_special_cases_and_copy(eng, pkg):
    inf = np.inf
    rows = np.float32([[1, 2, inf, 4], [inf, inf, inf, 1], [0.0, -0.0, -0.0, 0.0], [7.5] * 4,
                       [1, 2, 4, 7], [-FMAX, FMAX, FMAX, -FMAX]])
    a = np.asfortranarray(rows.reshape((24, 1, 1)))
    t = np.asfortranarray(rows.reshape((6, 1, 4)))
    for got in (eng.fb_to_numpy(eng.reduce(put(eng, a), 4, 1, "mad"))[:, 0, 0],
                eng.fb_to_numpy(eng.tstat(put(eng, t), 4, "mad"))[:, 0, 0]):
        assert got[0] == np.float32(1.5 * MAD_CONSTANT) and np.isnan(got[1])
        assert got[2] == 0 and not np.signbit(got[2]) and got[3] == 0 and not np.signbit(got[3])
        assert got[4] == np.float32(1.5 * MAD_CONSTANT)  # c = 3, d = 2, 1, 1, 4
        assert got[5] == np.inf  # c = 0, d = floatmax: the product is beyond Float32
    assert same_bits(eng.fb_to_numpy(eng.reduce(put(eng, a), 4, 1, "mad")), mad_ref(a, 4))
    # fqav(A, n <= 1) is A whatever f is: the ABI copies the window
    x = put(eng, a)
    assert same_bits(eng.fb_to_numpy(eng.reduce(x, 1, 1, "mad")), a)
    for n in (1, 0):  # (the tstat copy is the reduce's F = T = 1 sum for every op: values)
        assert np.array_equal(eng.fb_to_numpy(eng.tstat(put(eng, t), n, "mad")), t)
        assert same_bits(eng.fb_to_numpy(eng.tstat(put(eng, t), n, "mad")),
                         eng.fb_to_numpy(eng.tstat(put(eng, t), n, "median")))
    assert eng.tstat_plan(x, 1, "mad")["path"] == "copy"
    assert pkg.fqav(x, 1, "mad") is x
    with pytest.raises(TypeError, match="tavby"):
        eng.reduce(x, 4, 2, "mad")
    with pytest.raises(TypeError):
        eng.band_reduce_multi([x, x], 4, 1, "mad")


# ---------------------------------------------------------------------------
# two exact properties

PROP = [("F", 64), ("F", 100), ("F", 4100), ("T", 16), ("T", 100)]


def prop_data(axis, n):
    rng = np.random.default_rng(n)
    shape = (n * 6, 2, 3) if axis == "F" else (8, 2, n * 6)
    return np.asfortranarray(rng.gamma(2.0, 5e8, shape).astype(np.float32))


def run(eng, axis, a, n, op="mad"):
    x = put(eng, a)
    return eng.fb_to_numpy(eng.reduce(x, n, 1, op) if axis == "F" else eng.tstat(x, n, op))


@pytest.mark.parametrize("axis,n", PROP)
def test_power_of_two_scaling_is_exact(eng, axis, n):
    """mad(2^k x) == 2^k mad(x): every step commutes with an exact scaling
    (gamma(2, 5e8) data are ~2^30, so k in -100 .. 90 stays normal)."""
    a = prop_data(axis, n)
    base = run(eng, axis, a, n)
    assert same_bits(base, mad_ref(a, n, axis=0 if axis == "F" else 2)) and (base > 0).all()
    for k in (-100, -7, 1, 30, 90):
        scaled = np.asfortranarray(np.ldexp(a, k))
        assert np.isfinite(scaled).all() and (scaled >= np.finfo(np.float32).tiny).all()
        assert same_bits(run(eng, axis, scaled, n), np.ldexp(base, k)), (axis, n, k)


@pytest.mark.parametrize("axis,n", PROP)
def test_permuting_a_block_changes_nothing(eng, axis, n):
    ax = 0 if axis == "F" else 2
    a = chan_array(n, 6, 2, 3, n) if axis == "F" else time_array(n, 8, 2, 6, n)
    base = run(eng, axis, a, n)
    assert same_bits(base, mad_ref(a, n, axis=ax))
    rng = np.random.default_rng(n + 1)
    for _ in range(2):
        idx = (np.arange(a.shape[ax]) // n) * n + np.tile(rng.permutation(n), a.shape[ax] // n)
        assert same_bits(run(eng, axis, np.asfortranarray(np.take(a, idx, axis=ax)), n), base)


@pytest.mark.parametrize("axis,n", PROP + [("F", 4), ("T", 1024)])
def test_median_is_untouched(eng, axis, n):
    """The kernels are the median's with a flag: median gives the same bits
    before and after a mad call on the same tensor, and they are Julia's."""
    ax = 0 if axis == "F" else 2
    a = chan_array(n, 6, 2, 3, n + 7) if axis == "F" else time_array(n, 8, 2, 6, n + 7)
    x = put(eng, a)

    def call(op):
        return eng.fb_to_numpy(eng.reduce(x, n, 1, op) if axis == "F" else eng.tstat(x, n, op))

    before = call("median")
    mad = call("mad")
    after = call("median")
    assert same_bits(before, after) and same_bits(before, median_ref(a, n, axis=ax))
    assert same_bits(mad, mad_ref(a, n, axis=ax))
    assert same_bits(eng.fb_to_numpy(x), a)  # the input is read only


# ---------------------------------------------------------------------------
# layers

def test_engine_layers(eng, pkg):
    import torch

    banks = [chan_array(64, 16, 2, 3, 20 + k) for k in range(3)]
    xs = [put(eng, b) for b in banks]
    for F in (64, 256):
        want = [mad_ref(b, F) for b in banks]
        band = eng.fb_to_numpy(eng.band_reduce(xs, F, 1, "mad"))
        assert same_bits(band, np.concatenate(want, axis=0)), F
        p = eng.PreparedBandReduce(xs, F, 1, "mad")
        p.launch()
        assert same_bits(eng.fb_to_numpy(p.out), band)
        p.close()
        p = eng.PreparedReduce(xs[1], F, 1, "mad")
        for _ in range(2):
            p.out.zero_()
            p.launch()
            assert same_bits(eng.fb_to_numpy(p.out), want[1])
        e0, e1 = pkg._lib.HipEvent(timing=True), pkg._lib.HipEvent(timing=True)
        p.out.zero_()
        p.launch_timed(None, e0, e1)
        torch.cuda.synchronize()
        assert e0.elapsed_time(e1) >= 0 and same_bits(eng.fb_to_numpy(p.out), want[1])
        p.close()
        # a pageable host array through the GPU, and fqav on both kinds
        assert same_bits(eng.reduce_host(banks[0], F, 1, "mad"), want[0])
        assert same_bits(pkg.fqav(banks[0], F, "mad"), want[0])
        r = pkg.fqav(xs[0], F, "mad")
        assert isinstance(r, torch.Tensor) and r.is_cuda and same_bits(eng.fb_to_numpy(r), want[0])
    win = [5, 512, 1, 1, 1, 1, 0, 2, 2]
    assert same_bits(eng.reduce_host(banks[0], 64, 1, "mad", win), mad_ref(banks[0], 64, win))
    t = time_array(48, 12, 2, 4, 9)
    for T in (16, 48):
        assert same_bits(eng.tstat_host(t, T, "mad"), mad_ref(t, T, axis=2)), T
    win = [1, 8, 1, 1, 1, 1, 191, 96, -2]  # a reversed time range
    assert same_bits(eng.tstat_host(t, 16, "mad", win), mad_ref(t, 16, win, axis=2))
    with pytest.raises(TypeError, match="Float32"):
        eng.reduce(xs[0].to(torch.int16), 4, 1, "mad")


def test_getdata_files_and_getband(eng, pkg, orc, tmp_path):
    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
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
        got = W.getdata(src, fqavby=8, fqavfunc="mad")
        assert got.dtype == np.float32 and same_bits(got, mad_ref(data, 8)), src
        assert same_bits(W.getdata(src, idxs, 16, "mad"), mad_ref(data, 16, win)), src
        assert same_bits(W.getdata(src, tavby=8, tavfunc="mad"), mad_ref(data, 8, axis=2)), src
        assert same_bits(W.getdata(src, idxs, tavby=16, tavfunc="mad"),
                         mad_ref(data, 16, win, axis=2)), src
        with pytest.raises(TypeError, match="tavby"):
            W.getdata(src, fqavby=8, fqavfunc="mad", tavby=2)
    want = mad_ref(data, 8)
    band = pkg.GBT.getband([0, 0], [fil, raw], fqavby=8, fqavfunc="mad")
    assert same_bits(band, np.concatenate([want, want], axis=0))
    staged = pkg.GBT.getband([0, 0], [fil, bs], fqavby=8, fqavfunc="mad", staged=True)
    assert same_bits(staged, np.concatenate([want, want], axis=0))
    s1 = eng.fb_to_numpy(eng.reduce(put(eng, data), 4, 1, "max"))
    tw = mad_ref(s1, 8, axis=2)
    band = pkg.GBT.getband([0, 0], [fil, bs], fqavby=4, fqavfunc="max", tavby=8, tavfunc="mad")
    assert same_bits(band, np.concatenate([tw, tw], axis=0))
    parts = pkg.GBT.getdata([0, 0], [fil, bs], fqavby=8, fqavfunc="mad")
    assert all(same_bits(p, want) for p in parts)
    # the device path keeps the product on the GPU
    r = W.getdata_device(fil, fqavby=8, fqavfunc="mad")
    assert same_bits(eng.fb_to_numpy(r), want)
