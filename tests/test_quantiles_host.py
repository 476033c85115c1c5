"""CPU: the host side of fqavfunc / tavfunc quantiles(ps) -- the maker and its
refusals, the pure host entry points of the bldp_quantiles_* family (shape,
plan with the counts of distinct ranks and of reads; every refusal, without a
GPU), and the Python layer on NumPy arrays of the element types the GPU kernels
do not take.  Every plane is compared bit for bit with the single-p form."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, same_bits
from quantile_ref import quantile_ref, rank_weight

MEDIAN = 6
INF = np.inf
QUARTILES = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def darr(ps):
    return (ctypes.c_double * max(len(ps), 1))(*ps)


def n_ranks(n, ps):
    """Distinct 0-based ranks {j - 1, j} over ps, and distinct lower ranks."""
    lows = {rank_weight(n, p)[0] - 1 for p in ps}
    return len(lows | {q + 1 for q in lows}), len(lows)


# ---------------------------------------------------------------------------
# the maker

def test_maker_and_validation(pkg):
    assert pkg.quantiles([0.25, 0.5]) == ("quantiles", (0.25, 0.5))
    assert pkg.quantiles((1, 0, 1)) == ("quantiles", (1.0, 0.0, 1.0))  # unsorted, repeated
    assert pkg.quantiles(np.float32([0.5])) == ("quantiles", (0.5,))
    assert all(isinstance(p, float) for p in pkg.quantiles(np.float32([0.5, 0.25]))[1])
    assert pkg.quantiles(p for p in (0.1, 0.9)) == ("quantiles", (0.1, 0.9))
    assert len(pkg.quantiles(np.linspace(0, 1, 9))[1]) == 9  # the C limit is not the user's
    for bad in ([], (), [0.5, float("nan")], [0.5, 1.5], [-0.1], 0.5, None, ["x"], [None]):
        with pytest.raises(ValueError, match="quantile"):
            pkg.quantiles(bad)
    E = pkg._lib
    assert E.quantiles_of(("quantiles", (0.25, 0.5))) == (0.25, 0.5)
    assert E.quantiles_of(("quantiles", [1])) == (1.0,)
    assert E.quantiles_of(("quantile", 0.5)) is None and E.quantiles_of("median") is None
    assert E.quantiles_of(("quantiles",)) is None
    with pytest.raises(ValueError):
        E.quantiles_of(("quantiles", (0.5, 2.0)))
    with pytest.raises(ValueError):
        E.quantiles_of(("quantiles", ()))
    assert E.stat_op(pkg.quantiles([0.5])) and E.stat_op(pkg.quantile(0.5)) and E.stat_op("mad")
    assert not E.stat_op("sum") and not E.stat_op(("median", 0.5))
    # quantile() itself stays exactly as it is
    assert pkg.quantile(0.25) == ("quantile", 0.25) and pkg.quantile(1) == ("quantile", 1.0)
    assert E.quantile_of(("quantile", 0.5)) == 0.5 and E.quantile_of(pkg.quantiles([0.5])) is None
    with pytest.raises(ValueError, match="quantile"):
        pkg.quantile([0.5])
    assert "quantiles" not in E.OPS and E.MAX_QUANTILES == 8
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    assert re.search(r"#define BLDP_MAX_QUANTILES 8\b", hdr)
    assert pkg.engine.out_dtype(np.dtype(np.float32), pkg.quantiles([0.5])) == np.float32
    assert pkg.engine.out_dtype(np.dtype(np.uint8), pkg.quantiles([0.5])) == np.float64


# ---------------------------------------------------------------------------
# the host-only C calls

def qshape(L, dims, axis, n, k, win=None):
    out = (ctypes.c_int64 * 4)()
    w = (ctypes.c_int64 * 9)(*win) if win else None
    rc = L.bldp_quantiles_shape(*dims, ctypes.cast(w, ctypes.c_void_p) if w else None, axis, n, k,
                                out)
    return rc, list(out)


def qplan(L, dims, axis, n, ps, win=None):
    info = (ctypes.c_int64 * 10)()
    w = (ctypes.c_int64 * 9)(*win) if win else None
    rc = L.bldp_quantiles_plan_f32(None, *dims, ctypes.cast(w, ctypes.c_void_p) if w else None,
                                   axis, n, len(ps), darr(ps), None, info)
    return rc, list(info)


def test_shape(pkg, L):
    E = pkg._lib
    assert qshape(L, (64, 2, 12), 0, 8, 3) == (E.BLDP_OK, [8, 2, 12, 3])
    assert qshape(L, (64, 2, 12), 2, 4, 8) == (E.BLDP_OK, [64, 2, 3, 8])
    assert qshape(L, (64, 2, 12), 0, 1, 1) == (E.BLDP_OK, [64, 2, 12, 1])
    assert qshape(L, (64, 2, 12), 2, 0, 2) == (E.BLDP_OK, [64, 2, 12, 2])
    assert qshape(L, (64, 2, 12), 0, 8, 2, [4, 32, 1, 1, 1, 1, 11, 6, -2]) == \
        (E.BLDP_OK, [4, 1, 6, 2])
    assert qshape(L, (64, 2, 12), 0, 5, 2)[0] == E.BLDP_EDIM
    assert qshape(L, (64, 2, 12), 2, 5, 2)[0] == E.BLDP_EDIM
    assert qshape(L, (64, 2, 12), 0, 8, 2, [60, 8, 1, 0, 2, 1, 0, 12, 1])[0] == E.BLDP_EBOUNDS
    assert qshape(L, (64, 2, 12), 1, 4, 2)[0] == E.BLDP_EINVAL and "axis" in E.last_error()
    for k in (0, 9, -1):
        assert qshape(L, (64, 2, 12), 0, 8, k)[0] == E.BLDP_EINVAL and "np=" in E.last_error()
    assert L.bldp_quantiles_shape(64, 2, 12, None, 0, 8, 2, None) == E.BLDP_EINVAL


def test_rank_counts(pkg, L):
    E = pkg._lib
    rc, q = qplan(L, (64, 1, 4), 0, 8, (0.5, 0.5))
    assert rc == E.BLDP_OK and q[8] == 2, E.last_error()
    assert qplan(L, (64, 1, 4), 0, 2, (0.0, 1.0))[1][8] == 2   # both clamps on n = 2: ranks 0, 1
    assert qplan(L, (64, 1, 4), 2, 2, (0.0, 1.0))[1][8] == 2
    # adjacent pairs sharing a key: n = 5, p = 0.25 takes ranks 1, 2 and p = 0.5 ranks 2, 3
    assert (rank_weight(5, 0.25)[0], rank_weight(5, 0.5)[0]) == (2, 3)
    assert qplan(L, (65, 1, 4), 0, 5, (0.25, 0.5))[1][8] == 3
    assert qplan(L, (65, 1, 4), 0, 5, (0.5, 0.25, 0.5))[1][8] == 3  # order and repeats: no matter
    # the same ranks with two weights
    assert rank_weight(100, 0.251)[0] == rank_weight(100, 0.2515)[0]
    assert qplan(L, (200, 1, 4), 0, 100, (0.251, 0.2515))[1][8] == 2
    for n in (2, 5, 64, 100, 4100):
        for ps in (QUARTILES, (0.9, 0.1), (0.0, 1.0), tuple(np.linspace(0, 1, 8)), (1 / 3,)):
            assert qplan(L, (2 * n, 1, 2), 0, n, ps)[1][8] == n_ranks(n, ps)[0], (n, ps)
            assert qplan(L, (6, 1, 2 * n), 2, n, ps)[1][8] == n_ranks(n, ps)[0], (n, ps)


def test_plans_are_the_medians(pkg, L):
    E, P, TP = pkg._lib, pkg._lib.PATHS, pkg._lib.TSTAT_PATHS
    med = (ctypes.c_int64 * 8)()
    for F, path, reads in ((2, "median_sort", 1), (64, "median_sort", 1),
                           (65, "median_select", 1), (4096, "median_select", 1),
                           (4097, "median_stream", 4)):
        dims = (2 * F, 2, 3)
        for ps in (QUARTILES, (0.3,), tuple(np.linspace(0, 1, 8))):
            rc, q = qplan(L, dims, 0, F, ps)
            assert rc == E.BLDP_OK, E.last_error()
            assert L.bldp_reduce_plan_f32(None, *dims, None, F, 1, MEDIAN, None, med) == E.BLDP_OK
            assert P[q[0]] == path and q[:8] == list(med), (F, ps)
            assert q[9] == reads, (F, ps)  # four reads for any K on the stream form
    rc, q = qplan(L, (64, 2, 3), 0, 1, QUARTILES)  # the copy of n <= 1, as the median's
    assert L.bldp_reduce_plan_f32(None, 64, 2, 3, None, 1, 1, MEDIAN, None, med) == E.BLDP_OK
    assert rc == E.BLDP_OK and q[:8] == list(med) and q[8:] == [0, 1]
    # the time axis, in registers: the median's plan, one read
    for T in (2, 5, 32):
        for nc in (264, 6):
            dims = (nc, 2, 2 * T)
            rc, q = qplan(L, dims, 2, T, QUARTILES)
            assert rc == E.BLDP_OK, E.last_error()
            assert L.bldp_tstat_plan_f32(None, *dims, None, T, MEDIAN, None, med) == E.BLDP_OK
            assert TP[q[0]] == "regs_median" and q[:8] == list(med) and q[9] == 1, (T, nc)
    # the split form: one lower rank keeps the quantile's tile (32 columns) and its
    # 5 reads; more take 16 columns and 1 + 4 ceil(L / 3) reads
    single = (ctypes.c_int64 * 8)()
    for T in (33, 100, 1024):
        for nc, cpl in ((264, 4), (6, 1)):
            dims = (nc, 2, 2 * T)
            assert L.bldp_quantile_plan_f32(None, *dims, None, 2, T, 0.3, None, single) == E.BLDP_OK
            s = list(single)
            rc, q = qplan(L, dims, 2, T, (0.3,))
            assert rc == E.BLDP_OK and TP[q[0]] == "split_median"
            assert q[:5] + q[6:8] == s[:5] + s[6:8] and q[5] == 0 and q[8:] == [2, 5], (T, nc)
            for ps in (QUARTILES, (0.9, 0.1), tuple(np.linspace(0.1, 0.9, 8)), (0.5, 0.5)):
                nr, nlow = n_ranks(T, ps)
                rc, q = qplan(L, dims, 2, T, ps)
                assert rc == E.BLDP_OK and TP[q[0]] == "split_median" and q[1] == cpl
                want = 1 + 4 * -(-nlow // 3)
                assert q[3] == q[9] == want and q[8] == nr, (T, nc, ps)
                assert want < 5 * len(set(ps)) or len(set(ps)) == 1  # fewer than separate calls
                if nlow == 1:
                    assert q[:8] == s[:5] + [0] + s[6:8]
                else:
                    lanes = min(16 // cpl, 1 << (-(-nc // cpl) - 1).bit_length())
                    assert q[7] == lanes and q[2] == 256 // lanes, (T, nc, ps)
                    assert q[4] == -(-(nc // cpl) // lanes) * 2 * 2 and q[6] == 2
    rc, q = qplan(L, (264, 2, 8), 2, 1, QUARTILES)
    assert rc == E.BLDP_OK and q[0] == -1 and q[8:] == [0, 1]  # the copy
    # the read counts the header states, L = 1 .. 8
    assert [1 + 4 * -(-l // 3) for l in range(1, 9)] == [5, 5, 5, 9, 9, 9, 13, 13]
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    assert "5, 5, 5, 9," in hdr and "9, 9, 13, 13" in hdr


def test_every_refusal_without_a_gpu(pkg, L):
    E = pkg._lib
    nan = float("nan")
    info = (ctypes.c_int64 * 10)()
    ptrs = (ctypes.c_void_p * 2)(0, 0)
    banks = ctypes.cast(ptrs, ctypes.c_void_p)

    def entries(axis, n, ps, k=None, win=None):
        """Every entry point that takes p[], on null data."""
        k = len(ps) if k is None else k
        p = darr(ps)
        return [L.bldp_quantiles_plan_f32(None, 64, 2, 12, win, axis, n, k, p, None, info),
                L.bldp_quantiles_f32(None, 64, 2, 12, win, axis, n, k, p, None, 64, 128, 2048,
                                     None),
                L.bldp_band_quantiles_f32(2, banks, 64, 2, 12, win, axis, n, k, p, None, None),
                L.bldp_quantiles_host_f32(0, None, 64, 2, 12, win, axis, n, k, p, None)]

    for axis in (0, 2):
        for k in (0, 9, -3):  # np 0 and 9
            for rc in entries(axis, 4, (0.5,) * 9, k):
                assert rc == E.BLDP_EINVAL and "np=" in E.last_error(), (axis, k)
        for bad in (1.5, nan, -1e-300, INF):  # a bad p at index > 0
            for ps in ((0.5, bad), (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, bad)):
                for rc in entries(axis, 4, ps):
                    assert rc == E.BLDP_EINVAL and "[0, 1]" in E.last_error(), (axis, ps)
                assert "p[%d]" % (len(ps) - 1) in E.last_error()
    for axis in (1, 3, -1):
        for rc in entries(axis, 4, QUARTILES):
            assert rc == E.BLDP_EINVAL and "axis" in E.last_error(), axis
    for rc in (L.bldp_quantiles_plan_f32(None, 64, 2, 12, None, 0, 4, 2, None, None, info),
               L.bldp_quantiles_f32(None, 64, 2, 12, None, 0, 4, 2, None, None, 64, 128, 2048,
                                    None)):
        assert rc == E.BLDP_EINVAL and "null p" in E.last_error()
    # good (axis, np, p[]) pass those checks: the divisibility and window checks come next
    for axis in (0, 2):
        for rc in entries(axis, 5, QUARTILES):  # n not dividing the axis
            assert rc == E.BLDP_EDIM, axis
    w = (ctypes.c_int64 * 9)(60, 8, 1, 0, 2, 1, 0, 12, 1)  # a window out of bounds
    for axis in (0, 2):
        for rc in entries(axis, 4, QUARTILES, win=ctypes.cast(w, ctypes.c_void_p)):
            assert rc == E.BLDP_EBOUNDS, axis
    # ... then the null pointers (the plan takes them)
    rcs = entries(0, 4, QUARTILES) + entries(2, 4, QUARTILES)
    assert rcs[0] == rcs[4] == E.BLDP_OK
    assert [r for k, r in enumerate(rcs) if k % 4] == [E.BLDP_EINVAL] * 6
    assert "null" in E.last_error()
    # planes that overlap
    x = ctypes.c_void_p(16)  # (never dereferenced: the check comes before any launch)
    assert L.bldp_quantiles_f32(x, 64, 2, 12, None, 0, 4, 2, darr((0.1, 0.9)), x, 16, 32, 100,
                                None) == E.BLDP_EINVAL and "overlap" in E.last_error()
    assert L.bldp_quantiles_plan_f32(None, 64, 2, 12, None, 0, 4, 2, darr((0.1, 0.9)), None,
                                     None) == E.BLDP_EINVAL
    assert L.bldp_band_quantiles_f32(0, banks, 64, 2, 12, None, 2, 4, 1, darr((0.5,)), None,
                                     None) == E.BLDP_EINVAL
    # the internal op codes stay invalid for callers
    for op in (64, 65):
        assert L.bldp_reduce_plan_f32(None, 64, 1, 4, None, 4, 1, op, None, info) == E.BLDP_EINVAL
        assert L.bldp_tstat_plan_f32(None, 64, 1, 4, None, 2, op, None, info) == E.BLDP_EINVAL
    assert L.bldp_abi_version() == 5


# ---------------------------------------------------------------------------
# the Python layer on NumPy arrays

def planes_match(got, a, n, ps, axis=0, win=None, dtype=np.float64):
    assert got.dtype == dtype and got.ndim == 4 and got.shape[3] == len(ps)
    assert got.flags.f_contiguous
    for k, p in enumerate(ps):
        want = quantile_ref(a, n, p, win, axis)
        assert got[..., k].shape == want.shape and same_bits(got[..., k], want), (n, k, p, axis)
    return True


def test_other_element_types_are_float64_from_the_host(pkg, tmp_path):
    W = pkg.worker
    rng = np.random.default_rng(3)
    u8 = np.asfortranarray(rng.integers(0, 4, (24, 2, 6)).astype(np.uint8))  # heavy ties
    i16 = np.asfortranarray(rng.integers(-300, 300, (24, 2, 6)).astype(np.int16))
    f64 = np.asfortranarray(rng.standard_normal((24, 2, 6)))
    f64[5, 0, 0] = np.nan
    f64[8:12, 1, 2] = [INF, INF, INF, 1.0]
    f64[12:16, 1, 2] = [1.0, 2.0, -INF, 4.0]
    f64[16:20, 1, 2] = [-0.0, 0.0, -0.0, 0.0]
    sets = (QUARTILES, (0.9, 0.1), (0.5, 0.5), (0.0, 1.0), (1 / 3,), tuple(np.linspace(0, 1, 9)))
    for a in (u8, i16, f64):
        for ps in sets:
            q = pkg.quantiles(ps)
            for n in (2, 3, 4, 24):
                got = W._host_stat(a, n, q)
                assert planes_match(got, a, n, ps)
                # each plane is the existing single-p result
                for k, p in enumerate(ps):
                    assert same_bits(got[..., k], W._host_stat(a, n, ("quantile", p)))
                assert same_bits(pkg.fqav(a, n, q), got)
                assert same_bits(W.getdata(a, fqavby=n, fqavfunc=q), got)
            for n in (2, 3, 6):
                got = W._host_stat(a, n, q, axis=2)
                assert planes_match(got, a, n, ps, axis=2)
                for k, p in enumerate(ps):
                    assert same_bits(got[..., k], W._host_stat(a, n, ("quantile", p), axis=2))
                assert same_bits(W.getdata(a, tavby=n, tavfunc=q), got)
    # NaN wins in every plane
    r = pkg.fqav(f64, 4, pkg.quantiles(QUARTILES))
    assert np.isnan(r[1, 0, 0, :]).all() and not np.isnan(r[0, 0, 0, :]).any()
    # a window goes with it, on both axes; two stages on the host
    J, C = pkg.JRange, pkg.COLON
    q = pkg.quantiles((0.75, 0.25))
    got = W.getdata(i16, (J(24, -1, 1), C, J(2, 5)), 3, q)
    assert planes_match(got, i16, 3, q[1], win=[23, 24, -1, 0, 2, 1, 1, 4, 1])
    got = W.getdata(i16, (J(3, 2, 21), C, J(6, -1, 1)), tavby=3, tavfunc=q)
    assert planes_match(got, i16, 3, q[1], axis=2, win=[2, 10, 2, 0, 2, 1, 5, 6, -1])
    s1 = pkg.fqav(i16, 4, pkg.quantile(0.25))
    got = W.getdata(i16, fqavby=4, fqavfunc=pkg.quantile(0.25), tavby=3, tavfunc=q)
    assert planes_match(got, s1, 3, q[1], axis=2)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.fqav(i16, 5, q)
    # a UInt8 SIGPROC file gives the same
    fil = str(tmp_path / "u8.fil")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=24, nifs=2, tsamp=1.0, nbits=8,
                                    telescope_id=6, machine_id=10, data_type=1, tstart=59000.0,
                                    source_name="X"), u8)
    assert planes_match(W.getdata(fil, fqavby=4, fqavfunc=q), u8, 4, q[1])
    assert planes_match(W.getdata(fil, tavby=3, tavfunc=q), u8, 3, q[1], axis=2)
    parts = pkg.GBT.getdata([0, 0], [fil, fil], fqavby=4, fqavfunc=q)
    assert len(parts) == 2 and all(planes_match(p, u8, 4, q[1]) for p in parts)


def test_n_at_most_one_copies_the_window_into_every_plane(pkg):
    W = pkg.worker
    rng = np.random.default_rng(5)
    u8 = np.asfortranarray(rng.integers(0, 200, (6, 2, 4)).astype(np.uint8))
    i16 = np.asfortranarray(rng.integers(-300, 300, (6, 2, 4)).astype(np.int16))
    f64 = np.asfortranarray(rng.standard_normal((6, 2, 4)))
    q = pkg.quantiles(QUARTILES)
    for a in (u8, i16, f64):
        # the scalar form returns the window in its own type: so does every plane
        assert W.getdata(a, fqavby=1, fqavfunc=pkg.quantile(0.3)).dtype == a.dtype
        for r in (W.getdata(a, fqavby=1, fqavfunc=q), W.getdata(a, tavby=1, tavfunc=q),
                  W.getdata(a, tavby=0, tavfunc=q), pkg.fqav(a, 1, q), pkg.fqav(a, 0, q)):
            assert r.dtype == a.dtype and r.shape == a.shape + (3,) and r.flags.f_contiguous
            assert all(np.array_equal(r[..., k], a) for k in range(3))
        J, C = pkg.JRange, pkg.COLON
        r = W.getdata(a, (J(2, 5), C, J(4, -1, 1)), 1, q)
        assert r.dtype == a.dtype and r.shape == (4, 2, 4, 3)
        assert all(np.array_equal(r[..., k], a[1:5, :, ::-1]) for k in range(3))
        # _host_stat itself copies in Float64, as it does for the scalar form
        r = W._host_stat(a, 1, q)
        assert r.dtype == np.float64 and same_bits(r[..., 2], W._host_stat(a, 1, ("quantile", 0.75)))
    v = np.arange(5, dtype=np.int32)
    assert pkg.fqav(v, 1, pkg.quantiles((0.1, 0.9))).shape == (5, 2)


def test_the_type_errors(pkg):
    W = pkg.worker
    a = np.zeros((8, 1, 4), dtype=np.float32, order="F")
    q = pkg.quantiles(QUARTILES)
    for arr in (a, a.astype(np.int16), a.astype(np.float64)):
        with pytest.raises(TypeError, match="tavby"):
            W.getdata(arr, fqavby=2, fqavfunc=q, tavby=2)
        for tf in ("sum", "median", pkg.quantile(0.5), q):
            with pytest.raises(TypeError, match="tavfunc"):
                W.getdata(arr, fqavby=2, fqavfunc=q, tavby=2, tavfunc=tf)
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata("nothing.fil", fqavby=2, fqavfunc=q, tavfunc="sum")  # before any file is touched
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata_device(a, fqavby=2, fqavfunc=q, tavfunc="sum")
    for kw in (dict(fqavby=2, fqavfunc=q), dict(tavby=2, tavfunc=q),
               dict(fqavby=2, fqavfunc=("quantiles", [0.5]))):
        with pytest.raises(TypeError, match="engine.band_quantiles"):
            pkg.GBT.getband([0], ["nothing.fil"], **kw)
    with pytest.raises(ValueError, match="quantile"):
        pkg.GBT.getband([0], ["nothing.fil"], fqavby=2, fqavfunc=("quantiles", [0.5, 1.5]))
    for bad in (("quantiles", [0.5, 1.5]), ("quantiles", ())):
        for arr in (a, a.astype(np.uint8)):  # (Float32: before any GPU work)
            with pytest.raises(ValueError, match="quantile"):
                pkg.fqav(arr, 2, bad)
            with pytest.raises(ValueError, match="quantile"):
                W.getdata(arr, tavby=2, tavfunc=bad)
    eng = pkg.engine
    with pytest.raises(TypeError):
        eng.quantiles_host(np.zeros((4, 1, 4), np.float64, order="F"), 2, QUARTILES)
    with pytest.raises(pkg._lib.DimensionMismatch):
        eng.quantiles_host(np.zeros((4, 1, 4), np.float32, order="F"), 3, QUARTILES, axis=2)
    with pytest.raises(ValueError, match="axis"):
        eng.quantiles_host(a, 2, QUARTILES, axis=1)
    with pytest.raises(ValueError, match="quantile"):
        eng.quantiles_host(a, 2, [])
    assert eng.quantiles_host(np.zeros((4, 1, 0), np.float32, order="F"), 2,
                              QUARTILES).shape == (2, 1, 0, 3)
    with pytest.raises(TypeError):
        eng.band_reduce_multi([None, None], 4, 1, q)
    with pytest.raises(TypeError, match="quantile"):
        eng._no_quantile(q, "PreparedReduce")


def test_julia_shim_and_docs():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in ("bldp_quantiles_shape", "bldp_quantiles_plan_f32", "bldp_quantiles_f32",
                 "bldp_band_quantiles_f32", "bldp_quantiles_host_f32"):
        assert re.search(r"ccall\(\(:%s, libbldp\)" % name, src), name
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert re.search(r"\bquantiles\b", open(os.path.join(REPO, doc)).read()), doc
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert re.search(r"^#+ .*Quantiles", design, re.M)
