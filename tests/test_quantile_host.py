"""CPU: the host side of fqavfunc / tavfunc ("quantile", p) — the rule restated
in NumPy (quantile_ref.py) against numpy.quantile and on fixed cases, the pure
host entry points of the bldp_quantile_* family (shape, plan: the median's path
for the shape; every refusal, without a GPU), and the Python layer on NumPy
arrays of the element types the GPU kernels do not take."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, same_bits
from quantile_ref import neighbours, quantile_blocks, quantile_ref, rank_weight

MEDIAN = 6
INF = np.inf
FMAX = np.finfo(np.float32).max

NS = (2, 3, 5, 8, 64, 65, 100, 4097)
PS = (0.0, 1.0, 0.5, 0.25, 0.75, 0.1, 0.99, 1 / 3, 1e-300, np.nextafter(1.0, 0.0))


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---------------------------------------------------------------------------
# the restatement

@pytest.mark.parametrize("n", NS)
def test_restatement_against_numpy_quantile(n):
    """Within 2^-22 max(|a|, |b|) of NumPy's Float64 type-7 quantile: the
    Float32 rounding of b - a (<= 2^-24 |b - a| <= 2^-23 max, times g <= 1) plus
    the final rounding to Float32 (<= 2^-24 |r| <= 2^-24 max); NumPy's own
    Float64 error is 2^-29 of that."""
    rng = np.random.default_rng(n)
    R = np.concatenate([rng.gamma(2.0, 5e8, (n, 20)), rng.standard_normal((n, 20)) * 1e3],
                       axis=1).astype(np.float32)
    for p in PS:
        got = quantile_blocks(R, p)
        assert got.dtype == np.float32
        a, b, g = neighbours(R, p)
        want = np.quantile(R.astype(np.float64), p, axis=0)
        bound = 2.0 ** -22 * np.maximum(np.abs(a), np.abs(b)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (n, p, float((err / bound).max()))
        # Float64 blocks: the same steps with a Float64 difference.  The two index
        # formulas (aleph <= n + 1 here, NumPy's p (n - 1)) each round to 2^-52 n,
        # which moves g * (b - a) by <= 2^-51 n * 2 max; a few roundings of r besides
        got64 = quantile_blocks(R.astype(np.float64), p)
        assert got64.dtype == np.float64
        assert (np.abs(got64 - want) <= (n + 2) * 2.0 ** -50 * bound * 2.0 ** 22).all(), (n, p)


def test_rank_and_weight(pkg):
    assert rank_weight(5, 0.25) == (2, 0.0)
    assert rank_weight(5, 0.0) == (1, 0.0) and rank_weight(5, 1.0) == (4, 1.0)
    assert rank_weight(2, 0.5) == (1, 0.5) and rank_weight(4, 0.5) == (2, 0.5)
    assert rank_weight(100, 1e-300) == (1, 0.0)
    j, g = rank_weight(4097, np.nextafter(1.0, 0.0))
    assert j == 4096 and 0.999 < g <= 1.0
    for n in NS:
        for p in PS:
            j, g = rank_weight(n, p)
            assert 1 <= j <= n - 1 and 0.0 <= g <= 1.0
            assert pkg._lib.quantile_rank(n, p) == (j, g), (n, p)  # the package's own copy


def one(v, p, dt=np.float32):
    return quantile_ref(np.array(v, dt).reshape((len(v), 1, 1)), len(v), p)[0, 0, 0]


def test_restatement_fixed_cases():
    got = one([1, 2, 3, 4, 5], 0.25)
    assert got.dtype == np.float32 and got == 2.0
    assert one([5, 3, 1, 4, 2], 0.25) == 2.0 and one([1, 2, 3, 4, 5], 0.25, np.float64) == 2.0
    assert np.isnan(one([1, INF], 0.0))    # g == 0 next to an infinite b: 0 * Inf
    assert np.isnan(one([-INF, 1], 1.0))   # g == 1 next to an infinite a
    assert np.isnan(one([-FMAX, FMAX], 0.0))  # d overflows: 0 * Inf
    assert one([-FMAX, FMAX], 0.5) == INF  # ... and a + g * Inf otherwise: the formula as written
    assert one([-FMAX, FMAX], 0.0, np.float64) == -FMAX  # a Float64 difference does not overflow
    assert np.isnan(one([1, np.nan, 3], 0.5)) and np.isnan(one([np.nan, 1], 0.0))
    assert one([1, INF, 2, 3], 0.5) == 2.5 and one([INF, INF, 1], 0.75) == INF
    assert np.isnan(one([INF, INF, 1], 1.0))  # g == 1 next to an infinite a, again
    # -0.0 sorts before 0.0; the result is -0.0 + g * 0.0 = +0.0 all the same
    lo, hi, _ = neighbours(np.float32([[0.0], [-0.0], [0.0], [-0.0]]), 0.5)
    assert np.signbit(lo[0]) and not np.signbit(hi[0])
    for v in ([0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0]):
        for p in (0.0, 0.5, 1.0):
            z = one(v, p)
            assert z == 0.0 and not np.signbit(z), (v, p)
    assert one([1, 2, 3, 4], 0.5) == 2.5 and one([7.5] * 4, 0.3) == 7.5
    # g == 1 is a + d with d rounded, not b: 2^24 + 1 rounds to 2^24, and 1 + 2^24 again
    assert one([1, 2.0 ** 24 + 2], 1.0) == 2.0 ** 24 and one([1, 2.0 ** 24 + 2], 0.0) == 1.0
    assert one([1, 2.0 ** 24 + 2], 1.0, np.float64) == 2.0 ** 24 + 2
    # n <= 1: the window itself
    a = np.asfortranarray(np.arange(6, dtype=np.float32).reshape((3, 1, 2)))
    assert same_bits(quantile_ref(a, 1, 0.3), a) and same_bits(quantile_ref(a, 0, 0.3, axis=2), a)


# ---------------------------------------------------------------------------
# the host-only C calls

def qshape(L, dims, axis, n, win=None):
    out = (ctypes.c_int64 * 3)()
    w = (ctypes.c_int64 * 9)(*win) if win else None
    rc = L.bldp_quantile_shape(*dims, ctypes.cast(w, ctypes.c_void_p) if w else None, axis, n, out)
    return rc, list(out)


def qplan(L, dims, axis, n, p):
    info = (ctypes.c_int64 * 8)()
    rc = L.bldp_quantile_plan_f32(None, *dims, None, axis, n, p, None, info)
    return rc, list(info)


def test_shape(pkg, L):
    E = pkg._lib
    assert qshape(L, (64, 2, 12), 0, 8) == (E.BLDP_OK, [8, 2, 12])
    assert qshape(L, (64, 2, 12), 2, 4) == (E.BLDP_OK, [64, 2, 3])
    assert qshape(L, (64, 2, 12), 0, 1) == (E.BLDP_OK, [64, 2, 12])
    assert qshape(L, (64, 2, 12), 2, 0) == (E.BLDP_OK, [64, 2, 12])
    assert qshape(L, (64, 2, 12), 0, 8, [4, 32, 1, 1, 1, 1, 11, 6, -2]) == (E.BLDP_OK, [4, 1, 6])
    assert qshape(L, (64, 2, 12), 0, 5)[0] == E.BLDP_EDIM
    assert qshape(L, (64, 2, 12), 2, 5)[0] == E.BLDP_EDIM
    assert qshape(L, (64, 2, 12), 0, 8, [60, 8, 1, 0, 2, 1, 0, 12, 1])[0] == E.BLDP_EBOUNDS
    for axis in (1, 3, -1):
        assert qshape(L, (64, 2, 12), axis, 4)[0] == E.BLDP_EINVAL
        assert "axis" in E.last_error()
    assert L.bldp_quantile_shape(64, 2, 12, None, 0, 8, None) == E.BLDP_EINVAL


def test_plans_are_the_medians(pkg, L):
    E, P, TP = pkg._lib, pkg._lib.PATHS, pkg._lib.TSTAT_PATHS
    med = (ctypes.c_int64 * 8)()
    for F, path in ((2, "median_sort"), (64, "median_sort"), (65, "median_select"),
                    (4096, "median_select"), (4097, "median_stream")):
        dims = (2 * F, 2, 3)
        for p in (0.0, 0.25, 1.0):
            rc, q = qplan(L, dims, 0, F, p)
            assert rc == E.BLDP_OK, E.last_error()
            assert L.bldp_reduce_plan_f32(None, *dims, None, F, 1, MEDIAN, None, med) == E.BLDP_OK
            m = list(med)
            assert P[q[0]] == path and q[0] == m[0], (F, p)
            assert m[6] == 0 and q[:6] + q[7:] == m[:6] + m[7:]  # but for the rank's slot
            assert q[6] == rank_weight(F, p)[0] - 1, (F, p)
    rc, q = qplan(L, (64, 2, 3), 0, 1, 0.25)  # the copy of n <= 1, as the median's
    assert L.bldp_reduce_plan_f32(None, 64, 2, 3, None, 1, 1, MEDIAN, None, med) == E.BLDP_OK
    assert rc == E.BLDP_OK and q[6] == -1 and q[:6] + q[7:] == list(med)[:6] + list(med)[7:]
    # the time axis: the median's path; the split form always makes its fifth pass
    for T, path, passes in ((2, "regs_median", 1), (32, "regs_median", 1),
                            (33, "split_median", 5), (34, "split_median", 5),
                            (1024, "split_median", 5)):
        for nc in (264, 6):
            dims = (nc, 2, 2 * T)
            for p in (0.0, 0.9, 1.0):
                rc, q = qplan(L, dims, 2, T, p)
                assert rc == E.BLDP_OK, E.last_error()
                assert L.bldp_tstat_plan_f32(None, *dims, None, T, MEDIAN, None, med) == E.BLDP_OK
                m = list(med)
                assert TP[q[0]] == path and q[0] == m[0] and q[3] == passes, (T, nc, p)
                assert m[3] == (passes if T <= 32 or T % 2 == 0 else 4) and m[5] == 0
                assert q[:3] + [q[4]] + q[6:] == m[:3] + [m[4]] + m[6:]
                assert q[5] == rank_weight(T, p)[0] - 1, (T, p)
    rc, q = qplan(L, (264, 2, 8), 2, 1, 0.5)
    assert rc == E.BLDP_OK and q[0] == -1 and q[5] == -1  # the copy


def test_every_refusal_without_a_gpu(pkg, L):
    E = pkg._lib
    nan = float("nan")
    info = (ctypes.c_int64 * 8)()
    ptrs = (ctypes.c_void_p * 2)(0, 0)
    banks = ctypes.cast(ptrs, ctypes.c_void_p)

    def entries(axis, n, p):
        """Every entry point that takes p, on null data."""
        return [L.bldp_quantile_plan_f32(None, 64, 2, 12, None, axis, n, p, None, info),
                L.bldp_quantile_f32(None, 64, 2, 12, None, axis, n, p, None, 64, 128, None),
                L.bldp_band_quantile_f32(2, banks, 64, 2, 12, None, axis, n, p, None, None),
                L.bldp_quantile_host_f32(0, None, 64, 2, 12, None, axis, n, p, None)]

    for p in (-1e-300, np.nextafter(1.0, 2.0), 2.0, -1.0, INF, -INF, nan):
        for axis in (0, 2):
            for rc in entries(axis, 4, p):
                assert rc == E.BLDP_EINVAL and "[0, 1]" in E.last_error(), (axis, p)
    for axis in (1, 3, -1):
        for rc in entries(axis, 4, 0.5):
            assert rc == E.BLDP_EINVAL and "axis" in E.last_error(), axis
    # a good (axis, p) passes those checks: the divisibility and window checks come next
    for axis, n in ((0, 5), (2, 5)):
        for rc in entries(axis, n, 0.5):
            assert rc == E.BLDP_EDIM, (axis, n)
    w = (ctypes.c_int64 * 9)(60, 8, 1, 0, 2, 1, 0, 12, 1)
    wp = ctypes.cast(w, ctypes.c_void_p)
    assert L.bldp_quantile_plan_f32(None, 64, 2, 12, wp, 0, 4, 0.5, None, info) == E.BLDP_EBOUNDS
    assert L.bldp_quantile_f32(None, 64, 2, 12, wp, 2, 4, 0.5, None, 8, 16, None) == E.BLDP_EBOUNDS
    # ... then the null pointers (the plan takes them)
    rcs = entries(0, 4, 0.5) + entries(2, 4, 0.5)
    assert rcs[0] == rcs[4] == E.BLDP_OK
    assert [r for k, r in enumerate(rcs) if k % 4] == [E.BLDP_EINVAL] * 6
    assert "null" in E.last_error()
    assert L.bldp_quantile_plan_f32(None, 64, 2, 12, None, 0, 4, 0.5, None, None) == E.BLDP_EINVAL
    assert L.bldp_band_quantile_f32(0, banks, 64, 2, 12, None, 2, 4, 0.5, None, None) == E.BLDP_EINVAL
    # quantile is no op of the ABI: the codes next to mad's stay invalid
    for op in (7, 9, 64):
        assert L.bldp_reduce_plan_f32(None, 64, 1, 4, None, 4, 1, op, None, info) == E.BLDP_EINVAL
        assert "unknown op" in E.last_error()
        assert L.bldp_tstat_plan_f32(None, 64, 1, 4, None, 2, op, None, info) == E.BLDP_EINVAL
    assert L.bldp_abi_version() == 5 and "quantile" not in E.OPS


# ---------------------------------------------------------------------------
# the Python layer on NumPy arrays

def test_helper_and_bad_p(pkg):
    assert pkg.quantile(0.25) == ("quantile", 0.25) and pkg.quantile(1) == ("quantile", 1.0)
    assert isinstance(pkg.quantile(np.float32(0.5))[1], float)
    a = np.zeros((8, 1, 4), dtype=np.float32, order="F")
    for bad in (-0.1, 1.5, float("nan"), INF, "x", None):
        with pytest.raises(ValueError, match="quantile"):
            pkg.quantile(bad)
        for arr in (a, a.astype(np.float64), a.astype(np.uint8)):  # (Float32: before any GPU work)
            with pytest.raises(ValueError, match="quantile"):
                pkg.fqav(arr, 2, ("quantile", bad))
            with pytest.raises(ValueError, match="quantile"):
                pkg.worker.getdata(arr, fqavby=2, fqavfunc=("quantile", bad))
            with pytest.raises(ValueError, match="quantile"):
                pkg.worker.getdata(arr, tavby=2, tavfunc=("quantile", bad))
        with pytest.raises(ValueError, match="quantile"):
            pkg.engine.quantile_host(a, 2, bad)
        with pytest.raises(ValueError, match="quantile"):
            pkg.GBT.getband([0], ["nothing.fil"], fqavby=2, fqavfunc=("quantile", bad))
    for f in (("quantile",), ("quantile", 0.5, 1), ("median", 0.5)):
        with pytest.raises(ValueError):
            pkg.fqav(a, 2, f)
    with pytest.raises(ValueError, match="axis"):
        pkg.engine.quantile_host(a, 2, 0.5, axis=1)
    with pytest.raises(ValueError, match="quantile"):
        pkg.fqav(a, 2, "quantile")  # the string alone names no function
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(a, fqavby=2, fqavfunc=pkg.quantile(0.5), tavby=2)
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(a.astype(np.int16), fqavby=2, fqavfunc=pkg.quantile(0.5), tavby=2)
    assert pkg.engine.out_dtype(np.dtype(np.float32), pkg.quantile(0.5)) == np.float32
    assert pkg.engine.out_dtype(np.dtype(np.uint8), pkg.quantile(0.5)) == np.float64


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
    f64[20:24, 1, 2] = [-1.7e308, 1.7e308, 1.7e308, -1.7e308]  # d overflows Float64
    for a in (f64, u8, i16):
        for p in (0.0, 0.25, 0.5, 1 / 3, 1.0):
            q = pkg.quantile(p)
            for n in (2, 3, 4, 24):
                got = pkg.fqav(a, n, q)
                assert got.dtype == np.float64 and same_bits(got, quantile_ref(a, n, p)), \
                    (a.dtype, n, p)
            for n in (2, 3, 6):
                got = W.getdata(a, tavby=n, tavfunc=q)
                assert got.dtype == np.float64 and \
                    same_bits(got, quantile_ref(a, n, p, axis=2)), (a.dtype, n, p)
    q4 = pkg.fqav(f64, 4, ("quantile", 0.0))
    # a NaN; a = 1 beside b = Inf at g == 0; a = -Inf beside a finite b
    assert np.isnan(q4[1, 0, 0]) and np.isnan(q4[2, 1, 2]) and q4[3, 1, 2] == -INF
    assert q4[4, 1, 2] == 0.0 and not np.signbit(q4[4, 1, 2]) and q4[5, 1, 2] == -1.7e308
    assert pkg.fqav(f64, 4, ("quantile", 0.5))[5, 1, 2] == INF  # a + g * (d = Inf)
    # against NumPy where the rule and NumPy agree to rounding
    np.testing.assert_allclose(pkg.fqav(i16, 8, pkg.quantile(0.3)),
                               np.quantile(i16.reshape((8, 3, 2, 6), order="F"), 0.3, axis=0),
                               rtol=1e-13, atol=1e-13)
    # n <= 1 returns the window, in its own type
    assert pkg.fqav(f64, 1, pkg.quantile(0.3)) is f64
    r = W.getdata(u8, tavby=1, tavfunc=pkg.quantile(0.3))
    assert r.dtype == np.uint8 and np.array_equal(r, u8)
    r = W.getdata(i16, fqavby=1, fqavfunc=pkg.quantile(0.3))
    assert r.dtype == np.int16 and np.array_equal(r, i16)
    # a window goes with it, on both axes
    J, C = pkg.JRange, pkg.COLON
    got = W.getdata(i16, (J(24, -1, 1), C, J(2, 5)), 3, pkg.quantile(0.75))
    assert same_bits(got, quantile_ref(i16, 3, 0.75, [23, 24, -1, 0, 2, 1, 1, 4, 1]))
    got = W.getdata(i16, (J(3, 2, 21), C, J(6, -1, 1)), tavby=3, tavfunc=pkg.quantile(0.75))
    assert same_bits(got, quantile_ref(i16, 3, 0.75, [2, 10, 2, 0, 2, 1, 5, 6, -1], axis=2))
    # _host_stat itself, and two stages on the host
    assert same_bits(W._host_stat(u8, 4, ("quantile", 0.9)), quantile_ref(u8, 4, 0.9))
    assert same_bits(W._host_stat(u8, 3, ("quantile", 0.9), axis=2),
                     quantile_ref(u8, 3, 0.9, axis=2))
    s1 = pkg.fqav(i16, 4, pkg.quantile(0.25))
    assert same_bits(W.getdata(i16, fqavby=4, fqavfunc=pkg.quantile(0.25), tavby=3,
                               tavfunc=pkg.quantile(0.75)), quantile_ref(s1, 3, 0.75, axis=2))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.fqav(i16, 5, pkg.quantile(0.5))
    # a UInt8 SIGPROC file
    fil = str(tmp_path / "u8.fil")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=24, nifs=2, tsamp=1.0, nbits=8,
                                    telescope_id=6, machine_id=10, data_type=1, tstart=59000.0,
                                    source_name="X"), u8)
    got = W.getdata(fil, fqavby=4, fqavfunc=pkg.quantile(0.25))
    assert got.dtype == np.float64 and same_bits(got, quantile_ref(u8, 4, 0.25))
    got = W.getdata(fil, tavby=3, tavfunc=pkg.quantile(0.75))
    assert got.dtype == np.float64 and same_bits(got, quantile_ref(u8, 3, 0.75, axis=2))


def test_engine_checks_without_a_device(pkg):
    eng = pkg.engine
    with pytest.raises(TypeError):
        eng.quantile_host(np.zeros((4, 1, 4), np.float64, order="F"), 2, 0.5)
    with pytest.raises(pkg._lib.DimensionMismatch):
        eng.quantile_host(np.zeros((4, 1, 4), np.float32, order="F"), 3, 0.5, axis=2)
    assert eng.quantile_host(np.zeros((4, 1, 0), np.float32, order="F"), 2, 0.5).shape == (2, 1, 0)
    assert eng.tstat_host(np.zeros((4, 1, 0), np.float32, order="F"), 2,
                          ("quantile", 0.5)).shape == (4, 1, 0)
    with pytest.raises(TypeError):
        eng.band_reduce_multi([None, None], 4, 1, ("quantile", 0.5))
    with pytest.raises(TypeError, match="quantile"):
        eng._no_quantile(("quantile", 0.5), "PreparedReduce")


def test_julia_shim_and_docs():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in ("bldp_quantile_shape", "bldp_quantile_plan_f32", "bldp_quantile_f32",
                 "bldp_band_quantile_f32", "bldp_quantile_host_f32"):
        assert re.search(r"ccall\(\(:%s, libbldp\)" % name, src), name
    assert re.search(r"^function quantile\(X::AbstractArray, p::Real; dims", src, re.M)
    assert re.search(r"\bquantile\b", src.split("export")[1].split("\n\n")[0])
    assert "dims == 1 || dims == 3" in src
    assert re.findall(r"^using .*$", src, re.M) == ["using Statistics: mean, median, var, std"]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert re.search(r"\bquantile\b", open(os.path.join(REPO, doc)).read()), doc
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "from memory" in design.split("Quantile")[1]
