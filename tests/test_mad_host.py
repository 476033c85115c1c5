"""CPU: the host side of fqavfunc / tavfunc "mad" (BLDP_OP_MAD = 8, the
normalised median absolute deviation) — the op code and result types of the C
ABI, the refusals it shares with median, the plans (pure host functions of
libbldp_hip: mad reports the median's path for its shape), the rule restated
in NumPy (mad_ref.py) for the element types the GPU op does not take, and the
Julia shim."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, same_bits
from mad_ref import MAD_CONSTANT, mad_ref

F32, F64, U8, I16 = 0, 1, 2, 7  # bldp_dtype
MEDIAN, MAD = 6, 8
INF = np.inf


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def test_op_code_header_and_abi(pkg, L):
    assert pkg._lib.OPS["mad"] == MAD and "mad" in pkg._lib.STAT_OPS
    assert 7 not in pkg._lib.OPS.values()  # unassigned
    assert {k: pkg._lib.OPS[k] for k in ("var", "std", "median")} == \
        {"var": 4, "std": 5, "median": 6}
    assert pkg._lib.MAD_CONSTANT == MAD_CONSTANT == 1.4826022185056018
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    assert re.search(r"\bBLDP_OP_MAD = 8\b", hdr)
    assert not re.search(r"\bBLDP_OP_\w+ = 7\b", hdr)
    assert re.search(r"#define BLDP_ABI_VERSION 5\b", hdr)
    assert L.bldp_abi_version() == 5


def test_out_dtype(pkg, L):
    assert L.bldp_reduce_out_dtype(F32, MAD) == F32
    for dt in range(1, 10):
        assert L.bldp_reduce_out_dtype(dt, MAD) == F64, dt
    for op in (7, 9, -1):
        assert L.bldp_reduce_out_dtype(F32, op) == pkg._lib.BLDP_EINVAL, op
        assert L.bldp_reduce_out_dtype(U8, op) == pkg._lib.BLDP_EINVAL, op
    assert pkg.engine.out_dtype(np.dtype(np.float32), "mad") == np.float32
    assert pkg.engine.out_dtype(np.dtype(np.int16), "mad") == np.float64
    assert pkg.engine.out_dtype(np.dtype(np.float64), "mad") == np.float64


def test_codes_7_and_9_stay_invalid(pkg, L):
    E = pkg._lib
    info = (ctypes.c_int64 * 8)()
    for op in (7, 9):
        assert L.bldp_reduce_f32(None, 64, 1, 4, None, 4, 1, op, None, None) == E.BLDP_EINVAL, op
        assert "unknown op" in E.last_error()
        assert L.bldp_reduce_plan_f32(None, 64, 1, 4, None, 4, 1, op, None, info) == E.BLDP_EINVAL
        assert L.bldp_tstat_plan_f32(None, 64, 1, 4, None, 2, op, None, info) == E.BLDP_EINVAL
        assert "bldp_reduce_" in E.last_error()
        assert L.bldp_tstat_f32(None, 64, 1, 4, None, 2, op, None, 64, 64, None) == E.BLDP_EINVAL
        assert L.bldp_tstat_host_f32(0, None, 64, 1, 4, None, 2, op, None) == E.BLDP_EINVAL
        assert L.bldp_reduce_strided(F32, None, 64, 1, 4, None, 4, 1, op, None, 16, 16,
                                     None) == E.BLDP_EINVAL
    # 8 passes those checks: the plans below, and here the next check of each entry point
    assert L.bldp_reduce_f32(None, 64, 1, 4, None, 4, 1, MAD, None, None) == E.BLDP_EINVAL
    assert "null" in E.last_error()
    assert L.bldp_tstat_f32(None, 64, 1, 4, None, 2, MAD, None, 64, 64, None) == E.BLDP_EINVAL
    assert "null" in E.last_error()
    assert L.bldp_tstat_f32(None, 64, 1, 4, None, 3, MAD, None, 64, 64, None) == E.BLDP_EDIM
    assert L.bldp_reduce_f32(None, 64, 1, 4, None, 5, 1, MAD, None, None) == E.BLDP_EDIM
    # typed element types: Float32 only on the GPU, as for median
    rc = L.bldp_reduce_strided(I16, None, 256, 2, 3, None, 4, 1, MAD, None, 64, 128, None)
    assert rc == E.BLDP_EINVAL and "Float32" in E.last_error()


def test_tavby_is_refused(pkg, L):
    E = pkg._lib
    rc = L.bldp_reduce_f32(None, 64, 1, 4, None, 4, 2, MAD, None, None)
    assert rc == E.BLDP_EINVAL and "tavby" in E.last_error()
    info = (ctypes.c_int64 * 8)()
    assert L.bldp_reduce_plan_f32(None, 64, 1, 4, None, 4, 2, MAD, None, info) == E.BLDP_EINVAL
    assert "tavby" in E.last_error()
    a = np.zeros((8, 1, 4), dtype=np.float32, order="F")
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(a, fqavby=2, fqavfunc="mad", tavby=2)
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(a.astype(np.int16), fqavby=2, fqavfunc="mad", tavby=2)
    with pytest.raises(TypeError, match="tavby"):
        pkg.engine._check_stat("mad", 2)


def test_multi_device_entry_refuses(pkg, L):
    devs = (ctypes.c_int * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(0)
    rc = L.bldp_band_reduce_multi_f32(1, ctypes.cast(devs, ctypes.c_void_p),
                                      ctypes.cast(ptrs, ctypes.c_void_p), 64, 1, 4, None, 4, 1, MAD,
                                      0, None, 0)
    assert rc == pkg._lib.BLDP_EINVAL and "one device" in pkg._lib.last_error()


def reduce_plan(pkg, L, dims, F, op):
    info = (ctypes.c_int64 * 8)()
    rc = L.bldp_reduce_plan_f32(None, *dims, None, F, 1, op, None, info)
    assert rc == pkg._lib.BLDP_OK, pkg._lib.last_error()
    return list(info)


def tstat_plan(pkg, L, dims, T, op):
    info = (ctypes.c_int64 * 8)()
    rc = L.bldp_tstat_plan_f32(None, *dims, None, T, op, None, info)
    assert rc == pkg._lib.BLDP_OK, pkg._lib.last_error()
    return list(info)


def test_plans_are_the_medians(pkg, L):
    P, TP = pkg._lib.PATHS, pkg._lib.TSTAT_PATHS
    want = {64: "median_sort", 65: "median_select", 4096: "median_select", 4097: "median_stream"}
    for F, path in want.items():
        mad = reduce_plan(pkg, L, (2 * F, 2, 3), F, MAD)
        assert P[mad[0]] == path, F
        assert mad == reduce_plan(pkg, L, (2 * F, 2, 3), F, MEDIAN), F
    # fqavby <= 1 is the copy, as for median
    assert reduce_plan(pkg, L, (64, 2, 3), 1, MAD) == reduce_plan(pkg, L, (64, 2, 3), 1, MEDIAN)
    # the time axis: passes 2 in registers, 8 / 10 for an odd / even split block
    for T, path, passes, med_passes in ((32, "regs_median", 2, 1), (33, "split_median", 8, 4),
                                        (34, "split_median", 10, 5)):
        mad = tstat_plan(pkg, L, (264, 2, 2 * T), T, MAD)
        med = tstat_plan(pkg, L, (264, 2, 2 * T), T, MEDIAN)
        assert TP[mad[0]] == path and mad[3] == passes and med[3] == med_passes, T
        assert mad[:3] + mad[4:] == med[:3] + med[4:], T
    assert tstat_plan(pkg, L, (264, 2, 8), 1, MAD)[0] == -1  # the copy
    assert set(P.values()) >= set(want.values()) and len(P) == 12 and len(TP) == 5


def test_dimension_mismatch_and_n_le_1(pkg):
    a = np.arange(24, dtype=np.float32).reshape((4, 2, 3), order="F")
    with pytest.raises(pkg.DimensionMismatch):
        pkg.fqav(a, 3, "mad")
    with pytest.raises(pkg.DimensionMismatch):
        pkg.fqav(a.astype(np.int32), 3, "mad")
    with pytest.raises(pkg._lib.DimensionMismatch):
        pkg.worker.getdata(a.astype(np.int16), tavby=2, tavfunc="mad")
    assert pkg.fqav(a, 1, "mad") is a  # n <= 1 returns A itself whatever f is
    i = a.astype(np.int16)
    r = pkg.worker.getdata(i, tavby=1, tavfunc="mad")
    assert r.dtype == np.int16 and np.array_equal(r, i)
    with pytest.raises(ValueError):
        pkg.fqav(a, 2, "mads")
    assert pkg.worker._opname(np.median) is None  # callables stay on the host


def test_restatement_special_cases():
    def one(v, dt=np.float32):
        return mad_ref(np.array(v, dt).reshape((len(v), 1, 1)), len(v))[0, 0, 0]

    assert one([7.5] * 4) == 0.0 and not np.signbit(one([7.5] * 4))
    got = one([1, 2, INF, 4])  # c = 3, d = 2, 1, Inf, 1 -> m = 1.5
    assert got.dtype == np.float32 and got == np.float32(1.5 * MAD_CONSTANT)
    assert np.isnan(one([INF, INF, INF, 1]))  # c = Inf: Inf - Inf
    assert np.isnan(one([1, np.nan, 3]))
    z = one([0.0, -0.0, -0.0, 0.0, -0.0])
    assert z == 0.0 and not np.signbit(z)
    assert one([1, 2, 4, 7, 100]) == np.float32(3 * MAD_CONSTANT)  # c = 4, d = 3, 2, 0, 3, 96
    assert one([1, 2, INF, 4], np.float64) == 1.5 * MAD_CONSTANT
    # against the float64 numpy.median formulation (not bit for bit: its middle is (a + b) / 2)
    x = np.random.default_rng(0).gamma(2.0, 5e8, (64, 50, 1)).astype(np.float32)
    want = np.median(np.abs(x - np.median(x, axis=0)), axis=0).astype(np.float64) * MAD_CONSTANT
    np.testing.assert_allclose(mad_ref(np.asfortranarray(x), 64)[0], want, rtol=2e-7)


def test_other_element_types_are_float64_from_the_host(pkg, tmp_path):
    W = pkg.worker
    rng = np.random.default_rng(3)
    i16 = np.asfortranarray(rng.integers(-300, 300, (24, 2, 6)).astype(np.int16))
    u8 = np.asfortranarray(rng.integers(0, 4, (24, 2, 6)).astype(np.uint8))  # heavy ties
    f64 = np.asfortranarray(rng.standard_normal((24, 2, 6)))
    f64[5, 0, 0] = np.nan
    f64[8:12, 1, 2] = [INF, INF, INF, 1.0]
    f64[12:16, 1, 2] = [1.0, 2.0, INF, 4.0]
    f64[16:20, 1, 2] = [-0.0, 0.0, -0.0, 0.0]
    f64[20:24, 1, 2] = 3.25
    for a in (i16, u8, f64):
        for n in (2, 3, 4, 24):
            got = pkg.fqav(a, n, "mad")
            assert got.dtype == np.float64 and same_bits(got, mad_ref(a, n)), (a.dtype, n)
        for n in (2, 3, 6):
            got = W.getdata(a, tavby=n, tavfunc="mad")
            assert got.dtype == np.float64 and same_bits(got, mad_ref(a, n, axis=2)), (a.dtype, n)
    m4 = pkg.fqav(f64, 4, "mad")
    assert np.isnan(m4[1, 0, 0]) and np.isnan(m4[2, 1, 2]) and m4[3, 1, 2] == 1.5 * MAD_CONSTANT
    assert m4[4, 1, 2] == 0.0 and not np.signbit(m4[4, 1, 2]) and m4[5, 1, 2] == 0.0
    # a window goes with it, on both axes
    J, C = pkg.JRange, pkg.COLON
    got = W.getdata(i16, (J(24, -1, 1), C, J(2, 5)), 3, "mad")
    assert same_bits(got, mad_ref(i16, 3, [23, 24, -1, 0, 2, 1, 1, 4, 1]))
    got = W.getdata(i16, (J(3, 2, 21), C, J(6, -1, 1)), tavby=3, tavfunc="mad")
    assert same_bits(got, mad_ref(i16, 3, [2, 10, 2, 0, 2, 1, 5, 6, -1], axis=2))
    # _host_stat itself, and two stages on the host
    assert same_bits(W._host_stat(u8, 4, "mad"), mad_ref(u8, 4))
    assert same_bits(W._host_stat(u8, 3, "mad", axis=2), mad_ref(u8, 3, axis=2))
    s1 = pkg.fqav(i16, 4, "median")
    assert same_bits(W.getdata(i16, fqavby=4, fqavfunc="median", tavby=3, tavfunc="mad"),
                     mad_ref(s1, 3, axis=2))
    # a UInt8 SIGPROC file
    fil = str(tmp_path / "u8.fil")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=24, nifs=2, tsamp=1.0, nbits=8,
                                    telescope_id=6, machine_id=10, data_type=1, tstart=59000.0,
                                    source_name="X"), u8)
    got = W.getdata(fil, fqavby=4, fqavfunc="mad")
    assert got.dtype == np.float64 and same_bits(got, mad_ref(u8, 4))
    got = W.getdata(fil, tavby=3, tavfunc="mad")
    assert got.dtype == np.float64 and same_bits(got, mad_ref(u8, 3, axis=2))


def test_engine_checks_without_a_device(pkg):
    eng = pkg.engine
    with pytest.raises(TypeError):
        eng.tstat_host(np.zeros((4, 1, 4), np.float64, order="F"), 2, "mad")
    with pytest.raises(pkg._lib.DimensionMismatch):
        eng.tstat_host(np.zeros((4, 1, 4), np.float32, order="F"), 3, "mad")
    assert eng.tstat_host(np.zeros((4, 1, 0), np.float32, order="F"), 2, "mad").shape == (4, 1, 0)
    with pytest.raises(TypeError):
        eng.band_reduce_multi([None, None], 4, 1, "mad")


def test_julia_shim_and_docs():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    m = re.search(r"^opcode\(f, A\) =(.*?)\n\n", src, re.S | re.M)
    assert m and "Array{Float32,3}" in m.group(1)
    assert re.search(r"f === mad \? Cint\(8\)", m.group(1))
    assert re.search(r"f === median \? Cint\(6\)", m.group(1))
    assert not re.search(r"Cint\(7\)", m.group(1))
    s = re.search(r"^statcode\(f\) =(.*?)\n\n", src, re.S | re.M)
    assert s and re.search(r"f === mad \? Cint\(8\)", s.group(1))
    assert re.search(r"^mad\(X::AbstractArray; dims", src, re.M)  # defined, with dims
    assert re.search(r"\bmad\b", src.split("export")[1].split("\n\n")[0])  # and exported
    assert "1.4826022185056018" in src
    assert not re.search(r"^\s*(using|import)\s+StatsBase", src, re.M)  # no new dependency
    assert re.findall(r"^using .*$", src, re.M) == ["using Statistics: mean, median, var, std"]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert re.search(r"\bmad\b", open(os.path.join(REPO, doc)).read()), doc
