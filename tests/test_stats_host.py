"""CPU: the host side of fqavfunc "var" / "std" / "median" — the op codes and
result types of the C ABI (pure host functions of libbldp_hip), the tavby
rule, Julia's rules restated in NumPy for element types the GPU ops do not
take, and the Julia shim's opcode table."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

F32, U8, F64 = 0, 2, 1  # bldp_dtype


def test_ops_and_paths(pkg):
    assert {k: pkg._lib.OPS[k] for k in ("var", "std", "median")} == \
        {"var": 4, "std": 5, "median": 6}
    assert pkg._lib.OPS["sum"] == 0 and pkg._lib.OPS["min"] == 3
    names = [pkg._lib.PATHS[k] for k in (8, 9, 10, 11)]
    assert len(set(names)) == 4 and not set(names) & {pkg._lib.PATHS[k] for k in range(8)}


def test_out_dtype(pkg):
    L = pkg._lib.lib()
    for op in (4, 5, 6):
        assert L.bldp_reduce_out_dtype(F32, op) == F32
    assert L.bldp_reduce_out_dtype(U8, 6) == F64
    assert L.bldp_reduce_out_dtype(F64, 4) == F64
    assert L.bldp_reduce_out_dtype(F32, 9) == pkg._lib.BLDP_EINVAL
    assert pkg.engine.out_dtype(np.dtype(np.int16), "std") == np.float64


def test_tavby_is_einval(pkg):
    L = pkg._lib.lib()
    rc = L.bldp_reduce_f32(None, 64, 1, 4, None, 4, 2, 6, None, None)
    assert rc == pkg._lib.BLDP_EINVAL
    assert "tavby" in pkg._lib.last_error()
    info = (ctypes.c_int64 * 8)()
    for op in (4, 5):
        assert L.bldp_reduce_plan_f32(None, 64, 1, 4, None, 4, 2, op, None, info) == \
            pkg._lib.BLDP_EINVAL
    # the Python mirror says it as a TypeError before any call
    a = np.zeros((8, 1, 4), dtype=np.float32, order="F")
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(a, fqavby=2, fqavfunc="median", tavby=2)
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(a.astype(np.int16), fqavby=2, fqavfunc="var", tavby=2)


def test_multi_device_entry_refuses(pkg):
    L = pkg._lib.lib()
    devs = (ctypes.c_int * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(0)
    rc = L.bldp_band_reduce_multi_f32(1, ctypes.cast(devs, ctypes.c_void_p),
                                      ctypes.cast(ptrs, ctypes.c_void_p), 64, 1, 4, None, 4, 1, 6,
                                      0, None, 0)
    assert rc == pkg._lib.BLDP_EINVAL and "one device" in pkg._lib.last_error()


def test_int16_statistics_are_float64(pkg):
    # the array of test_host.py::test_fqav_generic_keeps_f_result_type
    a = np.asfortranarray(np.array([1, 2, 4, 7, -3, 8, 10, 11], dtype=np.int16).reshape((8, 1, 1)))
    med = pkg.fqav(a, 2, "median")
    assert med.dtype == np.float64 and med.shape == (4, 1, 1)
    np.testing.assert_array_equal(med[:, 0, 0], [1.5, 5.5, 2.5, 10.5])
    R = a.astype(np.float64).reshape((4, 2, 1, 1), order="F")
    sd = pkg.fqav(a, 4, "std")
    assert sd.dtype == np.float64 and sd.shape == (2, 1, 1)
    np.testing.assert_array_equal(sd, np.std(R, axis=0, ddof=1))
    vr = pkg.fqav(a, 4, "var")
    assert vr.dtype == np.float64
    np.testing.assert_array_equal(vr, np.var(R, axis=0, ddof=1))
    # odd blocks: the middle element, as Float64; a window goes with it
    odd = np.asfortranarray(np.array([5, 1, 3, 2, 9, 4], dtype=np.uint8).reshape((6, 1, 1)))
    np.testing.assert_array_equal(pkg.fqav(odd, 3, "median")[:, 0, 0], [3.0, 4.0])
    got = pkg.worker.getdata(odd, (pkg.JRange(6, -1, 1), pkg.COLON, pkg.COLON), 3, "median")
    np.testing.assert_array_equal(got[:, 0, 0], [4.0, 3.0])


def test_float64_median_rules(pkg):
    big = np.finfo(np.float64).max
    a = np.asfortranarray(np.array([big, big, -0.0, 0.0, 0.0, -0.0, 1.0, np.nan, 0.0, -0.0, -0.0,
                                    7.0], dtype=np.float64).reshape((12, 1, 1)))
    m2 = pkg.fqav(a, 2, "median")[:, 0, 0]
    assert m2[0] == big  # a/2 + b/2, not (a + b)/2
    assert np.isnan(m2[3]) and not np.isnan(m2[[0, 1, 2, 4, 5]]).any()
    m3 = pkg.fqav(a[6:], 3, "median")[:, 0, 0]  # (1, NaN, 0) and (-0, -0, 7)
    assert np.isnan(m3[0]) and m3[1] == 0.0 and np.signbit(m3[1])
    m3 = pkg.fqav(np.asfortranarray(a[2:5]), 3, "median")[:, 0, 0]  # (-0, 0, 0): isless order
    assert m3[0] == 0.0 and not np.signbit(m3[0])


def test_dimension_mismatch(pkg):
    a = np.arange(24, dtype=np.float32).reshape((4, 2, 3), order="F")
    with pytest.raises(pkg.DimensionMismatch):
        pkg.fqav(a, 3, "median")
    with pytest.raises(pkg.DimensionMismatch):
        pkg.fqav(a.astype(np.int32), 3, "var")
    assert pkg.fqav(a, 1, "var") is a  # n <= 1 returns A itself whatever f is


def test_numpy_callables_stay_on_the_host(pkg):
    # np.std is the population form: only the strings select Julia's
    a = np.arange(24, dtype=np.float32).reshape((4, 2, 3), order="F")
    assert pkg.worker._opname(np.median) is None and pkg.worker._opname(np.std) is None
    np.testing.assert_array_equal(pkg.fqav(a, 4, np.std),
                                  np.std(a.reshape((4, 1, 2, 3), order="F"), axis=0))
    with pytest.raises(ValueError):
        pkg.fqav(a, 2, "mode")


def test_julia_shim_opcodes():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    assert re.search(r"using Statistics:[^\n]*\bmedian\b", src)
    for fn in ("var", "std"):
        assert re.search(rf"using Statistics:[^\n]*\b{fn}\b", src)
    m = re.search(r"^opcode\(f, A\) =(.*?)\n\n", src, re.S | re.M)
    assert m, "opcode(f, A) not found"
    body = m.group(1)
    assert "Array{Float32,3}" in body
    for fn, code in (("var", 4), ("std", 5), ("median", 6)):
        assert re.search(rf"f === {fn} \? Cint\({code}\)", body), fn
    # the Float32 method and gpu_fqav ask with the array; the typed method does not
    assert len(re.findall(r"opcode\(f, A\)", src)) >= 3


def test_header_names_the_ops():
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    for name, code in (("BLDP_OP_VAR", 4), ("BLDP_OP_STD", 5), ("BLDP_OP_MEDIAN", 6)):
        assert re.search(rf"\b{name} = {code}\b", hdr)
    assert re.search(r"#define BLDP_ABI_VERSION 5\b", hdr)
