"""CPU: the host side of getskewness — the four additive entry points of the C
ABI (plan and argument checks are pure host functions of libbldp_hip), the
Python layers' keyword and element-type errors, the Julia shim, and the
statement's own arithmetic against the bounds of tests/skewness_ref.py."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from skewness_ref import SKEW_LEAF_TOL, skew_statement, skew_sum_tol

NEW = ("bldp_skewness_plan_f32", "bldp_skewness_f32", "bldp_band_skewness_f32",
       "bldp_skewness_host_f32")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def win(*w):
    a = (ctypes.c_int64 * 9)(*w)
    return a, ctypes.cast(a, ctypes.c_void_p)


def splan(pkg, L, dims, w, tblock):
    info = (ctypes.c_int64 * 4)()
    rc = L.bldp_skewness_plan_f32(None, *dims, w, tblock, info)
    assert rc == pkg._lib.BLDP_OK, pkg._lib.last_error()
    return {"path": pkg._lib.KURT_PATHS[info[0]], "fused": info[1], "blocks": info[2],
            "workspace_bytes": info[3]}


def test_symbols_declared_bound_and_exported(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    declared = set(re.findall(r"BLDP_API\s+\w+\s+(bldp_\w+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (bldp_\w+)", out))
    for name in NEW:
        assert name in declared, name
        assert name in pkg._lib.SIGNATURES, name
        assert name in exported, name
    assert L.bldp_abi_version() == 5
    for name in ("skewness", "band_skewness", "skewness_host", "skewness_plan"):
        assert callable(getattr(pkg.engine, name)) and name in pkg.engine.__all__, name
    assert callable(pkg.WorkerFunctions.getskewness) and callable(pkg.GBT.getskewness)
    assert pkg.getskewness is pkg.WorkerFunctions.getskewness and "getskewness" in pkg.__all__


@pytest.mark.parametrize("nc", [8, 6])
@pytest.mark.parametrize("nt", [16, 33, 512, 513, 2049])
def test_plan_is_the_kurtosis_plan(pkg, L, nt, nc):
    """With null pointers and no GPU: the whole window (tblock = 0) takes the
    path bldp_kurtosis_plan_f32 gives, blocks the path, form and count
    bldp_kurtosis_blocks_plan_f32 gives."""
    dims = (nc, 2, 3 * nt)
    keep, w = win(0, nc, 1, 0, 2, 1, 0, nt, 1)
    info = (ctypes.c_int64 * 4)()
    assert L.bldp_kurtosis_plan_f32(None, *dims, w, info) == 0
    p = splan(pkg, L, dims, w, 0)
    assert p["path"] == pkg._lib.KURT_PATHS[info[0]]
    assert (p["fused"], p["blocks"]) == (1, 1)
    want = {16: "regs", 33: "mid", 512: "mid", 513: "leaf", 2049: "leaf"}[nt]
    if nc == 6:  # no float4 columns
        want = "mid" if nt <= 512 else "twopass"
    assert p["path"] == want
    assert p["workspace_bytes"] <= L.bldp_kurtosis_workspace_size(*dims, w)
    binfo = (ctypes.c_int64 * 4)()
    assert L.bldp_kurtosis_blocks_plan_f32(None, *dims, None, nt, binfo) == 0
    pb = splan(pkg, L, dims, None, nt)
    assert (pkg._lib.KURT_PATHS[binfo[0]], binfo[1], binfo[2]) == \
        (pb["path"], pb["fused"], pb["blocks"])
    assert pb["blocks"] == 3 and pb["fused"] == (1 if nc == 8 and nt <= 1024 else 0)


def test_error_codes(pkg, L):
    E = pkg._lib
    dims = (512, 1, 1024)
    info = (ctypes.c_int64 * 4)()
    out = np.zeros(8, dtype=np.float64)
    a = np.zeros(8, dtype=np.float32)
    ptrs = (ctypes.c_void_p * 2)(0, 0)
    pp = ctypes.cast(ptrs, ctypes.c_void_p)

    def every(w, tblock, code):
        assert L.bldp_skewness_plan_f32(None, *dims, w, tblock, info) == code
        assert L.bldp_skewness_f32(None, *dims, w, tblock, None, 512, 512, None) == code
        assert L.bldp_band_skewness_f32(2, pp, *dims, w, tblock, None, None) == code
        assert L.bldp_skewness_host_f32(0, None, *dims, w, tblock, None) == code

    every(None, 3, E.BLDP_EDIM)  # nt % M != 0
    assert "tblock" in E.last_error()
    every(None, -1, E.BLDP_EINVAL)  # M < 0
    assert "tblock" in E.last_error()
    keep, w = win(0, 512, 1, 0, 1, 1, 1000, 32, 1)  # past the last spectrum
    every(w, 0, E.BLDP_EBOUNDS)
    every(w, 16, E.BLDP_EBOUNDS)
    assert L.bldp_skewness_plan_f32(None, *dims, None, 0, None) == E.BLDP_EINVAL
    # null in / out for a non-empty result, both forms
    for M in (0, 16):
        assert L.bldp_skewness_f32(None, *dims, None, M, out.ctypes.data, 512, 512,
                                   None) == E.BLDP_EINVAL
        assert L.bldp_skewness_f32(a.ctypes.data, *dims, None, M, None, 512, 512,
                                   None) == E.BLDP_EINVAL
        assert L.bldp_skewness_host_f32(0, None, *dims, None, M, out.ctypes.data) == E.BLDP_EINVAL
        assert L.bldp_skewness_host_f32(0, a.ctypes.data, *dims, None, M, None) == E.BLDP_EINVAL
        assert L.bldp_band_skewness_f32(1, None, *dims, None, M, out.ctypes.data,
                                        None) == E.BLDP_EINVAL
        assert L.bldp_band_skewness_f32(2, pp, *dims, None, M, out.ctypes.data,
                                        None) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers (and no GPU)
    keep, w = win(0, 0, 1, 0, 1, 1, 0, 64, 1)  # no channels
    for M in (0, 16):
        assert L.bldp_skewness_f32(None, *dims, w, M, None, 512, 512, None) == E.BLDP_OK
        assert L.bldp_skewness_host_f32(0, None, *dims, w, M, None) == E.BLDP_OK
        assert L.bldp_band_skewness_f32(2, pp, *dims, w, M, None, None) == E.BLDP_OK
    keep, w = win(0, 512, 1, 0, 1, 1, 5, 0, 1)  # no spectra: no blocks
    assert L.bldp_skewness_f32(None, *dims, w, 16, None, 512, 512, None) == E.BLDP_OK
    assert splan(pkg, L, dims, w, 16)["blocks"] == 0


def test_python_keyword_and_type_errors_before_any_launch(pkg):
    import torch

    a = np.zeros((8, 1, 12), dtype=np.float32, order="F")
    W, eng = pkg.worker, pkg.engine
    x = torch.zeros((12, 1, 8)).permute(2, 1, 0)
    calls = (lambda **k: W.getskewness(a, **k), lambda **k: eng.skewness_host(a, **k),
             lambda **k: eng.skewness(x, **k), lambda **k: eng.band_skewness([x, x], **k),
             lambda **k: eng.skewness_plan(x, **k), lambda **k: W.getskewness(x, **k))
    for f in calls:
        for bad in (True, 2.5):  # bool, non-integer
            with pytest.raises(TypeError, match="tblock"):
                f(tblock=bad)
        for bad in (-1, 0):  # (tblock=None is the whole window)
            with pytest.raises(ValueError, match="tblock"):
                f(tblock=bad)
        with pytest.raises(pkg.DimensionMismatch, match="tblock=5"):  # non-divisor
            f(tblock=5)
    idxs = (pkg.COLON, pkg.COLON, pkg.JRange(1, 2, 12))  # 6 selected spectra
    with pytest.raises(pkg.DimensionMismatch, match="tblock=4"):
        W.getskewness(a, idxs, tblock=4)
    # anything but Float32 is a TypeError naming Float32
    for dt in (np.int16, np.uint8, np.float64):
        b = a.astype(dt)
        t = torch.from_numpy(np.ascontiguousarray(b.transpose(2, 1, 0))).permute(2, 1, 0)
        for f in (lambda: W.getskewness(b), lambda: eng.skewness_host(b),
                  lambda: W.getskewness(b, tblock=4), lambda: W.getskewness(t),
                  lambda: eng.skewness(t), lambda: eng.band_skewness([t])):
            with pytest.raises(TypeError, match="Float32"):
                f()


def test_eight_bit_sigproc_file_is_a_type_error(pkg, tmp_path):
    a = np.asfortranarray(np.arange(8 * 12, dtype=np.uint8).reshape((8, 1, 12), order="F"))
    fil = str(tmp_path / "u8.fil")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=8, nifs=1, tsamp=1.0, nbits=8,
                                    telescope_id=6, machine_id=10, data_type=1, tstart=59000.0,
                                    source_name="X"), a)
    with pytest.raises(TypeError, match="Float32"):
        pkg.WorkerFunctions.getskewness(fil)


def test_julia_shim_ccall_agrees_with_the_header():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    assert re.search(r"function gpu_skewness\(A::Array\{Float32,3\};[^\n]*\n\s*tblock::Integer=0\)",
                     src)
    assert re.search(r"export[^\n]*\n[^\n]*gpu_skewness", src)
    call = re.search(r"ccall\(\(:bldp_skewness_host_f32, libbldp\), Cint,\s*\(([^()]*)\)", src, re.S)
    assert " ".join(call.group(1).split()) == \
        "Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}"
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    decl = re.search(r"BLDP_API int bldp_skewness_host_f32\(([^)]*)\)", hdr, re.S)
    types = [" ".join(p.split()[:-1]) for p in " ".join(decl.group(1).split()).split(",")]
    assert types == ["int", "const float", "int64_t", "int64_t", "int64_t", "const int64_t",
                     "int64_t", "double"]


def test_the_statements_own_arithmetic_sits_inside_the_bounds(orc):
    """The recipe against an exact-Float64-z evaluation about the same m (what
    the leaf class differs by) and against an 8-partial reordering of its own
    terms (the sum class), on gamma rows of mean / sigma 1.4 .. 30000 and a row
    of one value and an ulp."""
    rng = np.random.default_rng(5)
    R = np.array([np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0])
    for nt in (33, 513, 4096):
        a = np.empty((6, 1, nt), dtype=np.float32, order="F")
        a[:5, 0] = rng.gamma((R ** 2)[:, None], (1e6 / R ** 2)[:, None], (5, nt))
        a[5, 0] = np.float32(2.0 ** 20) + np.float32(0.125) * rng.integers(0, 2, nt)
        s, A = skew_statement(orc, a)
        assert np.isfinite(s).all() and (A >= np.abs(s)).all()
        m = orc.mean_f32(a)[:, 0].astype(np.float64)[:, None]
        z = a[:, 0].astype(np.float64) - m
        exact = (z ** 3).sum(axis=1) / nt / ((z ** 2).sum(axis=1) / nt) ** 1.5
        assert (np.abs(exact - s[:, 0]) <= SKEW_LEAF_TOL * A[:, 0]).all(), nt
        z32 = (a[:, 0] - orc.mean_f32(a)[:, 0][:, None]).astype(np.float32)
        q = (z32 * z32).astype(np.float32)
        c = (q * z32).astype(np.float32).astype(np.float64)
        parts = np.array_split(np.arange(nt), 8)
        c3 = sum(np.add.accumulate(c[:, p], axis=1)[:, -1] for p in parts) / nt
        c2 = sum(np.add.accumulate(q[:, p].astype(np.float64), axis=1)[:, -1] for p in parts) / nt
        re8 = c3 / np.sqrt(c2 * c2 * c2)
        assert (np.abs(re8 - s[:, 0]) <= skew_sum_tol(nt) * A[:, 0]).all(), nt
