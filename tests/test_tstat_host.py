"""CPU: the host side of getdata(...; tavby, tavfunc) — the five additive
bldp_tstat_* entry points (shape, plan and argument checks are pure host
functions of libbldp_hip), the Float64 host path of the other element types,
the keyword's rules, and the Julia shim."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

NEW = ("bldp_tstat_shape", "bldp_tstat_plan_f32", "bldp_tstat_f32", "bldp_band_tstat_f32",
       "bldp_tstat_host_f32")
VAR, STD, MEDIAN = 4, 5, 6


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def win(*w):
    a = (ctypes.c_int64 * 9)(*w)
    return a, ctypes.cast(a, ctypes.c_void_p)


def shape(L, dims, w, tavby):
    d = (ctypes.c_int64 * 3)(-1, -1, -1)
    rc = L.bldp_tstat_shape(*dims, w, tavby, d)
    return rc, tuple(d)


def plan(pkg, L, dims, w, tavby, op):
    info = (ctypes.c_int64 * 8)()
    rc = L.bldp_tstat_plan_f32(None, *dims, w, tavby, op, None, info)
    assert rc == pkg._lib.BLDP_OK, pkg._lib.last_error()
    keys = ("path", "cpl", "tsplit", "passes", "workgroups", "workspace_bytes", "blocks", "lanes")
    d = dict(zip(keys, info))
    d["path"] = pkg._lib.TSTAT_PATHS.get(d["path"], "copy")
    return d


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
    assert re.search(r"#define BLDP_ABI_VERSION 5\b", hdr)
    assert set(pkg._lib.TSTAT_PATHS.values()) == {"regs_moments", "regs_median", "split_moments",
                                                  "split_median", "chunk_moments"}


def test_shape_and_argument_checks(pkg, L):
    E = pkg._lib
    dims = (512, 1, 1024)
    assert shape(L, dims, None, 16) == (E.BLDP_OK, (512, 1, 64))
    assert shape(L, dims, None, 1024) == (E.BLDP_OK, (512, 1, 1))
    rc, _ = shape(L, dims, None, 3)
    assert rc == E.BLDP_EDIM and "tavby" in E.last_error()
    # tavby <= 1: the dims of the window (fqav's n <= 1 rule)
    for t in (1, 0, -5):
        assert shape(L, dims, None, t) == (E.BLDP_OK, (512, 1, 1024))
    keep, w = win(4, 252, 2, 0, 1, 1, 3, 100, 2)  # the blocks cut the selected spectra
    assert shape(L, dims, w, 25) == (E.BLDP_OK, (126 * 2, 1, 4))
    assert shape(L, dims, w, 16)[0] == E.BLDP_EDIM
    assert shape(L, dims, w, 1) == (E.BLDP_OK, (252, 1, 100))
    keep, w = win(0, 512, 1, 0, 1, 1, 1000, 32, 1)  # past the last spectrum
    assert shape(L, dims, w, 16)[0] == E.BLDP_EBOUNDS
    keep, w = win(500, 16, 1, 0, 1, 1, 0, 32, 1)  # past the last channel
    assert shape(L, dims, w, 16)[0] == E.BLDP_EBOUNDS
    assert L.bldp_tstat_shape(*dims, None, 16, None) == E.BLDP_EINVAL
    # the op: var / std / median only, the message names the reduce
    info = (ctypes.c_int64 * 8)()
    for op in (0, 1, 2, 3, 7, -1):
        rc = L.bldp_tstat_plan_f32(None, *dims, None, 16, op, None, info)
        assert rc == E.BLDP_EINVAL and "bldp_reduce_" in E.last_error(), op
        rc = L.bldp_tstat_host_f32(0, None, *dims, None, 16, op, None)
        assert rc == E.BLDP_EINVAL and "bldp_reduce_" in E.last_error(), op
    # the other entry points run the same checks before touching a device
    assert L.bldp_tstat_f32(None, *dims, None, 3, MEDIAN, None, 512, 512, None) == E.BLDP_EDIM
    assert L.bldp_tstat_host_f32(0, None, *dims, None, 3, MEDIAN, None) == E.BLDP_EDIM
    assert L.bldp_tstat_f32(None, *dims, w, 16, MEDIAN, None, 16, 16, None) == E.BLDP_EBOUNDS
    assert L.bldp_band_tstat_f32(2, None, *dims, None, 3, VAR, None, None) == E.BLDP_EDIM
    assert L.bldp_band_tstat_f32(0, None, *dims, None, 16, VAR, None, None) == E.BLDP_EINVAL
    assert L.bldp_tstat_f32(None, *dims, None, 16, STD, None, 512, 512, None) == E.BLDP_EINVAL
    assert "null" in E.last_error()
    assert L.bldp_tstat_plan_f32(None, *dims, None, 16, STD, None, None) == E.BLDP_EINVAL


def test_plans(pkg, L):
    # blocks of <= 32 spectra: registers, one launch, no workspace
    band = (65536, 1, 272)
    for T, nt in ((2, 272), (16, 272), (32, 256)):
        keep, w = win(0, 65536, 1, 0, 1, 1, 0, nt, 1)
        for op, path in ((MEDIAN, "regs_median"), (VAR, "regs_moments"), (STD, "regs_moments")):
            p = plan(pkg, L, band, w, T, op)
            assert p == {"path": path, "cpl": 4, "tsplit": 1, "passes": 1,
                         "workgroups": 65536 // 4 * (nt // T) // 256, "workspace_bytes": 0,
                         "blocks": nt // T, "lanes": 0}, (T, op, p)
    # longer blocks: the time slices of a workgroup split T
    bank = (512, 1, 879616)
    for T in (1024, 879616):
        m = plan(pkg, L, bank, None, T, MEDIAN)
        assert m["path"] == "split_median" and m["cpl"] == 4 and m["lanes"] * m["cpl"] <= 32
        assert m["tsplit"] * m["lanes"] == 256 and m["tsplit"] > 1 and m["passes"] == 5
        assert m["workgroups"] == (128 // m["lanes"]) * (879616 // T) and m["workspace_bytes"] == 0
        v = plan(pkg, L, bank, None, T, VAR)
        assert v["passes"] == 2 and v["tsplit"] * v["lanes"] == 256 and v["tsplit"] > 1
        assert plan(pkg, L, bank, None, T, STD) == v
        if T == 1024:  # 859 blocks fill the GPU: one workgroup per tile and block
            assert v["path"] == "split_moments" and v["workspace_bytes"] == 0
            assert v["workgroups"] == -(-128 // v["lanes"]) * 859
        else:  # the whole scan as one block: time chunks across workgroups, partials in scratch
            assert v["path"] == "chunk_moments" and v["workgroups"] >= 256
            nchunk = v["workgroups"] // -(-128 // v["lanes"])
            assert 879616 // nchunk >= 4096 and v["workspace_bytes"] == 2 * nchunk * 512 * 8
    p33 = plan(pkg, L, (264, 2, 99), None, 33, MEDIAN)
    assert p33["path"] == "split_median" and p33["passes"] == 4 and p33["tsplit"] > 1  # odd T
    assert plan(pkg, L, (264, 2, 99), None, 33, STD)["path"] == "split_moments"
    assert plan(pkg, L, (264, 2, 99), None, 1, STD)["path"] == "copy"
    # float4 columns only for a unit channel step and nc % 4 == 0 (any offset)
    dims = (203, 3, 40)
    for w, cpl in (((3, 200, 1), 4), ((0, 200, 1), 4), ((0, 203, 1), 1), ((0, 100, 2), 1),
                   ((199, 200, -1), 1), ((1, 2, 1), 1), ((5, 4, 1), 4)):
        keep, wp = win(*w, 0, 3, 1, 0, 40, 1)
        for T in (8, 40):
            assert plan(pkg, L, dims, wp, T, MEDIAN)["cpl"] == cpl, (w, T)
            assert plan(pkg, L, dims, wp, T, VAR)["cpl"] == cpl, (w, T)
    # a launch too large for one grid
    info = (ctypes.c_int64 * 8)()
    rc = L.bldp_tstat_plan_f32(None, 1 << 20, 1, 1 << 24, None, 2, VAR, None, info)
    assert rc == pkg._lib.BLDP_EINVAL and "one launch" in pkg._lib.last_error()


def test_host_typed_path_is_float64(pkg):
    W = pkg.worker
    a = np.asfortranarray(np.array([[[1, 9, 4, 4, -7, 2]], [[3, 3, 10, -2, 5, 6]]], np.int16)
                          .reshape(2, 1, 6))
    r = W.getdata(a, tavby=2, tavfunc="median")
    assert r.dtype == np.float64 and r.shape == (2, 1, 3)
    assert np.array_equal(r[:, 0, :], [[5.0, 4.0, -2.5], [3.0, 4.0, 5.5]])
    r = W.getdata(a, tavby=3, tavfunc="var")
    assert r.dtype == np.float64
    np.testing.assert_allclose(r[:, 0, :], [[np.var([1, 9, 4], ddof=1), np.var([4, -7, 2], ddof=1)],
                                            [np.var([3, 3, 10], ddof=1), np.var([-2, 5, 6], ddof=1)]],
                               rtol=1e-15)
    np.testing.assert_allclose(W.getdata(a, tavby=3, tavfunc="std"), np.sqrt(r), rtol=1e-15)
    u = np.asfortranarray(np.array([200, 7, 255, 0, 0, 1, 9, 9, 3], np.uint8).reshape(1, 1, 9))
    r = W.getdata(u, tavby=3, tavfunc="median")  # an odd T: the middle element
    assert r.dtype == np.float64 and np.array_equal(r[0, 0], [200.0, 0.0, 9.0])
    # a reversed time range: the blocks follow the selected order
    J, C = pkg.JRange, pkg.COLON
    r = W.getdata(a, (C, C, J(6, -1, 3)), tavby=2, tavfunc="median")
    assert np.array_equal(r[:, 0, :], [[-2.5, 4.0], [5.5, 4.0]])
    r = W.getdata(a, (J(2, 2), C, J(1, 2, 5)), tavby=3, tavfunc="median")
    assert np.array_equal(r[:, 0, :], [[5.0]])
    with pytest.raises(pkg._lib.DimensionMismatch):
        W.getdata(a, tavby=4, tavfunc="median")
    with pytest.raises(pkg._lib.DimensionMismatch):
        W.getdata(a, (C, C, J(1, 5)), tavby=2, tavfunc="var")
    with pytest.raises(IndexError):
        W.getdata(a, (C, C, J(1, 8)), tavby=2, tavfunc="var")
    # stage 1 with a statistic, stage 2 with another: both on the host in Float64
    b = np.asfortranarray(np.arange(4 * 1 * 4, dtype=np.int32).reshape(4, 1, 4, order="F"))
    r = W.getdata(b, fqavby=2, fqavfunc="median", tavby=2, tavfunc="var")
    assert r.dtype == np.float64 and np.array_equal(r[:, 0, :], [[8.0, 8.0], [8.0, 8.0]])
    # _host_stat's axis: the channel form is what it was
    f = np.asfortranarray(np.arange(24, dtype=np.float64).reshape(4, 2, 3, order="F"))
    assert np.array_equal(W._host_stat(f, 2, "median"), (f[0::2] + f[1::2]) / 2)
    assert np.array_equal(W._host_stat(f, 3, "median", axis=2), f[:, :, 1:2])
    nan = f.copy(order="F")
    nan[1, 0, 2] = np.nan
    r = W._host_stat(nan, 3, "median", axis=2)
    assert np.isnan(r[1, 0, 0]) and np.isnan(r).sum() == 1


def test_keyword_rules(pkg, monkeypatch):
    W = pkg.worker
    a = np.asfortranarray(np.arange(48, dtype=np.int16).reshape(4, 2, 6, order="F"))
    # tavfunc=None is today's call: the same reduce, the same arguments
    calls = []
    monkeypatch.setattr(W, "_reduce_host", lambda *args: calls.append(args) or "result")
    assert W.getdata(a, fqavby=2, tavby=2) == "result"
    assert W.getdata(a, fqavby=2, tavby=2, tavfunc=None) == "result"
    assert len(calls) == 2 and calls[0][1:] == calls[1][1:] == (2, 2, "sum", None, 0)
    monkeypatch.undo()
    # ... including its errors: a statistic as fqavfunc has no time integration
    for kw in ({}, {"tavfunc": None}):
        with pytest.raises(TypeError, match="tavby"):
            W.getdata(a, fqavfunc="median", tavby=2, **kw)
        with pytest.raises(TypeError, match="tavby"):
            W.getdata(a.astype(np.float32), fqavfunc="median", tavby=2, **kw)
    # tavby <= 1: stage 2 is skipped whatever tavfunc is (fqav's n <= 1 rule)
    s1 = W.getdata(a, fqavby=2, fqavfunc="median")
    for t in (1, 0):
        r = W.getdata(a, fqavby=2, fqavfunc="median", tavby=t, tavfunc="median")
        assert r.dtype == s1.dtype and np.array_equal(r, s1)
    r = W.getdata(a, tavby=1, tavfunc="std")
    assert r.dtype == np.int16 and np.array_equal(r, a)
    # names and callables that _opname maps; anything else is refused
    assert np.array_equal(W.getdata(a, tavby=1, tavfunc=max), a)
    with pytest.raises(ValueError):
        W.getdata(a, tavby=2, tavfunc="mode")
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata(a, tavby=2, tavfunc=np.ptp)
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata(a, fqavby=2, fqavfunc=np.ptp, tavby=2, tavfunc="median")
    with pytest.raises(TypeError, match="tavfunc"):
        pkg.GBT.getband([0], ["no_such_file.fil"], tavby=2, tavfunc=np.ptp)  # before any read


def test_engine_checks_without_a_device(pkg):
    eng = pkg.engine
    with pytest.raises(pkg._lib.ArgumentError, match="reduce"):
        eng.tstat_host(np.zeros((4, 1, 4), np.float32, order="F"), 2, "sum")
    with pytest.raises(TypeError):
        eng.tstat_host(np.zeros((4, 1, 4), np.float64, order="F"), 2, "var")
    with pytest.raises(pkg._lib.DimensionMismatch):
        eng.tstat_host(np.zeros((4, 1, 4), np.float32, order="F"), 3, "var")
    assert eng.tstat_host(np.zeros((4, 1, 0), np.float32, order="F"), 2, "var").shape == (4, 1, 0)


def test_julia_shim_and_docs():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    assert "function gpu_tstat" in src and "export" in src and "gpu_tstat" in src.split("export")[1]
    assert re.search(r"ccall\(\(:bldp_tstat_f32, libbldp\)", src)
    assert re.search(r"ccall\(\(:bldp_tstat_host_f32, libbldp\)", src)
    for fn in ("getdata", "getband"):
        sig = re.search(r"function %s\(.*?\)\n" % fn, src, re.S)
        assert sig and "tavfunc" in sig.group(0), fn
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    assert "tavfunc" in hdr
    assert "tavfunc" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "tstats.hip" in open(os.path.join(REPO, "DESIGN.md")).read()
