"""CPU: the host side of getkurtosis(...; tblock) — the five additive entry
points of the C ABI (shape, plan and argument checks are pure host functions
of libbldp_hip), the Python keyword's errors, and the Julia shim."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

NEW = ("bldp_kurtosis_blocks_f32", "bldp_band_kurtosis_blocks_f32",
       "bldp_kurtosis_blocks_host_f32", "bldp_kurtosis_blocks_plan_f32",
       "bldp_kurtosis_blocks_shape")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def win(*w):
    a = (ctypes.c_int64 * 9)(*w)
    return a, ctypes.cast(a, ctypes.c_void_p)


def shape(L, dims, w, tblock):
    d = (ctypes.c_int64 * 3)(-1, -1, -1)
    rc = L.bldp_kurtosis_blocks_shape(*dims, w, tblock, d)
    return rc, tuple(d)


def plan(pkg, L, dims, w, tblock):
    info = (ctypes.c_int64 * 4)()
    rc = L.bldp_kurtosis_blocks_plan_f32(None, *dims, w, tblock, info)
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
    assert re.search(r"#define BLDP_ABI_VERSION 5\b", hdr)


def test_shape_and_argument_checks(pkg, L):
    E = pkg._lib
    dims = (512, 1, 1024)
    assert shape(L, dims, None, 16) == (E.BLDP_OK, (512, 1, 64))
    assert shape(L, dims, None, 1024) == (E.BLDP_OK, (512, 1, 1))
    rc, _ = shape(L, dims, None, 3)
    assert rc == E.BLDP_EDIM and "tblock" in E.last_error()
    for bad in (0, -1):
        rc, _ = shape(L, dims, None, bad)
        assert rc == E.BLDP_EINVAL and "tblock" in E.last_error()
    # the blocks cut the selected spectra: offset 3, step 2, 100 of them
    keep, w = win(4, 252, 1, 0, 1, 1, 3, 100, 2)
    assert shape(L, dims, w, 25) == (E.BLDP_OK, (252, 1, 4))
    assert shape(L, dims, w, 16)[0] == E.BLDP_EDIM
    keep, w = win(0, 512, 1, 0, 1, 1, 1000, 32, 1)  # past the last spectrum
    assert shape(L, dims, w, 16)[0] == E.BLDP_EBOUNDS
    keep, w = win(0, 512, 1, 0, 1, 1, 5, 0, 1)  # no spectra: no blocks
    assert shape(L, dims, w, 16) == (E.BLDP_OK, (512, 1, 0))
    keep, w = win(0, 0, 1, 0, 1, 1, 0, 64, 1)  # no channels
    assert shape(L, dims, w, 16) == (E.BLDP_OK, (0, 1, 4))
    assert L.bldp_kurtosis_blocks_shape(*dims, None, 16, None) == E.BLDP_EINVAL


def test_plan_without_a_gpu(pkg, L):
    dims = (512, 1, 1024)
    assert plan(pkg, L, dims, None, 16) == \
        {"path": "regs", "fused": 1, "blocks": 64, "workspace_bytes": 0}
    assert plan(pkg, L, dims, None, 32)["path"] == "regs"
    assert plan(pkg, L, dims, None, 64) == \
        {"path": "leaf", "fused": 1, "blocks": 16, "workspace_bytes": 0}
    assert plan(pkg, L, dims, None, 1024) == \
        {"path": "leaf", "fused": 1, "blocks": 1, "workspace_bytes": 0}
    # more than one leaf of Julia's tree: block by block on the whole-window path
    p = plan(pkg, L, (512, 1, 2050), None, 1025)
    assert (p["path"], p["fused"], p["blocks"]) == ("leaf", 0, 2) and p["workspace_bytes"] > 0
    # the whole-window plan of one such block says the same path
    info = (ctypes.c_int64 * 4)()
    keep, w = win(0, 512, 1, 0, 1, 1, 0, 1025, 1)
    assert L.bldp_kurtosis_plan_f32(None, 512, 1, 2050, w, info) == 0
    assert pkg._lib.KURT_PATHS[info[0]] == p["path"]
    # a channel step leaves no float4 columns
    keep, w = win(0, 256, 2, 0, 1, 1, 0, 1024, 1)
    p = plan(pkg, L, dims, w, 16)
    assert (p["path"], p["fused"], p["blocks"]) == ("mid", 0, 64)
    keep, w = win(1, 257, 1, 0, 1, 1, 0, 1024, 1)
    assert plan(pkg, L, dims, w, 64)["fused"] == 0
    # the plan call makes the same checks as the shape call
    info = (ctypes.c_int64 * 4)()
    assert L.bldp_kurtosis_blocks_plan_f32(None, *dims, None, 3, info) == pkg._lib.BLDP_EDIM
    assert L.bldp_kurtosis_blocks_plan_f32(None, *dims, None, 0, info) == pkg._lib.BLDP_EINVAL
    assert L.bldp_kurtosis_blocks_plan_f32(None, *dims, None, 16, None) == pkg._lib.BLDP_EINVAL


def test_null_pointers_and_empty_results(pkg, L):
    E = pkg._lib
    dims = (512, 1, 1024)
    out = np.zeros(8, dtype=np.float64)
    assert L.bldp_kurtosis_blocks_f32(None, *dims, None, 16, out.ctypes.data, 512, 512,
                                      None) == E.BLDP_EINVAL
    assert "tblock" in E.last_error()
    a = np.zeros(8, dtype=np.float32)
    assert L.bldp_kurtosis_blocks_f32(a.ctypes.data, *dims, None, 16, None, 512, 512,
                                      None) == E.BLDP_EINVAL
    assert L.bldp_kurtosis_blocks_host_f32(0, None, *dims, None, 16, out.ctypes.data) == \
        E.BLDP_EINVAL
    assert L.bldp_kurtosis_blocks_host_f32(0, a.ctypes.data, *dims, None, 16, None) == \
        E.BLDP_EINVAL
    assert L.bldp_band_kurtosis_blocks_f32(1, None, *dims, None, 16, out.ctypes.data,
                                           None) == E.BLDP_EINVAL
    ptrs = (ctypes.c_void_p * 2)(0, 0)
    assert L.bldp_band_kurtosis_blocks_f32(2, ctypes.cast(ptrs, ctypes.c_void_p), *dims, None, 16,
                                           out.ctypes.data, None) == E.BLDP_EINVAL
    # argument errors come before the pointer checks
    assert L.bldp_kurtosis_blocks_f32(None, *dims, None, 3, None, 512, 512, None) == E.BLDP_EDIM
    assert L.bldp_kurtosis_blocks_host_f32(0, None, *dims, None, 0, None) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers (and no GPU)
    keep, w = win(0, 512, 1, 0, 1, 1, 5, 0, 1)
    assert L.bldp_kurtosis_blocks_f32(None, *dims, w, 16, None, 512, 512, None) == E.BLDP_OK
    assert L.bldp_kurtosis_blocks_host_f32(0, None, *dims, w, 16, None) == E.BLDP_OK
    assert L.bldp_band_kurtosis_blocks_f32(2, ctypes.cast(ptrs, ctypes.c_void_p), *dims, w, 16,
                                           None, None) == E.BLDP_OK


def test_python_keyword_errors_before_any_launch(pkg):
    import torch

    a = np.zeros((8, 1, 12), dtype=np.float32, order="F")
    W, eng = pkg.worker, pkg.engine
    with pytest.raises(pkg.DimensionMismatch, match="tblock"):
        W.getkurtosis(a, tblock=5)
    with pytest.raises(pkg.DimensionMismatch, match="tblock"):
        W.getkurtosis(a.astype(np.int16), tblock=5)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="tblock"):
            W.getkurtosis(a, tblock=bad)
        with pytest.raises(ValueError, match="tblock"):
            eng.kurtosis_host(a, tblock=bad)
    with pytest.raises(TypeError, match="tblock"):
        eng.kurtosis_host(a, tblock=2.5)
    # the blocks cut the selected spectra: 12 / 2 = 6 selected, 4 does not divide them
    idxs = (pkg.COLON, pkg.COLON, pkg.JRange(1, 2, 12))
    with pytest.raises(pkg.DimensionMismatch, match="tblock=4"):
        W.getkurtosis(a, idxs, tblock=4)
    # the tensor forms check before they look at the device
    x = torch.zeros((12, 1, 8)).permute(2, 1, 0)
    with pytest.raises(pkg.DimensionMismatch, match="tblock"):
        eng.kurtosis(x, tblock=5)
    with pytest.raises(ValueError, match="tblock"):
        eng.kurtosis(x, tblock=0)
    with pytest.raises(pkg.DimensionMismatch, match="tblock"):
        eng.kurtosis_blocks_plan(x, 5)


def test_julia_shim_has_the_keyword():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    assert "bldp_kurtosis_blocks_host_f32" in src
    sigs = re.findall(r"function gpu_kurtosis\((.*?)\)\s*(?:where|\n)", src, re.S)
    assert len(sigs) == 2
    for s in sigs:
        assert re.search(r"tblock::Union\{Nothing,\s*Integer\}\s*=\s*nothing", s), s
    assert re.search(r"Array\{Float64,\s*3\}\(undef, shp\.\.\.\)", src)
