"""CPU: the host side of getmoments — the four additive entry points of the C
ABI (plan and argument checks are pure host functions of libbldp_hip), the
Python layers' keyword and element-type errors, the Julia shim, and the
statement's own variance against the bounds of tests/moments_ref.py."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from moments_ref import PLANES, VAR_LEAF_TOL, var_statement, var_sum_tol

NEW = ("bldp_moments_plan_f32", "bldp_moments_f32", "bldp_band_moments_f32",
       "bldp_moments_host_f32")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def win(*w):
    a = (ctypes.c_int64 * 9)(*w)
    return a, ctypes.cast(a, ctypes.c_void_p)


def plan(pkg, L, name, dims, w, tblock):
    info = (ctypes.c_int64 * 4)()
    rc = getattr(L, name)(None, *dims, w, tblock, info)
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
    for name in ("moments", "band_moments", "moments_host", "moments_plan"):
        assert callable(getattr(pkg.engine, name)) and name in pkg.engine.__all__, name
    assert pkg.engine.Moments._fields == PLANES == pkg.engine.MOMENTS
    assert callable(pkg.WorkerFunctions.getmoments) and callable(pkg.GBT.getmoments)
    assert pkg.getmoments is pkg.WorkerFunctions.getmoments and "getmoments" in pkg.__all__
    assert "uncorrected" in pkg.WorkerFunctions.getmoments.__doc__.lower()
    assert "uncorrected" in pkg.engine.moments.__doc__.lower()


@pytest.mark.parametrize("tblock", [0, 16])
@pytest.mark.parametrize("nc", [8, 6])
@pytest.mark.parametrize("nt", [16, 33, 512, 513, 2049])
def test_plan_is_the_skewness_plan(pkg, L, nt, nc, tblock):
    """With null pointers and no GPU: path, form and block count are
    bldp_skewness_plan_f32's, and so is the workspace wherever the plan holds
    nothing per moment.  Two plans do: the two-pass path keeps three partial
    sums per time chunk where skewness keeps two (half as much again of that
    region), and the block-by-block form stages a block's four planes where
    skewness stages one (three more (nc, ni) Float64 planes).  Those are
    checked at exactly that size."""
    ni = 2
    nsel = nt if tblock == 0 else -(-nt // tblock) * tblock  # (blocks: nt rounded up to whole ones)
    dims = (nc, ni, 3 * nsel)
    keep, w = win(0, nc, 1, 0, ni, 1, 0, nsel, 1)
    s = plan(pkg, L, "bldp_skewness_plan_f32", dims, w, tblock)
    m = plan(pkg, L, "bldp_moments_plan_f32", dims, w, tblock)
    for k in ("path", "fused", "blocks"):
        assert m[k] == s[k], (k, m, s)
    if tblock == 0:
        want = {16: "regs", 33: "mid", 512: "mid", 513: "leaf", 2049: "leaf"}[nt]
        if nc == 6:  # no float4 columns
            want = "mid" if nt <= 512 else "twopass"
        assert m["path"] == want and (m["fused"], m["blocks"]) == (1, 1)
    else:
        assert m["blocks"] == nsel // tblock and m["fused"] == (1 if nc == 8 else 0)
    extra = m["workspace_bytes"] - s["workspace_bytes"]
    if tblock and not m["fused"]:
        assert extra == 3 * nc * ni * 8, (m, s)  # a block's three further planes
    elif m["path"] == "twopass":
        # skewness' region of 2 partials per chunk is the last of its workspace;
        # a third partial adds half of it (regions are rounded up to 256 bytes)
        def region(parts, c):
            return -(-(parts * c * nc * ni * 8) // 256) * 256

        assert extra > 0 and any(region(3, c) - region(2, c) == extra for c in range(2, 4096)), \
            (m, s)
    else:
        assert extra == 0, (m, s)


def test_error_codes(pkg, L):
    E = pkg._lib
    dims = (512, 1, 1024)
    info = (ctypes.c_int64 * 4)()
    out = np.zeros(4 * 512 * 64, dtype=np.float64)
    o = [out[q * 512 * 64:].ctypes.data for q in range(4)]
    a = np.zeros(512 * 1024, dtype=np.float32)
    ptrs = (ctypes.c_void_p * 2)(0, 0)
    pp = ctypes.cast(ptrs, ctypes.c_void_p)
    N4 = (None, None, None, None)

    def every(w, tblock, code):
        assert L.bldp_moments_plan_f32(None, *dims, w, tblock, info) == code
        assert L.bldp_moments_f32(None, *dims, w, tblock, *N4, 512, 512, None) == code
        assert L.bldp_band_moments_f32(2, pp, *dims, w, tblock, *N4, None) == code
        assert L.bldp_moments_host_f32(0, None, *dims, w, tblock, *N4) == code

    every(None, 3, E.BLDP_EDIM)  # nt % M != 0
    assert "tblock" in E.last_error()
    every(None, -1, E.BLDP_EINVAL)  # M < 0
    assert "tblock" in E.last_error()
    keep, w = win(0, 512, 1, 0, 1, 1, 1000, 32, 1)  # past the last spectrum
    every(w, 0, E.BLDP_EBOUNDS)
    every(w, 16, E.BLDP_EBOUNDS)
    assert L.bldp_moments_plan_f32(None, *dims, None, 0, None) == E.BLDP_EINVAL
    for M in (0, 16):
        # null in for a non-empty result
        assert L.bldp_moments_f32(None, *dims, None, M, *o, 512, 512, None) == E.BLDP_EINVAL
        assert L.bldp_moments_host_f32(0, None, *dims, None, M, *o) == E.BLDP_EINVAL
        assert L.bldp_band_moments_f32(1, None, *dims, None, M, *o, None) == E.BLDP_EINVAL
        assert L.bldp_band_moments_f32(2, pp, *dims, None, M, *o, None) == E.BLDP_EINVAL
        # all four planes null
        assert L.bldp_moments_f32(a.ctypes.data, *dims, None, M, *N4, 512, 512,
                                  None) == E.BLDP_EINVAL
        assert "null" in E.last_error()
        assert L.bldp_moments_host_f32(0, a.ctypes.data, *dims, None, M, *N4) == E.BLDP_EINVAL
        one = (ctypes.c_void_p * 1)(a.ctypes.data)
        assert L.bldp_band_moments_f32(1, ctypes.cast(one, ctypes.c_void_p), *dims, None, M, *N4,
                                       None) == E.BLDP_EINVAL
        # planes that overlap each other (one element apart, and the same plane twice)
        for q, r in ((0, 1), (1, 3), (2, 3)):
            pl = [None] * 4
            pl[q], pl[r] = o[0], o[0] + 8
            assert L.bldp_moments_f32(a.ctypes.data, *dims, None, M, *pl, 512, 512,
                                      None) == E.BLDP_EINVAL
            assert "overlap" in E.last_error()
            pl[r] = o[0]
            assert L.bldp_moments_host_f32(0, a.ctypes.data, *dims, None, M, *pl) == E.BLDP_EINVAL
            assert "overlap" in E.last_error()
        # a plane inside the input array
        inside = a.ctypes.data + 4096
        assert L.bldp_moments_f32(a.ctypes.data, *dims, None, M, None, inside, None, None, 512,
                                  512, None) == E.BLDP_EINVAL
        assert "overlap" in E.last_error()
    # overlapping strides
    assert L.bldp_moments_f32(a.ctypes.data, *dims, None, 16, *o, 511, 512, None) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers (and no GPU)
    keep, w = win(0, 0, 1, 0, 1, 1, 0, 64, 1)  # no channels
    for M in (0, 16):
        assert L.bldp_moments_f32(None, *dims, w, M, *N4, 512, 512, None) == E.BLDP_OK
        assert L.bldp_moments_host_f32(0, None, *dims, w, M, *N4) == E.BLDP_OK
        assert L.bldp_band_moments_f32(2, pp, *dims, w, M, *N4, None) == E.BLDP_OK
    keep, w = win(0, 512, 1, 0, 1, 1, 5, 0, 1)  # no spectra: no blocks
    assert L.bldp_moments_f32(None, *dims, w, 16, *N4, 512, 512, None) == E.BLDP_OK
    assert plan(pkg, L, "bldp_moments_plan_f32", dims, w, 16)["blocks"] == 0


def test_python_keyword_and_type_errors_before_any_launch(pkg):
    import torch

    a = np.zeros((8, 1, 12), dtype=np.float32, order="F")
    W, eng = pkg.worker, pkg.engine
    x = torch.zeros((12, 1, 8)).permute(2, 1, 0)
    calls = (lambda **k: W.getmoments(a, **k), lambda **k: eng.moments_host(a, **k),
             lambda **k: eng.moments(x, **k), lambda **k: eng.band_moments([x, x], **k),
             lambda **k: W.getmoments(x, **k))
    for f in calls + (lambda **k: eng.moments_plan(x, **k),):
        for bad in (True, 2.5):  # bool, non-integer
            with pytest.raises(TypeError, match="tblock"):
                f(tblock=bad)
        for bad in (-1, 0):  # (tblock=None is the whole window)
            with pytest.raises(ValueError, match="tblock"):
                f(tblock=bad)
        with pytest.raises(pkg.DimensionMismatch, match="tblock=5"):  # non-divisor
            f(tblock=5)
    for f in calls:  # which: names of planes, at least one
        for bad in (("mean", "variance"), "kurt", ()):
            with pytest.raises(ValueError, match="which"):
                f(which=bad)
    with pytest.raises(ValueError, match="which"):  # before the file is touched
        W.getmoments("/nonexistent/file.fil", which=("median",))
    idxs = (pkg.COLON, pkg.COLON, pkg.JRange(1, 2, 12))  # 6 selected spectra
    with pytest.raises(pkg.DimensionMismatch, match="tblock=4"):
        W.getmoments(a, idxs, tblock=4)
    # anything but Float32 is a TypeError naming Float32
    for dt in (np.int16, np.uint8, np.float64):
        b = a.astype(dt)
        t = torch.from_numpy(np.ascontiguousarray(b.transpose(2, 1, 0))).permute(2, 1, 0)
        for f in (lambda: W.getmoments(b), lambda: eng.moments_host(b),
                  lambda: W.getmoments(b, tblock=4), lambda: W.getmoments(t),
                  lambda: eng.moments(t), lambda: eng.band_moments([t]),
                  lambda: W.getmoments(b, which=("var",))):
            with pytest.raises(TypeError, match="Float32"):
                f()


def test_eight_bit_sigproc_file_is_a_type_error(pkg, tmp_path):
    a = np.asfortranarray(np.arange(8 * 12, dtype=np.uint8).reshape((8, 1, 12), order="F"))
    fil = str(tmp_path / "u8.fil")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=8, nifs=1, tsamp=1.0, nbits=8,
                                    telescope_id=6, machine_id=10, data_type=1, tstart=59000.0,
                                    source_name="X"), a)
    with pytest.raises(TypeError, match="Float32"):
        pkg.WorkerFunctions.getmoments(fil)


def test_julia_shim_ccall_agrees_with_the_header():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    assert re.search(r"function gpu_moments\(A::Array\{Float32,3\};[^\n]*\n\s*tblock::Integer=0\)",
                     src)
    assert re.search(r"export[^\n]*\n[^\n]*gpu_moments", src)
    assert re.search(r"\(mean=m, var=v, skewness=s, kurtosis=k\)", src)
    call = re.search(r"ccall\(\(:bldp_moments_host_f32, libbldp\), Cint,\s*\(([^()]*)\)", src, re.S)
    assert " ".join(call.group(1).split()) == \
        ("Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, "
         "Ptr{Float64}, Ptr{Float64}")
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    decl = re.search(r"BLDP_API int bldp_moments_host_f32\(([^)]*)\)", hdr, re.S)
    types = [" ".join(p.split()[:-1]) for p in " ".join(decl.group(1).split()).split(",")]
    assert types == ["int", "const float", "int64_t", "int64_t", "int64_t", "const int64_t",
                     "int64_t", "double", "double", "double", "double"]


def test_the_statements_own_variance_sits_inside_the_bounds(orc):
    """NumPy's cm2 / n with Float32 z and z2 against an exact-Float64-z
    evaluation about the same m (what the leaf class differs by) and against an
    8-partial reordering of its own terms (the sum class), on gamma rows of
    mean / sigma 1.4 .. 30000 and a row of one value and an ulp."""
    rng = np.random.default_rng(5)
    R = np.array([np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0])
    for nt in (33, 513, 4096):
        a = np.empty((6, 1, nt), dtype=np.float32, order="F")
        a[:5, 0] = rng.gamma((R ** 2)[:, None], (1e6 / R ** 2)[:, None], (5, nt))
        a[5, 0] = np.float32(2.0 ** 20) + np.float32(0.125) * rng.integers(0, 2, nt)
        v = var_statement(orc, a)[:, 0]
        assert np.isfinite(v).all() and (v > 0).all()
        m32 = orc.mean_f32(a)[:, 0][:, None]
        z = a[:, 0].astype(np.float64) - m32.astype(np.float64)
        exact = (z ** 2).sum(axis=1) / nt
        leaf = np.abs(exact - v) / (VAR_LEAF_TOL * v)
        z32 = (a[:, 0] - m32).astype(np.float32)
        q = (z32 * z32).astype(np.float32).astype(np.float64)
        parts = np.array_split(np.arange(nt), 8)
        re8 = sum(np.add.accumulate(q[:, p], axis=1)[:, -1] for p in parts) / nt
        summ = np.abs(re8 - v) / (var_sum_tol(nt) * v)
        print(f"var statement nt={nt}: worst error / bound leaf {leaf.max():.3g}, "
              f"sum {summ.max():.3g}")
        assert (leaf <= 1.0).all(), (nt, leaf)
        assert (summ <= 1.0).all(), (nt, summ)
