"""CPU: fold and unfold without a GPU: the NumPy restatement on windows written
out by hand, bldp_fold_shape, the plan entry points with null pointers, every
refusal of the rule (include/bldp.h) with pointers that are never dereferenced,
which kernels the GPU cases of tests/fold_cases.py run (from the plan alone), the
Python argument checks, and the symbols."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import fold_cases as fc
from fold_ref import fold_ref, unfold_ref

NAMES = ("bldp_fold_shape", "bldp_fold_plan_f32", "bldp_fold_f32", "bldp_band_fold_f32",
         "bldp_fold_host_f32", "bldp_unfold_plan_f32", "bldp_unfold_f32", "bldp_band_unfold_f32",
         "bldp_unfold_host_f32")
NAN, INF = np.float32(np.nan), np.float32(np.inf)
CSRC = os.path.join(REPO, "bldistributeddataproducts.jl_amd", "csrc")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---- the restatement, on windows written out by hand ---------------------------------
def test_restatement_by_hand():
    # nfpc = 4, J = 2, nt = 3: channel c = 4 j + k holds 10 c + t
    a = (10 * np.arange(8)[:, None, None] + np.arange(3)[None, None, :]).astype(np.float32)
    s, k, s32, mean = fold_ref(a, 4)            # T = nt
    assert s.shape == (4, 1, 1) and (k == 6).all()
    # k = 1: channels 1 and 5 over three spectra: 10+11+12 + 50+51+52
    assert s[1, 0, 0] == 186 and s32.dtype == np.float32 and mean[1, 0, 0] == np.float32(31)
    s, k, _, _ = fold_ref(a, 4, 1)              # T = 1: over the coarse channels alone
    assert s.shape == (4, 1, 3) and (k == 2).all() and s[2, 0, 1] == 21 + 61
    s, k, _, _ = fold_ref(a, 8, 3)              # nfpc = nc: J = 1, over time alone
    assert s.shape == (8, 1, 1) and s[7, 0, 0] == 70 + 71 + 72
    # the DC spike at fine bin nfpc / 2 of every coarse channel comes out in the profile,
    # and the unfold takes it out
    b = np.ones((8, 1, 2), np.float32)
    b[2::4] = 10
    _, _, _, mean = fold_ref(b, 4)
    assert mean.ravel().tolist() == [1, 1, 10, 1]
    assert (unfold_ref(b, mean, 4) == 1).all() and (unfold_ref(b, mean, 4, how="subtract") == 0).all()
    # a mask: flagged NaN and Inf leave the result finite; a kept NaN propagates to its k alone
    c = a.copy()
    c[1, 0, 0], c[5, 0, 1], c[2, 0, 2] = NAN, INF, NAN
    m = np.zeros(a.shape, np.uint8)
    m[1, 0, 0], m[5, 0, 1] = 1, 255
    s, k, s32, mean = fold_ref(c, 4, mask=m)
    assert s[1, 0, 0] == 186 - 10 - 51 and k[1, 0, 0] == 4 and mean[1, 0, 0] == np.float32(125 / 4)
    assert np.isnan(s32[2, 0, 0]) and np.isfinite(s32[[0, 1, 3]]).all()
    # a block with nothing kept: 0.0 and NaN
    m[:] = 0
    m[3::4] = 2
    s, k, s32, mean = fold_ref(a, 4, mask=m)
    assert s32[3, 0, 0] == 0 and not np.signbit(s32[3, 0, 0]) and k[3, 0, 0] == 0
    assert np.isnan(mean[3, 0, 0]) and mean.dtype == np.float32
    # a bad-channel list broadcasts
    bad = np.zeros((8, 1, 1), np.uint8)
    bad[4] = 1
    assert fold_ref(a, 4, mask=bad)[1].ravel().tolist() == [3, 6, 6, 6]
    # the mean is the Float64 quotient rounded once
    d = np.array([1, 1, 0], np.float32).reshape(3, 1, 1)
    assert fold_ref(d, 1)[3][0, 0, 0] == np.float32(2 / 3)
    # unfold: IEEE results for a zero, infinite or NaN profile value
    p = np.array([0, INF, NAN, 2], np.float32).reshape(4, 1, 1)
    u = unfold_ref(np.full((4, 1, 1), 3, np.float32), p, 4)
    assert u[0, 0, 0] == INF and u[1, 0, 0] == 0 and np.isnan(u[2, 0, 0]) and u[3, 0, 0] == 1.5
    # t div T picks the profile's time block
    p2 = np.array([[[1, 2]]], np.float32)
    assert unfold_ref(np.full((2, 1, 4), 8, np.float32), p2, 1, 2)[1, 0].tolist() == [8, 8, 4, 4]


# ---- bldp_fold_shape ------------------------------------------------------------------
def test_fold_shape(pkg, L):
    E = pkg._lib
    d = (ctypes.c_int64 * 3)()
    assert L.bldp_fold_shape(64, 2, 12, None, 8, 4, d) == 0 and list(d) == [8, 2, 3]
    assert L.bldp_fold_shape(64, 2, 12, None, 64, 0, d) == 0 and list(d) == [64, 2, 12]
    keep, wp = E.win_arg([1, 30, 2, 1, 1, 1, 11, 6, -2])
    assert L.bldp_fold_shape(64, 2, 12, wp, 3, 6, d) == 0 and list(d) == [3, 1, 1]
    assert L.bldp_fold_shape(64, 2, 12, None, 0, 1, d) == E.BLDP_EINVAL
    assert L.bldp_fold_shape(64, 2, 12, None, 5, 1, d) == E.BLDP_EDIM and "nfpc=5" in E.last_error()
    assert L.bldp_fold_shape(64, 2, 12, None, 8, 5, d) == E.BLDP_EDIM and "tavby=5" in E.last_error()
    assert L.bldp_fold_shape(64, 2, 12, None, 8, 4, None) == E.BLDP_EINVAL
    keep, wp = E.win_arg([0, 0, 1, 0, 2, 1, 0, 12, 1])  # an empty window
    assert L.bldp_fold_shape(64, 2, 12, wp, 8, 4, d) == 0 and list(d) == [0, 2, 3]


# ---- the plan calls: null pointers, no GPU -------------------------------------------
KEYS = ["path", "lanes", "chunks", "wgs", "ws", "launches", "mload", "vec", "nout", "cu"]


def plan(pkg, L, dims, nfpc, T, win=None, ptr=None, mask=None, ld=None):
    info = (ctypes.c_int64 * 10)(*([-1] * 10))
    keep, wp = pkg._lib.win_arg(win)
    mld = (ctypes.c_int64 * 3)(*ld) if ld is not None else None
    rc = L.bldp_fold_plan_f32(ptr, *dims, wp, nfpc, T, mask, mld, info)
    assert rc == 0, pkg._lib.last_error()
    d = dict(zip(KEYS, [int(v) for v in info]))
    d["path"] = pkg._lib.FOLD_PATHS[d["path"]]
    d["mload"] = pkg._lib.FOLD_MASK_LOADS[d["mload"]]
    # one launch and no workspace, or the merge behind the fold and its partials
    if d["nout"]:  # (an empty window reports zeros)
        assert (d["launches"], d["ws"]) == ((1, 0) if d["chunks"] == 1 else
                                            (2, d["chunks"] * d["nout"] * 12))
    return d


def test_plan_product_shapes(pkg, L):
    # one 0000 bank: 262144 float4 columns fill the device in one launch
    p = plan(pkg, L, (64 * 1048576, 1, 16), 1048576, 16)
    assert (p["path"], p["vec"], p["lanes"], p["chunks"], p["wgs"]) == ("cols", 1, 256, 1, 1024)
    assert p["mload"] == "none" and p["nout"] == 1048576
    # one 0002 bank and the band of 8: one workgroup of columns, so (j, tt) is chunked
    for J in (64, 512):
        p = plan(pkg, L, (J * 1024, 1, 272), 1024, 272, ld=[1, J * 1024, J * 1024])
        assert (p["path"], p["vec"], p["mload"], p["nout"]) == ("cols", 1, "dword", 1024)
        assert p["chunks"] > 256 and p["wgs"] == p["chunks"] and p["cu"] >= 16
        assert (p["chunks"] - 1) * p["cu"] < J * 272 <= p["chunks"] * p["cu"]  # no empty chunk
    # one 0001 bank: lanes along c over the 64 coarse channels of a row, time chunked
    p = plan(pkg, L, (512, 1, 879616), 8, 879616, ld=[1, 0, 0])
    assert (p["path"], p["vec"], p["lanes"], p["mload"], p["nout"]) == ("rows", 1, 128, "dword", 8)
    assert p["chunks"] > 1024 and (p["chunks"] - 1) * p["cu"] < 879616 <= p["chunks"] * p["cu"]
    # anything else: nfpc = 3, a channel step, a window off the float4 boundary
    assert plan(pkg, L, (192, 2, 16), 3, 16)["vec"] == 0
    assert plan(pkg, L, (128, 2, 16), 8, 16, win=[0, 64, 2, 0, 2, 1, 0, 16, 1])["vec"] == 0
    assert plan(pkg, L, (128, 2, 16), 8, 16, win=[1, 64, 1, 0, 2, 1, 0, 16, 1])["vec"] == 0
    assert plan(pkg, L, (128, 2, 16), 8, 16, win=[4, 64, 1, 0, 2, 1, 0, 16, 1])["vec"] == 1
    assert plan(pkg, L, (128, 2, 16), 8, 16, ptr=(1 << 20) + 4)["vec"] == 0
    assert plan(pkg, L, (130, 2, 16), 8, 16, win=[0, 64, 1, 0, 2, 1, 0, 16, 1])["vec"] == 0
    assert plan(pkg, L, (130, 1, 1), 8, 1, win=[0, 64, 1, 0, 1, 1, 0, 1, 1])["vec"] == 1
    # the mask's forms
    dims, ld = (256, 2, 16), [1, 256, 512]
    assert plan(pkg, L, dims, 8, 4, ld=ld)["mload"] == "dword"
    assert plan(pkg, L, dims, 8, 4, mask=(1 << 20) + 4, ld=ld)["mload"] == "dword"
    assert plan(pkg, L, dims, 8, 4, mask=(1 << 20) + 1, ld=ld)["mload"] == "byte"
    assert plan(pkg, L, dims, 8, 4, mask=(1 << 20))["mload"] == "dword"  # NULL strides: dense
    assert plan(pkg, L, dims, 8, 4, ld=[1, 258, 516])["mload"] == "byte"
    assert plan(pkg, L, dims, 8, 4, ld=[2, 512, 1024])["mload"] == "byte"
    assert plan(pkg, L, dims, 8, 4, ld=[0, 0, 1])["mload"] == "row"
    assert plan(pkg, L, dims, 8, 4, ld=[0, 1, 0])["mload"] == "row"
    assert plan(pkg, L, dims, 8, 4, ld=[1, 0, 0])["mload"] == "dword"
    assert plan(pkg, L, dims, 3, 4, win=[0, 255, 1, 0, 2, 1, 0, 16, 1], ld=ld)["mload"] == "byte"
    assert plan(pkg, L, dims, 8, 4)["mload"] == "none"


def test_plan_huge_and_empty_windows(pkg, L):
    # 2^44 elements, both paths
    p = plan(pkg, L, (1 << 22, 1, 1 << 22), 1 << 20, 1 << 22)
    assert (p["path"], p["chunks"], p["wgs"], p["nout"]) == ("cols", 1, 1024, 1 << 20)
    p = plan(pkg, L, (1 << 13, 2, 1 << 30), 8, 1 << 20)
    assert (p["path"], p["chunks"], p["wgs"], p["nout"]) == ("rows", 1, 2048, 8 * 2 * 1024)
    info = (ctypes.c_int64 * 4)(*([-1] * 4))
    assert L.bldp_unfold_plan_f32(None, 1 << 22, 1, 1 << 22, None, 1 << 20, 1 << 22, None, 1 << 20,
                                  1 << 20, None, 1 << 22, 1 << 22, info) == 0
    assert list(info) == [1, 1 << 20, 4, 0]
    # an empty window plans without a fault and reports nothing
    p = plan(pkg, L, (256, 1, 4), 8, 1, win=[0, 0, 1, 0, 1, 1, 0, 4, 1])
    assert p["nout"] == 0 and p["wgs"] == 0


def unfold_plan(pkg, L, dims, nfpc, T, win=None, ptr=None, prof=None, out=None, pld=None,
                old=None):
    info = (ctypes.c_int64 * 4)(*([-1] * 4))
    keep, wp = pkg._lib.win_arg(win)
    nc, ni, nt = (win[1], win[4], win[7]) if win else dims
    pld = pld or (nfpc, nfpc * ni)
    old = old or (nc, nc * ni)
    rc = L.bldp_unfold_plan_f32(ptr, *dims, wp, nfpc, T, prof, pld[0], pld[1], out, old[0], old[1],
                                info)
    assert rc == 0, pkg._lib.last_error()
    assert info[2] == (4 if info[0] else 1 if info[1] else 0) and info[3] == 0
    return int(info[0]), int(info[1])


def test_unfold_plan(pkg, L):
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2) == (1, 1)            # 16 * 2 * 6 float4s
    assert unfold_plan(pkg, L, (4096, 2, 6), 8, 2) == (1, 48)
    assert unfold_plan(pkg, L, (60, 2, 6), 3, 2) == (0, 3)             # nfpc = 3: scalar
    assert unfold_plan(pkg, L, (128, 2, 6), 8, 2, win=[1, 64, 1, 0, 2, 1, 0, 6, 1])[0] == 0
    assert unfold_plan(pkg, L, (128, 2, 6), 8, 2, win=[0, 64, 2, 0, 2, 1, 0, 6, 1])[0] == 0
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, ptr=(1 << 20) + 4)[0] == 0
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, prof=(1 << 20) + 4)[0] == 0
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, out=(1 << 20) + 8)[0] == 0
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, out=(1 << 20) + 16)[0] == 1
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, old=(66, 132))[0] == 0   # a pitch off the grid
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, old=(68, 136))[0] == 1   # a slot of a wider band
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, pld=(10, 20))[0] == 0
    assert unfold_plan(pkg, L, (64, 2, 6), 8, 2, win=[0, 0, 1, 0, 2, 1, 0, 6, 1]) == (0, 0)


# ---- which kernels the GPU cases run, from the plan alone ------------------------------
def compiled_instantiations():
    """Every kernel instantiation fold.hip compiles, read from its dispatch tables."""
    src = open(os.path.join(CSRC, "fold.hip")).read()
    table = src[src.index("void (*fold_kernel(bool vec, int mf))"):src.index("}  // namespace\n")]
    forms = re.findall(r"return k_fold<ROWS, (true|false), (\d)>;", table)
    assert len(forms) == len(set(forms)) == 7
    rows = set(re.findall(r"fold_kernel<(true|false)>\(", src))
    assert rows == {"true", "false"}
    out = {"k_fold<%s, %s, %s>" % (r, v, m) for r in rows for v, m in forms}
    out |= {"k_unfold<%s>" % v for v in re.findall(r"launch_kernel\(k_unfold<(true|false)>", src)}
    assert "launch_kernel(k_fold_merge" in src
    out.add("k_fold_merge")
    # (nothing else is a kernel of the file)
    assert len(re.findall(r"__global__", src)) == 3
    return out


def case_plan(pkg, L, c):
    addr, ld = fc.mask_ld(c)
    return plan(pkg, L, fc.array_shape(c), c.nfpc, c.T or c.nt, win=fc.window(c), mask=addr, ld=ld)


def test_cases_reach_every_instantiation(pkg, L):
    named, ids = set(), set()
    seen = {k: set() for k in ("path", "mload", "vec", "chunked")}
    for c in fc.CASES:
        assert fc.case_id(c) not in ids
        ids.add(fc.case_id(c))
        n = np.prod(fc.array_shape(c))
        assert n <= 4 << 20, fc.case_id(c)
        p = case_plan(pkg, L, c)
        got = (p["path"], p["vec"], p["mload"], p["chunks"] > 1)
        assert got == c.plan, (fc.case_id(c), got)
        for k, v in zip(("path", "vec", "mload", "chunked"), got):
            seen[k].add(v)
        mf = {"byte": 0, "dword": 1, "row": 2, "none": 3}[p["mload"]]
        named.add("k_fold<%s, %s, %d>" % (str(p["path"] == "rows").lower(), str(bool(p["vec"])).lower(),
                                          mf))
        if p["chunks"] > 1:
            named.add("k_fold_merge")
    assert seen == {"path": {"cols", "rows"}, "mload": {"byte", "dword", "row", "none"},
                    "vec": {0, 1}, "chunked": {False, True}}
    for c, vec in fc.UNFOLD_CASES:
        got = unfold_plan(pkg, L, fc.array_shape(c), c.nfpc, c.T or c.nt, win=fc.window(c))[0]
        assert got == vec, fc.case_id(c)
        named.add("k_unfold<%s>" % str(bool(vec)).lower())
    compiled = compiled_instantiations()
    assert named == compiled, (sorted(compiled - named), sorted(named - compiled))
    # the shapes the issue names are all there
    assert {c.nfpc for c in fc.CASES} >= {1, 2, 3, 4, 5, 8, 12, 64, 256, 1024, 1028, 2048, 4100}
    assert {c.J for c in fc.CASES} >= {1, 2, 3, 7, 64} and {c.ni for c in fc.CASES} == {1, 2}
    assert {c.T for c in fc.CASES} >= {1, 2, 3, 16, 17, None}
    assert {c.win for c in fc.CASES} == {"full", "c0", "cs2", "rev", "ts3", "if1"}
    assert {c.mask for c in fc.CASES} >= {None, "zero", "all", "random", "odd_address",
                                          "bad_channels", "bad_spectra", "bool"}
    for shape in ((8, 4, 2, 4099, None), (4, 1, 1, 20000, None), (1024, 5, 1, 273, None)):
        assert any(c[:5] == shape and c.plan[3] for c in fc.CASES), shape


# ---- the refusals, before any launch ---------------------------------------------------
def test_fold_refusals(pkg, L):
    E = pkg._lib
    A, M, O, K = 1 << 20, 2 << 20, 3 << 20, 4 << 20  # never dereferenced
    info = (ctypes.c_int64 * 10)()

    def run(in_=A, dims=(64, 2, 4), nfpc=16, T=2, op=0, mask=M, ld=None, out=O, kept=K, ld_i=16,
            ld_t=32, win=None):
        keep, wp = E.win_arg(win)
        mld = (ctypes.c_int64 * 3)(*ld) if ld is not None else None
        return L.bldp_fold_f32(in_, *dims, wp, nfpc, T, op, mask, mld, out, kept, ld_i, ld_t, None)

    for nfpc in (0, -1):
        assert run(nfpc=nfpc) == E.BLDP_EINVAL and "nfpc" in E.last_error()
    for op in (2, 3, 4, 5, 6, 7, 8, -1, 64):
        assert run(op=op) == E.BLDP_EINVAL and "sum" in E.last_error()
    # J * T = 2^31 is beyond Int32; 2^31 - 2^16 is not
    assert L.bldp_fold_plan_f32(None, 65536, 1, 32768, None, 1, 32768, None, None,
                                info) == E.BLDP_EINVAL and "2^31" in E.last_error()
    assert L.bldp_fold_plan_f32(None, 65536, 1, 32767, None, 1, 32767, None, None, info) == 0
    assert L.bldp_fold_plan_f32(None, 64, 1, 4, None, 4, 1, None, None, None) == E.BLDP_EINVAL
    # both outputs null, a null input; a null mask keeps everything and is no refusal
    assert run(out=None, kept=None) == E.BLDP_EINVAL and "both null" in E.last_error()
    assert run(in_=None) == E.BLDP_EINVAL and "null input" in E.last_error()
    for ld in ([-1, 64, 128], [1, -64, 128], [1, 64, -128]):
        assert run(ld=ld) == E.BLDP_EINVAL and "negative" in E.last_error()
    # outputs over each other, over the input window, over the mask's span
    nout_bytes = 4 * (16 * 2 * 2)
    assert run(kept=O + nout_bytes - 4) == E.BLDP_EINVAL and "out and kept" in E.last_error()
    assert run(out=A + 4 * (64 * 2 * 4) - 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(kept=A) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(out=M + 64 * 2 * 4 - 1) == E.BLDP_EINVAL and "the mask" in E.last_error()
    assert run(kept=M - nout_bytes + 1) == E.BLDP_EINVAL and "the mask" in E.last_error()
    assert run(out=M + 63, ld=[1, 0, 0]) == E.BLDP_EINVAL and "the mask" in E.last_error()
    # negative or overlapping output strides
    for ld_i, ld_t in ((15, 32), (16, 31), (-16, 32), (16, -32)):
        assert run(ld_i=ld_i, ld_t=ld_t) == E.BLDP_EINVAL and "strides" in E.last_error()
    # factors that do not divide the window; a window outside the array
    assert run(nfpc=3) == E.BLDP_EDIM and "nfpc=3" in E.last_error()
    assert run(T=3) == E.BLDP_EDIM and "tavby=3" in E.last_error()
    assert run(win=[60, 8, 1, 0, 2, 1, 0, 4, 1]) == E.BLDP_EBOUNDS
    # the band and host calls make the same checks
    ptrs = (ctypes.c_void_p * 2)(A, A + (1 << 16))
    band = L.bldp_band_fold_f32
    assert band(2, ptrs, 64, 2, 4, None, 16, 2, 2, M, None, O, K, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 16, 2, 0, M, None, None, None, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 5, 2, 0, M, None, O, K, None) == E.BLDP_EDIM
    assert band(0, ptrs, 64, 2, 4, None, 16, 2, 0, M, None, O, K, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 0, 2, 0, M, None, O, K, None) == E.BLDP_EINVAL
    # (the dense band mask spans both banks: 2 * 64 * 2 * 4 bytes)
    assert band(2, ptrs, 64, 2, 4, None, 16, 2, 0, M, None, M + 1023, K, None) == E.BLDP_EINVAL
    assert "the mask" in E.last_error()
    host = L.bldp_fold_host_f32
    assert host(0, A, 64, 2, 4, None, 16, 2, 3, M, None, O, K) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 3, 2, 0, M, None, O, K) == E.BLDP_EDIM
    assert host(0, A, 64, 2, 4, None, 0, 2, 0, M, None, O, K) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 16, 2, 0, M, None, None, None) == E.BLDP_EINVAL
    assert host(0, None, 64, 2, 4, None, 16, 2, 0, M, None, O, K) == E.BLDP_EINVAL
    neg = (ctypes.c_int64 * 3)(1, -1, 0)
    assert host(0, A, 64, 2, 4, None, 16, 2, 0, M, neg, O, K) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers
    assert run(in_=None, dims=(64, 2, 0), mask=None, out=None, kept=None) == 0
    assert host(0, None, 64, 2, 0, None, 16, 2, 0, None, None, None, None) == 0


def test_unfold_refusals(pkg, L):
    E = pkg._lib
    A, P, O = 1 << 20, 2 << 20, 3 << 20  # never dereferenced

    def run(in_=A, dims=(64, 2, 4), nfpc=16, T=2, uop=0, prof=P, pld=(16, 32), out=O, old=(64, 128),
            win=None):
        keep, wp = E.win_arg(win)
        return L.bldp_unfold_f32(in_, *dims, wp, nfpc, T, uop, prof, pld[0], pld[1], out, old[0],
                                 old[1], None)

    assert run(nfpc=0) == E.BLDP_EINVAL and "nfpc" in E.last_error()
    for uop in (2, -1, 8):
        assert run(uop=uop) == E.BLDP_EINVAL and "divide" in E.last_error()
    assert run(in_=None) == E.BLDP_EINVAL and "null input" in E.last_error()
    assert run(prof=None) == E.BLDP_EINVAL and "null profile" in E.last_error()
    assert run(out=None) == E.BLDP_EINVAL and "null output" in E.last_error()
    for old in ((63, 128), (64, 127), (-64, 128), (64, -128)):
        assert run(old=old) == E.BLDP_EINVAL and "strides" in E.last_error()
    for pld in ((-16, 32), (16, -32)):
        assert run(pld=pld) == E.BLDP_EINVAL and "negative" in E.last_error()
    # in place, or over any part of the window; over the profile
    assert run(out=A) == E.BLDP_EINVAL and "not in place" in E.last_error()
    assert run(out=A + 4 * 64 * 2 * 4 - 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(out=P + 4 * 16 * 2 * 2 - 4) == E.BLDP_EINVAL and "profile" in E.last_error()
    assert run(out=P - 4 * 64 * 2 * 4 + 4) == E.BLDP_EINVAL and "profile" in E.last_error()
    assert run(nfpc=3) == E.BLDP_EDIM and run(T=3) == E.BLDP_EDIM
    assert run(win=[60, 8, 1, 0, 2, 1, 0, 4, 1]) == E.BLDP_EBOUNDS
    ptrs = (ctypes.c_void_p * 2)(A, A + (1 << 16))
    band = L.bldp_band_unfold_f32
    assert band(2, ptrs, 64, 2, 4, None, 16, 2, 2, P, 16, 32, O, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 16, 2, 0, None, 16, 32, O, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 16, 2, 0, P, 16, 32, A + (1 << 16), None) == E.BLDP_EINVAL
    assert band(9, ptrs, 64, 2, 4, None, 16, 2, 0, P, 16, 32, O, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 5, 2, 0, P, 16, 32, O, None) == E.BLDP_EDIM
    host = L.bldp_unfold_host_f32
    assert host(0, A, 64, 2, 4, None, 16, 2, 2, P, O) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 3, 2, 0, P, O) == E.BLDP_EDIM
    assert host(0, A, 64, 2, 4, None, 16, 2, 0, None, O) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 16, 2, 0, P, None) == E.BLDP_EINVAL
    assert host(0, None, 64, 2, 4, None, 16, 2, 0, P, O) == E.BLDP_EINVAL
    assert run(in_=None, dims=(64, 2, 0), prof=None, out=None) == 0
    assert host(0, None, 64, 2, 0, None, 16, 2, 0, None, None) == 0


# ---- Python: TypeError and ValueError before any GPU work -------------------------
def test_python_checks(pkg):
    import torch

    eng, W = pkg.engine, pkg.worker
    x = torch.zeros(8, 2, 4)
    m = torch.zeros(8, 2, 4, dtype=torch.uint8)
    p = torch.zeros(4, 2, 1)
    a = np.zeros((8, 2, 4), np.float32, order="F")
    for bad in (x.double(), x.to(torch.int16), a):
        with pytest.raises(TypeError):
            eng.fold(bad, 4)
        with pytest.raises(TypeError):
            eng.unfold(bad, p, 4)
    with pytest.raises(TypeError):
        eng.band_fold([x.double()], 4)
    with pytest.raises(TypeError):
        eng.band_unfold([x.double()], p, 4)
    for op in ("max", "median", "argmax", 0):
        with pytest.raises(ValueError, match="sum"):
            eng.fold(x, 4, op=op)
        with pytest.raises(ValueError, match="sum"):
            eng.fold_host(a, 4, op=op)
    for how in ("multiply", "div", 0, None):
        with pytest.raises(ValueError, match="divide"):
            eng.unfold(x, p, 4, how=how)
        with pytest.raises(ValueError, match="divide"):
            eng.unfold_host(a, p.numpy(), 4, how=how)
    for nfpc in (0, -2, None):
        with pytest.raises(ValueError, match="nfpc"):
            eng.fold(x, nfpc)
    with pytest.raises(pkg.DimensionMismatch):
        eng.fold(x, 3)
    with pytest.raises(pkg.DimensionMismatch):
        eng.fold(x, 4, tavby=3)
    for badm in (m.float(), m.to(torch.int8), m.numpy()):
        with pytest.raises(TypeError):
            eng.fold(x, 4, mask=badm)
    with pytest.raises(ValueError, match="mask"):
        eng.fold(x, 4, mask=torch.zeros(8, 2, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):  # a host mask of the right shape is still no device tensor
        eng.fold(x, 4, mask=m)
    with pytest.raises(TypeError):
        eng.unfold(x, p.double(), 4)
    with pytest.raises(ValueError, match="profile"):
        eng.unfold(x, torch.zeros(4, 2, 2), 4)
    with pytest.raises(TypeError):  # the profile of the right shape is still no device tensor
        eng.unfold(x, p, 4)
    with pytest.raises(TypeError):
        eng.fold_host(a.astype(np.float64), 4)
    with pytest.raises(TypeError):
        eng.fold_host(a, 4, mask=np.zeros((8, 2, 4), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.fold_host(a, 4, mask=np.zeros((8, 2, 5), np.uint8))
    with pytest.raises(TypeError):
        eng.unfold_host(a, p.numpy().astype(np.float64), 4)
    with pytest.raises(ValueError, match="profile"):
        eng.unfold_host(a, np.zeros((4, 2, 2), np.float32), 4)
    # the workers: before any file is touched
    with pytest.raises(ValueError):
        W.getbandpass("/no/such/file.fil", nfpc=4, func="max")
    with pytest.raises(TypeError):
        W.getbandpass("/no/such/file.fil", nfpc=4, mask=np.zeros((8, 2, 4), np.float32))
    with pytest.raises(ValueError, match="nfpc"):
        W.getbandpass(a)  # an array source must name nfpc
    with pytest.raises(ValueError, match="nfpc"):
        W.getflattened(a)
    with pytest.raises(ValueError, match="nfpc"):
        W.getbandpass(a, nfpc=0)
    with pytest.raises(TypeError):
        W.getbandpass(a.astype(np.int8), nfpc=4)
    with pytest.raises(ValueError):
        W.getflattened("/no/such/file.fil", nfpc=4, how="multiply")
    with pytest.raises(ValueError):
        W.getflattened("/no/such/file.fil", nfpc=4, nsigma=-1.0)
    with pytest.raises(ValueError):
        W.getflattened("/no/such/file.fil", nfpc=4, nsigma=5.0, axis=1)
    with pytest.raises(TypeError):
        W.getflattened(a.astype(np.uint8), nfpc=4)
    with pytest.raises(ValueError):
        pkg.GBT.getbandpass([0], ["/no/such/file.fil"], nfpc=4, func="median")


def test_gbt_combines_in_float64(pkg):
    """GBT.getbandpass adds the banks' sums and counts before the one division."""
    parts = [{"data": np.full((2, 1, 1), 2 ** 24, np.float32), "kept": np.full((2, 1, 1), 3, np.int32)},
             {"data": np.ones((2, 1, 1), np.float32), "kept": np.ones((2, 1, 1), np.int32)}]
    r = pkg.GBT._combine_bandpass(parts, "mean")
    assert r["data"].dtype == np.float32 and r["kept"].tolist() == [[[4]], [[4]]]
    assert r["data"][0, 0, 0] == np.float32((2.0 ** 24 + 1) / 4)
    assert pkg.GBT._combine_bandpass(parts, "sum")["data"][0, 0, 0] == np.float32(2.0 ** 24 + 1)
    for p in parts:  # nothing kept anywhere: 0 / 0
        p["kept"][:] = 0
        p["data"][:] = 0
    assert np.isnan(pkg.GBT._combine_bandpass(parts, "mean")["data"]).all()


# ---- the symbols and the documents -----------------------------------------------
def test_symbols_everywhere(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    shim = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in NAMES:
        assert name in pkg._lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"BLDP_API int %s\(" % name, hdr)
    for name in ("bldp_fold_shape", "bldp_fold_plan_f32", "bldp_fold_f32", "bldp_band_fold_f32",
                 "bldp_fold_host_f32", "bldp_unfold_f32", "bldp_band_unfold_f32",
                 "bldp_unfold_host_f32"):
        assert ":%s" % name in shim
    for fn in ("gpu_fold", "gpu_fold_plan", "gpu_band_fold", "gpu_unfold", "gpu_band_unfold"):
        assert re.search(r"^function %s\(" % fn, shim, re.M) and fn in shim[:shim.index("const libbldp")]
    assert int(re.search(r"#define BLDP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert "bldp_*fold_* and bldp_*unfold_*" in hdr[:hdr.index("#define BLDP_ABI_VERSION")]
    assert "BLDP_UNFOLD_DIV = 0, BLDP_UNFOLD_SUB = 1" in hdr
    assert pkg._lib.FOLD_PATHS == {0: "cols", 1: "rows"}
    assert pkg._lib.FOLD_MASK_LOADS == {0: "byte", 1: "dword", 2: "row", 3: "none"}
    assert pkg._lib.UNFOLD_OPS == {"divide": 0, "subtract": 1}
    for fn in ("fold", "fold_plan", "band_fold", "fold_host", "unfold", "unfold_plan", "band_unfold",
               "unfold_host"):
        assert callable(getattr(pkg.engine, fn))
    assert callable(pkg.getbandpass) and callable(pkg.getflattened)
    assert callable(pkg.GBT.getbandpass) and callable(pkg.GBT.getflattened)
    assert "fold.hip" in open(os.path.join(CSRC, "Makefile")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "fold.hip" in design
    for item in ("median over coarse channels", "typed input", "prepared handles",
                 "multi-device band entry", "in-place unfold", "unit mean"):
        assert item in design, item
