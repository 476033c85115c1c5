"""The histogram without a GPU: the NumPy restatement of the rule against
numpy.histogram and against the clamp cases of include/bldp.h, the plan of every
path and load width (the table the GPU tests iterate over), every refusal of the
ABI with pointers that are never dereferenced, the Python argument checks, and
the symbols."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from histogram_ref import PLAN_CASES, hist_edges_ref, hist_k, hist_planes, histogram_ref

NAMES = ("bldp_histogram_plan_f32", "bldp_histogram_f32", "bldp_band_histogram_f32",
         "bldp_histogram_host_f32")
KEYS = ("path", "workgroups", "chunks_per_block", "blocks_per_workgroup", "lds_bytes", "replicas",
        "workspace_bytes", "vector_loads", "channel_lanes", "rows_per_chunk")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---- the restatement against an independent check ------------------------------------
@pytest.mark.parametrize("B,width,lo", [(16, 4, -32), (256, 1, 0), (5, 8, -8), (4096, 0.5, -1024)])
def test_restatement_against_numpy_histogram(B, width, lo):
    """Integer-valued data and power-of-two bin widths: every Float32 operation of
    the rule is exact, so the counts are numpy.histogram's of the Float64 data,
    with the samples equal to hi moved out of NumPy's closed last bin."""
    hi = lo + B * width
    rng = np.random.default_rng(B)
    a = rng.integers(int(lo) - 3 * int(np.ceil(width)) - 2, int(hi) + 3 * int(np.ceil(width)) + 3,
                     (16, 2, 24)).astype(np.float32)
    a[3, 1, 5] = hi      # at least one sample on the closed edge
    a[4, 0, 6] = lo
    for F, T in ((16, 24), (4, 8), (1, 1)):
        got = histogram_ref(a, B, lo, hi, F, T)
        assert got.shape == (16 // F, 2, 24 // T, B + 3) and (got.sum(axis=-1) == F * T).all()
        for co in range(16 // F):
            for i in range(2):
                for to in range(24 // T):
                    blk = a[co * F:(co + 1) * F, i, to * T:(to + 1) * T].astype(np.float64).ravel()
                    want = np.histogram(blk, bins=B, range=(float(lo), float(hi)))[0].copy()
                    want[-1] -= int((blk == hi).sum())
                    assert np.array_equal(got[co, i, to, :B], want)
                    assert got[co, i, to, B] == (blk < lo).sum()
                    assert got[co, i, to, B + 1] == (blk >= hi).sum()
                    assert got[co, i, to, B + 2] == 0


# ---- the clamp ---------------------------------------------------------------------
def test_clamp_cases():
    """The largest Float32 below hi gives k == B where include/bldp.h says so."""
    for lo, hi, B, k in ((-1, 1, 7, 7), (-5, 5, 100, 100), (-3, 3, 6, 6), (0, 3, 3, 2),
                         (0, 10, 10, 9)):
        x = np.nextafter(np.float32(hi), np.float32(-np.inf))
        assert x < np.float32(hi) and hist_k([x], B, lo, hi)[0] == k
        assert hist_planes([x], B, lo, hi)[0] == B - 1
    rng = np.random.default_rng(1)
    for _ in range(300):  # k never exceeds B
        lo = np.float32(rng.normal(0, 100))
        hi = np.float32(lo + abs(rng.normal(0, 50)) + 1e-3)
        B = int(rng.integers(1, 4097))
        x = np.nextafter(hi, np.float32(-np.inf))
        assert hist_k([x], B, lo, hi)[0] <= B


def test_restatement_special_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([nan, -nan, -inf, inf, -0.0, 0.0, 1e-45, -1e-45, 1.0, np.nextafter(np.float32(1), 0)],
                 dtype=np.float32)
    assert list(hist_planes(x, 4, 0, 1)) == [6, 6, 4, 5, 0, 0, 0, 4, 5, 3]
    e = hist_edges_ref(4, 0, 1)
    assert e.dtype == np.float64 and list(e) == [0.0, 0.25, 0.5, 0.75, 1.0]


# ---- the plan call: null pointers, no GPU ------------------------------------------------
def plan(pkg, L, dims, F, T, B, win=None, ptr=None, lo=-1.0, hi=1.0):
    info = (ctypes.c_int64 * 10)(*([-1] * 10))
    keep, wp = pkg._lib.win_arg(win)
    rc = L.bldp_histogram_plan_f32(ptr, *dims, wp, F, T, B, lo, hi, info)
    assert rc == 0, pkg._lib.last_error()
    d = dict(zip(KEYS, [int(v) for v in info]))
    assert d["workspace_bytes"] == 0
    d["path"] = pkg._lib.HIST_PATHS[d["path"]]
    return d


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_plan_forms(pkg, L, name):
    dims, F, T, B, win, (path, vec, chunks, bpw) = PLAN_CASES[name]
    p = plan(pkg, L, dims, F, T, B, win)
    assert (p["path"], p["vector_loads"], p["chunks_per_block"], p["blocks_per_workgroup"]) == \
        (path, vec, chunks, bpw)
    nc, ni, nt = (dims if win is None else (win[1], win[4], win[7]))
    groups = -(-(nc // F) // bpw)
    assert p["workgroups"] == groups * ni * (nt // T) * chunks
    assert (path in ("block_split", "lanes_tsplit")) == (chunks > 1)
    assert (path in ("lanes", "lanes_tsplit")) == (bpw > 1)
    # LDS: (B + 3) counters for every block of the workgroup and every replica; 48 KiB at most
    assert p["lds_bytes"] == 4 * (B + 3) * bpw * p["replicas"] <= 49152
    assert p["replicas"] & (p["replicas"] - 1) == 0 and 1 <= p["replicas"] <= 32
    assert 256 % p["channel_lanes"] == 0 and p["rows_per_chunk"] % (256 // p["channel_lanes"]) == 0
    # the lo / hi of the call do not move the plan; a pointer off the dword grid takes dwords
    assert plan(pkg, L, dims, F, T, B, win, lo=3.0, hi=1e6) == p
    assert plan(pkg, L, dims, F, T, B, win, ptr=(1 << 20) + 4) == p
    q = plan(pkg, L, dims, F, T, B, win, ptr=(1 << 20) + 2)
    assert q["vector_loads"] == 0 and q["path"] in (path, "block" if chunks == 1 else "block_split")


def test_plan_names_every_path_and_width():
    seen = {(c[5][0], c[5][1]) for c in PLAN_CASES.values()}
    assert seen == {(p, v) for p in ("block", "block_split", "lanes", "lanes_tsplit") for v in (0, 1)}


def test_plan_split_block_inside_the_test_cap(pkg, L):
    """A single block shared by workgroups, its rows no multiple of the chunk."""
    dims, F, T, B, win, _ = PLAN_CASES["block_split_vec"]
    assert dims[0] * dims[1] * dims[2] <= 2 ** 22 and dims[0] == F and dims[2] == T
    p = plan(pkg, L, dims, F, T, B)
    assert p["workgroups"] == p["chunks_per_block"] >= 2 and T % p["rows_per_chunk"] != 0
    assert (p["chunks_per_block"] - 1) * p["rows_per_chunk"] < T <= \
        p["chunks_per_block"] * p["rows_per_chunk"]


def test_plan_fills_the_gpu_with_one_block(pkg, L):
    """The shapes of the issue: no big block runs on a handful of workgroups."""
    for dims, F, T in (((65536, 1, 272), 65536, 272), ((512, 1, 879616), 512, 879616),
                       ((1 << 26, 1, 16), 1 << 26, 16), ((512, 1, 879616), 1, 879616)):
        for B in (64, 256, 4096):
            p = plan(pkg, L, dims, F, T, B)
            assert p["workgroups"] >= 512 and p["chunks_per_block"] > 1, (dims, F, B, p)
    p = plan(pkg, L, (65536, 1, 272), 64, 16, 64)
    assert p["path"] == "lanes" and p["blocks_per_workgroup"] == 16 and p["vector_loads"] == 1
    # an empty window plans without a fault
    assert plan(pkg, L, (256, 1, 4), 8, 1, 64, win=[0, 0, 1, 0, 1, 1, 0, 4, 1])["workgroups"] == 0


# ---- the refusals, before any launch -------------------------------------------------
def test_refusals(pkg, L):
    E = pkg._lib
    A, O = 1 << 20, 3 << 20  # never dereferenced
    info = (ctypes.c_int64 * 10)()

    def run(in_=A, dims=(64, 2, 4), F=4, T=2, B=16, lo=-1.0, hi=1.0, out=O, ld_i=16, ld_t=32,
            ld_q=64, win=None):
        keep, wp = E.win_arg(win)
        return L.bldp_histogram_f32(in_, *dims, wp, F, T, B, lo, hi, out, ld_i, ld_t, ld_q, None)

    def refused(**kw):
        a = dict(dims=(64, 2, 4), F=4, T=2, B=16, lo=-1.0, hi=1.0)
        a.update(kw)
        rcs = {run(**kw), L.bldp_histogram_plan_f32(None, *a["dims"], None, a["F"], a["T"], a["B"],
                                                    a["lo"], a["hi"], info),
               L.bldp_histogram_host_f32(0, A, *a["dims"], None, a["F"], a["T"], a["B"], a["lo"],
                                         a["hi"], O)}
        return rcs == {E.BLDP_EINVAL}

    # 1 <= B <= 4096
    for B in (0, -1, 4097, 1 << 20):
        assert refused(B=B) and "nbins" in E.last_error()
    # lo and hi finite as Float32, lo < hi as Float32
    inf, nan = float("inf"), float("nan")
    for lo, hi in ((nan, 1.0), (0.0, nan), (-inf, 1.0), (0.0, inf), (1.0, 1.0), (2.0, 1.0),
                   (0.0, 1e39), (-1e39, 0.0), (1.0, 1.0 + 1e-9)):
        assert refused(lo=lo, hi=hi) and "finite" in E.last_error(), (lo, hi)
    # hi - lo overflows Float32
    assert refused(lo=-3e38, hi=3e38) and "overflows" in E.last_error()
    # the scale B / w is not finite (a subnormal width) or is 0 (a huge width, one bin)
    assert refused(lo=0.0, hi=1e-44, B=4096) and "scale" in E.last_error()
    # (s = 2.9e-39, a subnormal above 0, is legal: the plan call launches nothing)
    assert L.bldp_histogram_plan_f32(None, 64, 2, 4, None, 4, 2, 1, -1.7e38, 1.7e38, info) == 0
    # F * T = 2^31 is beyond Int32; 2^31 - 2^16 is not
    assert L.bldp_histogram_plan_f32(None, 65536, 1, 32768, None, 65536, 32768, 16, 0.0, 1.0,
                                     info) == E.BLDP_EINVAL and "2^31" in E.last_error()
    assert L.bldp_histogram_plan_f32(None, 65536, 1, 32767, None, 65536, 32767, 16, 0.0, 1.0,
                                     info) == 0
    assert L.bldp_histogram_plan_f32(None, 64, 1, 4, None, 4, 1, 16, 0.0, 1.0, None) == E.BLDP_EINVAL
    # null pointers
    assert run(in_=None) == E.BLDP_EINVAL and "null input" in E.last_error()
    assert run(out=None) == E.BLDP_EINVAL and "null output" in E.last_error()
    # the output over the input window; output strides that overlap
    assert run(out=A + 4 * (64 * 2 * 4) - 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(out=A - 4 * (18 * 64 + 64) + 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(ld_i=15) == E.BLDP_EINVAL and "strides" in E.last_error()
    assert run(ld_t=31) == E.BLDP_EINVAL and "strides" in E.last_error()
    assert run(ld_q=63) == E.BLDP_EINVAL and "strides" in E.last_error()
    # factors that do not divide the window; a window outside the array
    assert run(F=3) == E.BLDP_EDIM and "fqavby=3" in E.last_error()
    assert run(T=3) == E.BLDP_EDIM and "tavby=3" in E.last_error()
    assert run(win=[60, 8, 1, 0, 2, 1, 0, 4, 1]) == E.BLDP_EBOUNDS
    # the band and host calls make the same checks
    ptrs = (ctypes.c_void_p * 2)(A, A + (1 << 16))
    band = L.bldp_band_histogram_f32
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 0, -1.0, 1.0, O, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 16, 1.0, 1.0, O, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 16, -1.0, 1.0, None, None) == E.BLDP_EINVAL
    assert "null output" in E.last_error()
    assert band(2, ptrs, 64, 2, 4, None, 5, 2, 16, -1.0, 1.0, O, None) == E.BLDP_EDIM
    assert band(0, ptrs, 64, 2, 4, None, 4, 2, 16, -1.0, 1.0, O, None) == E.BLDP_EINVAL
    assert band(2, None, 64, 2, 4, None, 4, 2, 16, -1.0, 1.0, O, None) == E.BLDP_EINVAL
    host = L.bldp_histogram_host_f32
    assert host(0, A, 64, 2, 4, None, 3, 2, 16, -1.0, 1.0, O) == E.BLDP_EDIM
    assert host(0, None, 64, 2, 4, None, 4, 2, 16, -1.0, 1.0, O) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 4, 2, 16, -1.0, 1.0, None) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers
    assert run(in_=None, dims=(64, 2, 0), out=None) == 0
    assert host(0, None, 64, 2, 0, None, 4, 2, 16, -1.0, 1.0, None) == 0


# ---- Python: TypeError and ValueError before any GPU work -------------------------
def test_python_checks(pkg):
    import torch

    eng, W = pkg.engine, pkg.worker
    x = torch.zeros(8, 2, 4)
    a = np.zeros((8, 2, 4), np.float32, order="F")
    for bad in (x.double(), x.to(torch.int16), x.to(torch.uint8)):
        with pytest.raises(TypeError, match="Float32"):
            eng.histogram(bad, 16, 0, 1)
        with pytest.raises(TypeError, match="Float32"):
            eng.band_histogram([bad], 16, 0, 1)
    for dt in (np.float64, np.int8, np.uint16):
        with pytest.raises(TypeError, match="Float32"):
            eng.histogram_host(a.astype(dt), 16, 0, 1)
        with pytest.raises(TypeError, match="Float32"):
            W.gethistogram(a.astype(dt), nbins=16, lo=0, hi=1)
    with pytest.raises(TypeError):
        eng.histogram_host(np.ascontiguousarray(a), 16, 0, 1)  # not Fortran-ordered
    # the parameter conditions, as the library words them (ValueError)
    bad_params = [(0, 0, 1), (4097, 0, 1), (16, 1, 1), (16, 2, 1), (16, float("nan"), 1),
                  (16, 0, float("inf")), (16, -3e38, 3e38), (4096, 0, 1e-44), (16, 1, 1 + 1e-9)]
    for B, lo, hi in bad_params:
        for call in (lambda: eng.histogram(x, B, lo, hi), lambda: eng.histogram_host(a, B, lo, hi),
                     lambda: eng.band_histogram([x], B, lo, hi), lambda: eng.hist_edges(B, lo, hi),
                     lambda: W.gethistogram("/no/such/file.fil", nbins=B, lo=lo, hi=hi),
                     lambda: pkg.GBT.gethistogram([0], ["/no/such/file.fil"], nbins=B, lo=lo, hi=hi)):
            with pytest.raises(ValueError, match="histogram"):
                call()
    with pytest.raises(TypeError):
        eng.histogram(x, 2.5, 0, 1)
    with pytest.raises(TypeError):
        eng.histogram(x, "many", 0, 1)
    # factors that do not divide the window (DimensionMismatch) before any GPU work
    with pytest.raises(pkg.DimensionMismatch):
        eng.histogram_host(a, 16, 0, 1, fqavby=3)
    with pytest.raises(pkg.DimensionMismatch):
        eng.histogram_host(a, 16, 0, 1, tavby=3)
    # a caller's out: dtype, shape, device, layout and planes that overlap
    dims, K = (4, 2, 2), 19
    good = torch.empty((K, 2, 2, 4), dtype=torch.int32).permute(3, 2, 1, 0)
    assert eng._hist_out(good, dims, K, "cpu")[1:] == (4, 8, 16)
    with pytest.raises(TypeError):
        eng._hist_out(good.numpy(), dims, K, "cpu")
    for dt in (torch.float32, torch.int64, torch.uint8):
        with pytest.raises(TypeError, match="int32"):
            eng._hist_out(good.to(dt), dims, K, "cpu")
    with pytest.raises(ValueError, match="expected"):
        eng._hist_out(good[..., :18], dims, K, "cpu")
    with pytest.raises(ValueError, match="expected"):
        eng._hist_out(good[..., 0], dims, K, "cpu")
    with pytest.raises(ValueError, match="is on"):
        eng._hist_out(good, dims, K, "cuda:0")
    with pytest.raises(ValueError, match="layout"):
        eng._hist_out(torch.empty((4, 2, 2, K), dtype=torch.int32), dims, K, "cpu")
    with pytest.raises(ValueError, match="overlap"):
        eng._hist_out(torch.as_strided(torch.empty(400, dtype=torch.int32), (4, 2, 2, K),
                                       (1, 4, 8, 15)), dims, K, "cpu")
    with pytest.raises(ValueError, match="overlap"):
        eng._hist_out(good.expand(4, 2, 2, K)[..., :1].expand(4, 2, 2, K), dims, K, "cpu")
    # the edges: Float64, a reading aid
    e = eng.hist_edges(100, -5, 5)
    assert e.dtype == np.float64 and e.shape == (101,) and np.array_equal(e, hist_edges_ref(100, -5, 5))


# ---- the symbols and the documents -----------------------------------------------
def test_symbols_everywhere(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    shim = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in NAMES:
        assert name in pkg._lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"BLDP_API int %s\(" % name, hdr)
    for name in ("bldp_histogram_f32", "bldp_band_histogram_f32", "bldp_histogram_host_f32"):
        assert ":%s" % name in shim
    assert "gpu_histogram" in shim and "gpu_band_histogram" in shim
    assert int(re.search(r"#define BLDP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert "bldp_*histogram_* entry points" in hdr
    assert int(re.search(r"#define BLDP_MAX_HIST_BINS (\d+)", hdr).group(1)) == pkg._lib.MAX_HIST_BINS
    assert pkg._lib.HIST_PATHS == {0: "block", 1: "block_split", 2: "lanes", 3: "lanes_tsplit"}
    for fn in ("histogram", "histogram_plan", "band_histogram", "histogram_host"):
        assert callable(getattr(pkg.engine, fn))
    assert callable(pkg.gethistogram) and callable(pkg.worker.gethistogram)
    assert callable(pkg.GBT.gethistogram)
    assert "hist.hip" in open(os.path.join(REPO, "DESIGN.md")).read()
    assert "hist.hip" in open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "csrc",
                                           "Makefile")).read()
