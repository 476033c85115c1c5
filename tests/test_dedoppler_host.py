"""CPU: the dedoppler without a GPU: the NumPy restatement on windows written out
by hand, the plan entry point with null pointers, every refusal of the rule
(include/bldp.h) with pointers that are never dereferenced, which kernels the GPU
cases of tests/dedoppler_cases.py run (from the plan alone), the pure helpers, the
Python argument checks, and the symbols."""
from __future__ import annotations

import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO
import dedoppler_cases as dc
from dedoppler_ref import bits, dedoppler_ref, off, offsets, scan_order

NAMES = ("bldp_dedoppler_plan_f32", "bldp_dedoppler_f32", "bldp_band_dedoppler_f32",
         "bldp_dedoppler_host_f32")
CSRC = os.path.join(REPO, "bldistributeddataproducts.jl_amd", "csrc")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---- the restatement, by hand ----------------------------------------------------------
def test_path_by_hand():
    assert [off(5, t, 16) for t in range(16)] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5]
    assert [off(1, t, 2) for t in range(2)] == [0, 1]
    assert [off(3, t, 3) for t in range(3)] == [0, 2, 3]      # 1.5 rounds away from zero
    assert [off(-3, t, 3) for t in range(3)] == [0, -2, -3]
    for T in (2, 3, 16, 17):
        for d in range(-40, 41):
            path = [off(d, t, T) for t in range(T)]
            assert path[0] == 0 and path[-1] == d
            assert path == [-off(-d, t, T) for t in range(T)]
            # the nearest channel to the straight line, halves away from zero
            for t in range(T):
                assert abs(path[t]) == math.floor(Fraction(abs(d) * t, T - 1) + Fraction(1, 2))
        tab = offsets(40, T)
        assert tab.shape == (81, T) and len({tuple(r) for r in tab}) == 81  # no shared path
    assert scan_order(3) == [0, -1, 1, -2, 2, -3, 3]


def test_restatement_by_hand():
    # 4 channels, T = 2, D = 1: off(+-1, 1) = +-1
    w = np.array([[1, 10], [2, 20], [3, 30], [4, 40]], np.float32).reshape(4, 1, 2)
    s, best, drift = dedoppler_ref(w, 1, 2)
    assert s[:, 0, 0, 1].tolist() == [11, 22, 33, 44]          # d = 0
    assert s[:, 0, 0, 0].tolist() == [1, 12, 23, 34]           # d = -1: c - 1 at t = 1
    assert s[:, 0, 0, 2].tolist() == [21, 32, 43, 4]           # d = +1: c + 1 at t = 1
    assert best[:, 0, 0].tolist() == [21, 32, 43, 44] and drift[:, 0, 0].tolist() == [1, 1, 1, 0]
    # segments of 2: channels 1 and 2 no longer see each other
    s, best, drift = dedoppler_ref(w, 1, 2, seg=2)
    assert s[:, 0, 0, 0].tolist() == [1, 12, 3, 34] and s[:, 0, 0, 2].tolist() == [21, 2, 43, 4]
    # a segment that does not divide nc: {0, 1, 2}, {3}
    s, _, _ = dedoppler_ref(w, 1, 2, seg=3)
    assert s[:, 0, 0, 0].tolist() == [1, 12, 23, 4] and s[:, 0, 0, 2].tolist() == [21, 32, 3, 4]
    # a flat window: every tie goes to the first in scan order, drift 0
    _, best, drift = dedoppler_ref(np.full((40, 2, 8), 2.5, np.float32), 6, 4)
    assert (drift == 0).all() and (best == 10.0).all()
    # Float32 adds in time order: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 does not
    a = np.array([2.0 ** 24, 1, 1], np.float32).reshape(1, 1, 3)
    assert dedoppler_ref(a, 0, 3)[1][0, 0, 0] == np.float32(2.0 ** 24)
    assert dedoppler_ref(a[:, :, ::-1], 0, 3)[1][0, 0, 0] == np.float32(2.0 ** 24 + 2)
    # an all -0.0 window gives +0.0; a NaN is in exactly the sums whose path passes it
    z = dedoppler_ref(np.full((6, 1, 4), -0.0, np.float32), 2, 4)[1]
    assert (bits(z) == 0).all()
    n = np.ones((9, 1, 4), np.float32)
    n[4, 0, 2] = np.nan
    s, best, drift = dedoppler_ref(n, 2, 4)
    tab = offsets(2, 4)
    for c in range(9):
        for k in range(5):
            assert np.isnan(s[c, 0, 0, k]) == (c + tab[k, 2] == 4)
    # off(+-1, 2) = +-1, off(+-2, 2) = +-1, off(0, 2) = 0: scan order picks 0, then -1, then +1
    assert drift[:, 0, 0].tolist() == [0, 0, 0, 1, 0, -1, 0, 0, 0]
    assert np.isnan(best[3:6, 0, 0]).all() and not np.isnan(best[[0, 1, 2, 6, 7, 8], 0, 0]).any()


@pytest.mark.parametrize("d", [0, 7, -32, 32])
def test_planted_line_is_found(d):
    T, D, nc, c0 = 32, 32, 160, 80
    w = np.random.default_rng(d + 40).integers(0, 4, (nc, 1, T)).astype(np.float32)
    for t in range(T):
        w[c0 + off(d, t, T), 0, t] = 100.0
    _, best, drift = dedoppler_ref(w, D, T)
    c = int(np.argmax(best[:, 0, 0]))
    assert (c, int(drift[c, 0, 0])) == (c0, d) and best[c, 0, 0] == 3200.0


# ---- the pure helpers --------------------------------------------------------------------
def test_drift_offsets_and_rates(pkg):
    eng = pkg.engine
    for D, T in ((0, 2), (1, 2), (5, 16), (40, 17), (1024, 3)):
        tab = eng.drift_offsets(D, T)
        assert tab.dtype == np.int64 and np.array_equal(tab, offsets(D, T))
    r = eng.drift_rates(2, 16, -2.7939677238464355e-06, 18.253611)
    hz = -2.7939677238464355
    want = [d * hz / (15 * 18.253611) for d in (-2, -1, 0, 1, 2)]
    assert r.dtype == np.float64 and np.allclose(r, want, rtol=1e-15, atol=0)
    assert r[0] > 0 > r[4]   # a negative foff turns the sign
    assert eng.drift_rates(1, 2, 1.0, 1.0).tolist() == [-1e6, 0.0, 1e6]
    for bad in ((-1, 4), (2, 1)):
        with pytest.raises(pkg.ArgumentError):
            eng.drift_offsets(*bad)
        with pytest.raises(pkg.ArgumentError):
            eng.drift_rates(*bad, 1.0, 1.0)


# ---- plans with null pointers ------------------------------------------------------------
def test_plan_product_shapes(pkg, L):
    bank = (1 << 26, 1, 16)
    # one 0000 bank: resident at every D; the tile grows with the halo
    p = dc.plan(pkg, L, bank, 16, 8)
    assert p == dict(path="resident", tile=256, halo=8, rows=16, G=8, groups=2,
                     lds=16 * 272 * 4, wgs=1 << 18, vec=1, ws=0)
    p = dc.plan(pkg, L, bank, 16, 64, seg=1 << 20)
    assert (p["path"], p["tile"], p["halo"], p["groups"], p["lds"]) == \
        ("resident", 256, 64, 16, 16 * 384 * 4)
    p = dc.plan(pkg, L, bank, 16, 512, seg=1 << 20)
    assert (p["path"], p["tile"], p["halo"], p["groups"], p["lds"], p["wgs"]) == \
        ("resident", 1024, 512, 128, 16 * 2048 * 4, 1 << 16)
    # one 0002 bank: 16 spectra a block, and the whole file a block (chunked)
    p = dc.plan(pkg, L, (65536, 1, 272), 16, 16)
    assert (p["path"], p["rows"], p["wgs"], p["vec"]) == ("resident", 16, 256 * 17, 1)
    p = dc.plan(pkg, L, (65536, 1, 272), 272, 16)
    assert (p["path"], p["rows"], p["wgs"]) == ("chunked", 65536 // (288 * 4), 256)
    assert p["lds"] == p["rows"] * 288 * 4 <= dc.LDS_CHUNK
    # the largest row there is: D = 1024 at the longest block
    p = dc.plan(pkg, L, (4096, 1, 1 << 20), 1 << 20, 1024)
    assert (p["path"], p["tile"], p["rows"], p["groups"]) == ("chunked", 1024, 5, 256)
    # 2^44 elements
    p = dc.plan(pkg, L, (1 << 26, 1, 1 << 18), 16, 64)
    assert (p["path"], p["wgs"], p["ws"]) == ("resident", (1 << 18) * (1 << 14), 0)
    # scalar staging: a window off the float4 boundary, a step, an odd pitch, an odd address
    assert dc.plan(pkg, L, (260, 2, 16), 16, 3, win=[1, 256, 1, 0, 2, 1, 0, 16, 1])["vec"] == 0
    assert dc.plan(pkg, L, (260, 2, 16), 16, 3, win=[4, 256, 1, 0, 2, 1, 0, 16, 1])["vec"] == 1
    assert dc.plan(pkg, L, (512, 2, 16), 16, 3, win=[0, 256, 2, 0, 2, 1, 0, 16, 1])["vec"] == 0
    assert dc.plan(pkg, L, (258, 2, 16), 16, 3)["vec"] == 0
    assert dc.plan(pkg, L, (256, 2, 16), 16, 3, ptr=(1 << 20) + 4)["vec"] == 0
    p = dc.plan(pkg, L, (258, 2, 16), 16, 3)
    assert p["halo"] == 3 and dc.plan(pkg, L, (256, 2, 16), 16, 3)["halo"] == 4
    # an empty window plans without a fault and reports nothing
    p = dc.plan(pkg, L, (256, 1, 4), 2, 3, win=[0, 0, 1, 0, 1, 1, 0, 4, 1])
    assert p["wgs"] == 0 and p["lds"] == 0


# ---- which kernels the GPU cases run, from the plan alone ------------------------------
def compiled_instantiations():
    src = open(os.path.join(CSRC, "dedoppler.hip")).read()
    out = {"k_dedoppler<%s>" % v for v in re.findall(r"launch_kernel\(k_dedoppler<(true|false)>", src)}
    assert len(re.findall(r"__global__", src)) == 1   # (nothing else is a kernel of the file)
    return out


def test_cases_reach_every_kernel_and_form(pkg, L):
    named, ids, seen = set(), set(), set()
    for c in dc.CASES:
        assert dc.case_id(c) not in ids
        ids.add(dc.case_id(c))
        assert np.prod(dc.array_shape(c)) * (2 * c.D + 1) * 4 <= 64 << 20, dc.case_id(c)
        p = dc.case_plan(pkg, L, c)
        assert (p["path"], p["vec"], p["tile"]) == c.plan, (dc.case_id(c), p)
        assert p["G"] == dc.GROUP and p["ws"] == 0 and p["halo"] >= c.D
        assert p["groups"] == max(1, -(-2 * c.D // dc.GROUP))
        assert p["rows"] == c.T if p["path"] == "resident" else p["rows"] < c.T
        assert p["lds"] <= (dc.LDS_RESIDENT if p["path"] == "resident" else dc.LDS_CHUNK)
        named.add("k_dedoppler<%s>" % str(bool(p["vec"])).lower())
        seen.add((p["path"], p["vec"], p["lds"] > dc.LDS_CHUNK))
    assert named == compiled_instantiations() == {"k_dedoppler<true>", "k_dedoppler<false>"}
    assert seen >= {("resident", 1, False), ("resident", 0, False), ("resident", 1, True),
                    ("chunked", 1, False), ("chunked", 0, False)}
    # the shapes the issue names are all there
    T = dc.TILE
    assert {c.nc for c in dc.CASES} >= {T - 1, T, T + 1, 2 * T + 3, 5, 1, 96}
    assert {c.D for c in dc.CASES} >= {0, 1, dc.GROUP - 1, dc.GROUP, dc.GROUP + 1, 64, 70, 1024}
    assert {c.T for c in dc.CASES} >= {2, 3, 16, 17, 272}
    assert {c.win for c in dc.CASES} == {"full", "c0", "cs2", "rev", "tsub"}
    assert any(c.seg == 16 and c.D == 20 for c in dc.CASES)
    assert any(c.seg and dc.TILE % c.seg and c.nc % c.seg == 0 for c in dc.CASES)
    assert any(c.seg and c.nc % c.seg for c in dc.CASES)
    assert any(c.ni == 2 and c.nt // c.T == 3 for c in dc.CASES)
    assert all(c.nc <= 512 and c.T == 4 for c in dc.CASES if c.D in (64, 1024))
    # one above what the small and the large LDS hold
    row = dc.case_plan(pkg, L, dc.CASES[0])["lds"] // 16 // 4  # (words of a row at D = 3: unused)
    assert row == dc.TILE + 2 * 3
    for c in dc.CASES:
        if (c.nc, c.D) == (96, 8):
            rb = (dc.TILE + 2 * 8) * 4
            assert c.T in (dc.LDS_CHUNK // rb + 1, dc.LDS_RESIDENT // rb + 1, 272)


# ---- the refusals, before any launch ---------------------------------------------------
def test_refusals(pkg, L):
    E = pkg._lib
    A, B, Dp, S = 1 << 20, 2 << 20, 3 << 20, 4 << 20  # never dereferenced
    info = (ctypes.c_int64 * 10)()

    def run(in_=A, dims=(64, 2, 8), T=4, D=3, seg=16, best=B, drift=Dp, sums=S, ld_i=64, ld_t=128,
            ld_q=256, win=None):
        keep, wp = E.win_arg(win)
        return L.bldp_dedoppler_f32(in_, *dims, wp, T, D, seg, best, drift, sums, ld_i, ld_t, ld_q,
                                    None)

    for T in (1, 0, -4):
        assert run(T=T) == E.BLDP_EINVAL and "tavby" in E.last_error()
    assert L.bldp_dedoppler_plan_f32(None, 64, 1, 1 << 22, None, (1 << 20) + 1, 3, 0,
                                     info) == E.BLDP_EINVAL and "2^20" in E.last_error()
    assert L.bldp_dedoppler_plan_f32(None, 64, 1, 1 << 22, None, 1 << 20, 3, 0, info) == 0
    for D in (-1, 1025, 1 << 40):
        assert run(D=D) == E.BLDP_EINVAL and "maxdrift" in E.last_error()
    assert L.bldp_dedoppler_plan_f32(None, 64, 2, 8, None, 4, 1024, 0, info) == 0
    assert run(seg=-1) == E.BLDP_EINVAL and "seg" in E.last_error()
    assert L.bldp_dedoppler_plan_f32(None, 64, 2, 8, None, 4, 3, 0, None) == E.BLDP_EINVAL
    # T that does not divide nt; a window outside the array
    assert run(T=3) == E.BLDP_EDIM and "tavby=3" in E.last_error()
    assert run(win=[60, 8, 1, 0, 2, 1, 0, 8, 1]) == E.BLDP_EBOUNDS
    assert run(win=[0, 64, 1, 0, 2, 1, 4, 8, 1]) == E.BLDP_EBOUNDS
    # null pointers: the input; best without drift; nothing asked for
    assert run(in_=None) == E.BLDP_EINVAL and "null input" in E.last_error()
    assert run(drift=None) == E.BLDP_EINVAL and "go together" in E.last_error()
    assert run(best=None) == E.BLDP_EINVAL and "go together" in E.last_error()
    assert run(best=None, drift=None, sums=None) == E.BLDP_EINVAL and "all null" in E.last_error()
    # outputs over the input window and over each other
    wbytes, plane = 4 * 64 * 2 * 8, 4 * 64 * 2 * 2
    assert run(best=A + wbytes - 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(drift=A - plane + 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(sums=A - 7 * plane + 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(drift=B + plane - 4) == E.BLDP_EINVAL and "best and drift" in E.last_error()
    assert run(sums=Dp + plane - 4) == E.BLDP_EINVAL and "drift and sums" in E.last_error()
    assert run(best=S + 7 * plane - 4) == E.BLDP_EINVAL and "best and sums" in E.last_error()
    # overlapping strides
    for ld_i, ld_t in ((63, 128), (64, 127), (-64, 128), (64, -128)):
        assert run(ld_i=ld_i, ld_t=ld_t) == E.BLDP_EINVAL and "strides" in E.last_error()
    assert run(ld_q=255) == E.BLDP_EINVAL and "planes" in E.last_error()
    # the band and host calls make the same checks
    ptrs = (ctypes.c_void_p * 2)(A, A + (1 << 16))
    band = L.bldp_band_dedoppler_f32
    assert band(2, ptrs, 64, 2, 8, None, 1, 3, 16, B, Dp, S, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 8, None, 4, 1025, 16, B, Dp, S, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 8, None, 4, 3, -2, B, Dp, S, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 8, None, 3, 3, 16, B, Dp, S, None) == E.BLDP_EDIM
    assert band(0, ptrs, 64, 2, 8, None, 4, 3, 16, B, Dp, S, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 8, None, 4, 3, 16, None, None, None, None) == E.BLDP_EINVAL
    # (the band's planes are twice a bank's)
    assert band(2, ptrs, 64, 2, 8, None, 4, 3, 16, B, B + 2 * plane - 4, S, None) == E.BLDP_EINVAL
    assert "best and drift" in E.last_error()
    host = L.bldp_dedoppler_host_f32
    assert host(0, A, 64, 2, 8, None, 1, 3, 16, B, Dp, S) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 8, None, 4, 2000, 16, B, Dp, S) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 8, None, 4, 3, -1, B, Dp, S) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 8, None, 5, 3, 16, B, Dp, S) == E.BLDP_EDIM
    assert host(0, None, 64, 2, 8, None, 4, 3, 16, B, Dp, S) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 8, None, 4, 3, 16, B, None, S) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 8, None, 4, 3, 16, None, None, None) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers
    assert run(in_=None, dims=(0, 2, 8), best=None, drift=None, sums=None) == 0
    assert host(0, None, 0, 2, 8, None, 4, 3, 16, None, None, None) == 0


def test_python_checks(pkg):
    import torch

    eng, W = pkg.engine, pkg.worker
    x = torch.zeros(8, 2, 4)
    a = np.zeros((8, 2, 4), np.float32, order="F")
    for bad in (x.double(), x.to(torch.int16), a):
        with pytest.raises(TypeError):
            eng.dedoppler(bad, 2)
    with pytest.raises(TypeError):
        eng.band_dedoppler([x.double()], 2)
    with pytest.raises(TypeError):
        eng.dedoppler_host(a.astype(np.float64), 2)
    for D in (-1, 1025, 1.5):
        with pytest.raises(pkg.ArgumentError, match="maxdrift"):
            eng.dedoppler(x, D)
        with pytest.raises(pkg.ArgumentError, match="maxdrift"):
            eng.dedoppler_host(a, D)
    for T in (1, 0):
        with pytest.raises(pkg.ArgumentError, match="tavby"):
            eng.dedoppler(x, 2, tavby=T)
    with pytest.raises(pkg.ArgumentError, match="tavby"):
        eng.dedoppler(torch.zeros(8, 2, 1), 2)   # the whole range is one spectrum
    with pytest.raises(pkg.ArgumentError, match="seg"):
        eng.dedoppler(x, 2, seg=-4)
    with pytest.raises(pkg.DimensionMismatch):
        eng.dedoppler(x, 2, tavby=3)
    with pytest.raises(pkg.BoundsError):
        eng.dedoppler(x, 2, win=[4, 8, 1, 0, 2, 1, 0, 4, 1])
    # the workers: before any file is touched
    with pytest.raises(ValueError, match="nfpc"):
        W.getdedoppler(a, maxdrift=2)   # an array source must name nfpc
    with pytest.raises(ValueError, match="nfpc"):
        W.getdrifthits(a, maxdrift=2)
    with pytest.raises(ValueError, match="despike"):
        W.getdedoppler(a, maxdrift=2, nfpc=0, despike=True)
    with pytest.raises(TypeError):
        W.getdedoppler(a.astype(np.int8), maxdrift=2, nfpc=4)
    with pytest.raises(ValueError):
        W.getdrifthits("/no/such/file.fil", maxdrift=2, nfpc=4, nsigma=-1.0)


# ---- the symbols and the documents -----------------------------------------------
def test_symbols_everywhere(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    shim = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in NAMES:
        assert name in pkg._lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"BLDP_API int %s\(" % name, hdr)
        assert ":%s" % name in shim
    for fn in ("gpu_dedoppler", "gpu_dedoppler_plan", "gpu_band_dedoppler"):
        assert re.search(r"^function %s\(" % fn, shim, re.M) and fn in shim[:shim.index("const libbldp")]
    assert int(re.search(r"#define BLDP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert "bldp_*dedoppler_*" in hdr[:hdr.index("#define BLDP_ABI_VERSION")]
    assert "#define BLDP_MAX_DRIFT 1024" in hdr and pkg._lib.MAX_DRIFT == 1024
    assert "0 0 1 1 1 2 2 2 3 3 3 4 4 4 5 5" in hdr
    assert pkg._lib.DEDOPPLER_PATHS == {0: "resident", 1: "chunked"}
    for fn in ("dedoppler", "dedoppler_plan", "band_dedoppler", "dedoppler_host", "drift_offsets",
               "drift_rates"):
        assert callable(getattr(pkg.engine, fn))
    assert callable(pkg.getdedoppler) and callable(pkg.getdrifthits)
    assert callable(pkg.GBT.getdedoppler) and callable(pkg.GBT.getdrifthits)
    assert "dedoppler.hip" in open(os.path.join(CSRC, "Makefile")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "dedoppler.hip" in design
    for item in ("Taylor-tree", "typed input", "prepared handles", "multi-device band entry",
                 "term count", "finer than one channel"):
        assert item in design, item
    assert "getdedoppler" in open(os.path.join(REPO, "README.md")).read()
