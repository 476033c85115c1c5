"""CPU: the hits list without a GPU: the NumPy restatement on blocks written out
by hand, the plan entry point with null pointers, every refusal of the rule
(include/bldp.h) with pointers that are never dereferenced, the Python argument
checks, hits_unravel, the snr formula, and the symbols."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from hits_ref import hits_ref, snr_ref

NAMES = ("bldp_hits_plan_f32", "bldp_hits_f32", "bldp_band_hits_f32", "bldp_hits_host_f32")
MAX_TILES = 8192     # include/bldp.h: at most 8192 tiles cover the window
SCAN_CHUNK = 2048    # tiles of one pass of the scan workgroup (256 lanes x 8)
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---- the restatement, on blocks written out by hand --------------------------------
def coords(pkg, idx, wshape):
    """engine.hits_unravel's (channel, if, time) of a list, as lists."""
    return [v.tolist() for v in pkg.engine.hits_unravel(idx, wshape)]


def test_restatement_by_hand(pkg):
    a = np.arange(24, dtype=np.float32).reshape(4, 2, 3, order="F")  # a[c, i, t] = c + 4*(i + 2*t)
    m = np.zeros((4, 2, 3), dtype=np.uint8)
    m[1, 0, 0], m[3, 1, 0], m[0, 0, 2], m[2, 1, 2] = 1, 2, 255, 1
    total, idx, val = hits_ref(a, m)
    assert total == 4 and idx.tolist() == [1, 7, 16, 22] and idx.dtype == np.int64
    assert val.tolist() == [1.0, 7.0, 16.0, 22.0] and val.dtype == np.float32
    # ... and the binding's hits_unravel gives back the samples that were flagged
    assert coords(pkg, idx, a.shape) == [[1, 3, 0, 2], [0, 1, 0, 1], [0, 0, 2, 2]]
    # the lists are cut, the total is not
    total, idx, val = hits_ref(a, m, cap=2)
    assert total == 4 and idx.tolist() == [1, 7] and val.tolist() == [1.0, 7.0]
    assert hits_ref(a, m, cap=0)[0] == 4 and hits_ref(a, m, cap=0)[1].size == 0
    assert hits_ref(a, m, cap=9)[1].tolist() == [1, 7, 16, 22]
    # nothing flagged, everything flagged
    assert hits_ref(a, np.zeros_like(m)) [0] == 0
    total, idx, val = hits_ref(a, np.ones_like(m))
    assert total == 24 and (idx == np.arange(24)).all() and (val == np.arange(24)).all()
    # the order is Julia's findall: the same as the column-major nonzero
    assert idx.tolist() == [c + 4 * (i + 2 * t) for t in range(3) for i in range(2)
                            for c in range(4)]


def test_restatement_broadcasts_and_bits(pkg):
    a = np.arange(24, dtype=np.float32).reshape(4, 2, 3, order="F")
    chan = np.zeros((4, 1, 1), dtype=np.uint8)
    chan[2] = 9   # a bad channel: every (i, t) of channel 2
    assert hits_ref(a, chan)[1].tolist() == [2, 6, 10, 14, 18, 22]
    assert coords(pkg, hits_ref(a, chan)[1], a.shape) == [[2] * 6, [0, 1] * 3, [0, 0, 1, 1, 2, 2]]
    spec = np.zeros((1, 1, 3), dtype=bool)
    spec[0, 0, 1] = True   # a bad spectrum: a contiguous run
    assert hits_ref(a, spec)[1].tolist() == list(range(8, 16))
    assert coords(pkg, hits_ref(a, spec)[1], a.shape)[2] == [1] * 8
    # the broadcast forms are the ones the binding's stride rule takes: stride 0 on an axis of 1
    for msk, want in ((chan, [1, 0, 0]), (spec, [0, 0, 1])):
        m = np.asfortranarray(msk)
        assert pkg.engine._mask_strides(m.shape, m.strides, a.shape, "t") == want
    ifs = np.zeros((1, 2, 1), dtype=np.uint8)
    ifs[0, 1] = 1
    assert hits_ref(a, ifs)[1].tolist() == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23]
    # the values' bits are untouched: a NaN payload, -0.0, a denormal
    bits = np.array([0x7fc01234, 0x80000000, 0x00000001, 0xff800000], dtype=np.uint32)
    b = bits.view(np.float32).reshape(4, 1, 1)
    _, idx, val = hits_ref(b, np.ones((4, 1, 1), np.uint8))
    assert (val.view(np.uint32) == bits).all()


def test_unravel_and_snr(pkg):
    eng = pkg.engine
    rng = np.random.default_rng(3)
    for wshape in ((7, 3, 5), (1, 1, 9), (64, 1, 1), (5, 2, 1)):
        k = np.sort(rng.choice(int(np.prod(wshape)), size=min(9, int(np.prod(wshape))),
                               replace=False)).astype(np.int64)
        c, i, t = eng.hits_unravel(k, wshape)
        wc, wi, wt = np.unravel_index(k, wshape, order="F")
        assert (c == wc).all() and (i == wi).all() and (t == wt).all()
    with pytest.raises(ValueError):
        eng.hits_unravel(np.zeros(1, np.int64), (0, 1, 1))
    # snr on a hand-made list: Float64 arithmetic on Float32 inputs, signed
    val = np.array([10.0, -2.0, 0.1, 3.0], np.float32)
    med = np.array([4.0, 4.0, 0.0, 3.0], np.float32)
    mad = np.array([2.0, 3.0, 0.3, 0.0], np.float32)
    got = eng.hits_snr(val, med, mad)
    assert got.dtype == np.float64
    assert got[0] == 3.0 and got[1] == -2.0
    assert got[2] == float(np.float32(0.1)) / float(np.float32(0.3))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(got[3])   # 0 / 0: a block with a zero mad flags nothing anyway
    assert (snr_ref(val, med, mad)[:3] == got[:3]).all()
    import torch

    tv = eng.hits_snr(torch.from_numpy(val), torch.from_numpy(med), torch.from_numpy(mad))
    assert tv.dtype == torch.float64 and (tv[:3].numpy() == got[:3]).all()


# ---- the plan call: null pointers, no GPU -----------------------------------------
KEYS = ["mload", "tile", "tiles", "ws", "chunks", "per_load", "launches", "r7", "r8", "r9"]


def plan(pkg, L, nchan, nif, ntime, win=None, ptr=None, mask=None, ld=None, cap=1):
    info = (ctypes.c_int64 * 10)(*([-1] * 10))
    keep, wp = pkg._lib.win_arg(win)
    mld = (ctypes.c_int64 * 3)(*ld) if ld is not None else None
    rc = L.bldp_hits_plan_f32(ptr, nchan, nif, ntime, wp, mask, mld, cap, info)
    assert rc == 0, pkg._lib.last_error()
    d = dict(zip(KEYS, [int(v) for v in info]))
    assert d["r7"] == d["r8"] == d["r9"] == 0
    d["mload"] = pkg._lib.HITS_LOADS[d["mload"]]
    return d


def test_plan_mask_forms(pkg, L):
    P = lambda *a, **k: plan(pkg, L, *a, **k)  # noqa: E731
    # dense: the widest aligned load that nc allows
    assert (P(64, 2, 4)["mload"], P(64, 2, 4)["per_load"]) == ("wide", 16)
    assert (P(12, 2, 4)["mload"], P(12, 2, 4)["per_load"]) == ("wide", 4)
    assert (P(6, 2, 4)["mload"], P(6, 2, 4)["per_load"]) == ("byte", 1)
    assert (P(65, 2, 4)["mload"], P(65, 2, 4)["per_load"]) == ("byte", 1)
    assert P(64, 2, 4, ld=[1, 64, 128]) == P(64, 2, 4)
    # a bad-channel list: the pitches are 0
    assert P(64, 2, 4, ld=[1, 0, 0])["per_load"] == 16
    # a bad-spectrum list and an IF list: one flag a row
    for ld in ([0, 0, 1], [0, 1, 0], [0, 1, 2]):
        q = P(64, 2, 4, ld=ld)
        assert (q["mload"], q["per_load"]) == ("row", 1)
    # a mask off the 16-byte grid: dwords; off the dword grid: bytes
    assert P(64, 2, 4, mask=(1 << 20) + 16)["per_load"] == 16
    assert P(64, 2, 4, mask=(1 << 20) + 4)["per_load"] == 4
    assert P(64, 2, 4, mask=(1 << 20) + 1)["mload"] == "byte"
    # pitches: multiples of the width where the axis is longer than 1
    assert P(64, 2, 4, ld=[1, 68, 136])["per_load"] == 4
    assert P(64, 2, 4, ld=[1, 64, 129])["mload"] == "byte"
    assert P(64, 1, 4, ld=[1, 65, 128])["per_load"] == 16   # (a single IF: its pitch is unused)
    assert P(64, 2, 1, ld=[1, 64, 3])["per_load"] == 16
    # a channel stride of 2 in the mask: bytes
    assert P(64, 2, 4, ld=[2, 128, 256])["mload"] == "byte"
    # the data's alignment, offset, step and direction do not matter: only flagged samples
    # are gathered
    assert P(64, 2, 4, ptr=(1 << 20) + 2) == P(64, 2, 4)
    assert P(200, 2, 4, win=[3, 64, 2, 0, 2, 1, 0, 4, 1]) == P(64, 2, 4)
    assert P(64, 2, 4, win=[63, 64, -1, 0, 2, 1, 0, 4, 1]) == P(64, 2, 4)
    # the window's nc decides, not the array's
    assert P(64, 2, 4, win=[0, 6, 1, 0, 2, 1, 0, 4, 1])["mload"] == "byte"


@pytest.mark.parametrize("dims", [(1, 1, 1), (63, 1, 1), (64, 1, 1), (65, 1, 1), (255, 1, 1),
                                  (256, 1, 1), (257, 1, 1), (1024, 1, 1), (1025, 1, 1),
                                  (16384, 1, 1), (16384, 1, 3), (6, 2, 100000), (4, 1, 3000000),
                                  (1 << 20, 1, 16), (65, 3, 40000), (1 << 26, 1, 16),
                                  (1 << 26, 2, 1 << 10), (1 << 26, 1, 1 << 18)])
def test_plan_tiles(pkg, L, dims):
    N = dims[0] * dims[1] * dims[2]
    for ld in (None, [0, 1, dims[1]], [3, 3 * dims[0], 3 * dims[0] * dims[1]]):
        p = plan(pkg, L, *dims, ld=ld)
        W = p["per_load"]
        assert p["tile"] % (256 * W) == 0 and p["tile"] <= 1 << 31
        assert p["tiles"] * p["tile"] >= N > (p["tiles"] - 1) * p["tile"]
        assert 1 <= p["tiles"] <= MAX_TILES
        assert p["ws"] == 12 * p["tiles"]   # a uint64 offset and a uint32 count a tile
        assert p["chunks"] == -(-p["tiles"] // SCAN_CHUNK)
        assert p["launches"] == 3
        # the tile is the smallest that stays under the cap: 4 steps, doubled
        assert p["tile"] == 1024 * W or -(-N // (p["tile"] // 2)) > MAX_TILES
        q = plan(pkg, L, *dims, ld=ld, cap=0)   # count-only: no list launch
        assert q["launches"] == 2 and {**q, "launches": 3} == p
        assert plan(pkg, L, *dims, ld=ld, cap=1 << 40) == p


def test_plan_scan_loops_and_empty(pkg, L):
    # more tiles than one pass of the scan workgroup covers, on a small window
    p = plan(pkg, L, 6, 1, 400000)
    assert p["mload"] == "byte" and p["tiles"] > SCAN_CHUNK and p["chunks"] == 2
    assert plan(pkg, L, 1 << 26, 1, 16)["chunks"] == 4
    # an empty window plans nothing
    z = plan(pkg, L, 256, 1, 4, win=[0, 0, 1, 0, 1, 1, 0, 4, 1])
    assert z["tiles"] == 0 and z["launches"] == 0 and z["ws"] == 0


# ---- the refusals of rule 7, before any launch ---------------------------------------
def test_refusals(pkg, L):
    E = pkg._lib
    A, M, X, V, T = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20  # never dereferenced
    info = (ctypes.c_int64 * 10)()

    def run(in_=A, dims=(64, 2, 4), mask=M, ld=None, cap=100, idx=X, val=V, total=T, win=None):
        keep, wp = E.win_arg(win)
        mld = (ctypes.c_int64 * 3)(*ld) if ld is not None else None
        return L.bldp_hits_f32(in_, *dims, wp, mask, mld, cap, idx, val, total, None)

    # a null total, a null mask, a null input, a negative cap
    assert run(total=None) == E.BLDP_EINVAL and "null total" in E.last_error()
    assert run(total=None, cap=0, idx=None, val=None) == E.BLDP_EINVAL
    assert run(mask=None) == E.BLDP_EINVAL and "null mask" in E.last_error()
    assert run(in_=None) == E.BLDP_EINVAL and "null input" in E.last_error()
    assert run(cap=-1) == E.BLDP_EINVAL and "cap" in E.last_error()
    assert L.bldp_hits_plan_f32(None, 64, 2, 4, None, None, None, -1, info) == E.BLDP_EINVAL
    assert L.bldp_hits_plan_f32(None, 64, 2, 4, None, None, None, 1, None) == E.BLDP_EINVAL
    # negative mask strides
    for ld in ([-1, 64, 128], [1, -64, 128], [1, 64, -128]):
        assert run(ld=ld) == E.BLDP_EINVAL and "negative" in E.last_error()
    # outputs over each other: idx holds 8 * min(cap, N) bytes, val 4 *, total 8
    assert run(val=X + 799) == E.BLDP_EINVAL and "idx and val" in E.last_error()
    assert run(total=X + 792) == E.BLDP_EINVAL and "idx and total" in E.last_error()
    assert run(total=V + 399) == E.BLDP_EINVAL and "val and total" in E.last_error()
    assert run(idx=V - 1) == E.BLDP_EINVAL and "idx and val" in E.last_error()
    # ... a cap beyond the window counts as the window: 512 entries
    assert run(cap=1 << 50, val=X + 8 * 512 - 1) == E.BLDP_EINVAL and "idx and val" in E.last_error()
    # ... over the input window (64 * 2 * 4 floats), over the mask's span
    assert run(idx=A + 4 * 512 - 1) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(val=A - 399) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(total=A) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(idx=M + 511) == E.BLDP_EINVAL and "the mask" in E.last_error()
    assert run(total=M - 7) == E.BLDP_EINVAL and "the mask" in E.last_error()
    # ... the span of a broadcast mask is what its strides reach: 64 bytes here
    assert run(val=M + 63, ld=[1, 0, 0]) == E.BLDP_EINVAL and "the mask" in E.last_error()
    # ... only the window's elements count: the other half of the channels is free
    assert run(dims=(128, 2, 4), win=[0, 64, 1, 0, 1, 1, 0, 1, 1], total=A + 4 * 64 - 1) \
        == E.BLDP_EINVAL
    # more tiles than one launch takes: 2^46 elements are more than 8192 tiles of 2^31
    big = (1 << 26, 1, 1 << 20)
    assert run(dims=big) == E.BLDP_EINVAL and "too many" in E.last_error()
    assert L.bldp_hits_plan_f32(None, *big, None, None, None, 1, info) == E.BLDP_EINVAL
    assert "too many" in E.last_error()
    assert L.bldp_hits_plan_f32(None, 1 << 26, 1, 1 << 18, None, None, None, 1, info) == 0
    # a window outside the array
    assert run(win=[60, 8, 1, 0, 2, 1, 0, 4, 1]) == E.BLDP_EBOUNDS
    assert run(win=[0, 8, 1, 0, 2, 1, 3, 2, 1]) == E.BLDP_EBOUNDS
    # the band and host calls make the same checks
    ptrs = (ctypes.c_void_p * 2)(A, A + (1 << 16))
    band = L.bldp_band_hits_f32
    assert band(2, ptrs, 64, 2, 4, None, None, None, 10, X, V, T, None) == E.BLDP_EINVAL
    assert "null mask" in E.last_error()
    assert band(2, ptrs, 64, 2, 4, None, M, None, 10, X, V, None, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, M, None, -2, X, V, T, None) == E.BLDP_EINVAL
    assert band(0, ptrs, 64, 2, 4, None, M, None, 10, X, V, T, None) == E.BLDP_EINVAL
    assert band(65, ptrs, 64, 2, 4, None, M, None, 10, X, V, T, None) == E.BLDP_EINVAL
    # (the dense band mask spans both banks: 2 * 64 * 2 * 4 bytes)
    assert band(2, ptrs, 64, 2, 4, None, M, None, 10, M + 1023, V, T, None) == E.BLDP_EINVAL
    assert "the mask" in E.last_error()
    assert band(2, ptrs, 64, 2, 4, None, M, None, 10, X, A + (1 << 16), T, None) == E.BLDP_EINVAL
    assert "bank 1" in E.last_error()
    assert band(2, ptrs, 64, 2, 9, E.win_arg([0, 64, 1, 0, 2, 1, 8, 2, 1])[1], M, None, 10, X, V,
                T, None) == E.BLDP_EBOUNDS
    host = L.bldp_hits_host_f32
    tot = ctypes.c_uint64(7)
    assert host(0, A, 64, 2, 4, None, M, None, -1, X, V, ctypes.byref(tot)) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, M, None, 10, X, V, None) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, None, None, 10, X, V, ctypes.byref(tot)) == E.BLDP_EINVAL
    assert host(0, None, 64, 2, 4, None, M, None, 10, X, V, ctypes.byref(tot)) == E.BLDP_EINVAL
    neg = (ctypes.c_int64 * 3)(1, -1, 0)
    assert host(0, A, 64, 2, 4, None, M, neg, 10, X, V, ctypes.byref(tot)) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, E.win_arg([0, 64, 1, 0, 3, 1, 0, 4, 1])[1], M, None, 10, X, V,
                ctypes.byref(tot)) == E.BLDP_EBOUNDS
    # an empty window on the host: total = 0, nothing launched, no pointers needed
    tot.value = 7
    assert host(0, None, 64, 2, 0, None, None, None, 10, None, None, ctypes.byref(tot)) == 0
    assert tot.value == 0


# ---- Python: TypeError and ValueError before any GPU work -------------------------
def test_python_checks(pkg):
    import torch

    eng, W = pkg.engine, pkg.worker
    x = torch.zeros(8, 2, 4)
    m = torch.zeros(8, 2, 4, dtype=torch.uint8)
    for bad in (x.double(), x.to(torch.int16), x.to(torch.uint8), x.to(torch.int8)):
        with pytest.raises(TypeError):
            eng.hits(bad, m)
    for bad in (m.float(), m.to(torch.int8), m.numpy(), None):
        with pytest.raises(TypeError):
            eng.hits(x, bad)
    for shape in ((8, 2, 3), (4, 2, 4), (8, 2), (8, 2, 4, 1), (2, 1, 1)):
        with pytest.raises(ValueError, match="mask"):
            eng.hits(x, torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):  # the window's shape, not the array's
        eng.hits(x, m, win=[0, 4, 1, 0, 2, 1, 0, 4, 1])
    for fn in (eng.hits, eng.hits_plan):
        with pytest.raises(ValueError, match="maxhits"):
            fn(x, m, maxhits=-1)
        for bad in (1.5, "3", True):
            with pytest.raises(TypeError, match="maxhits"):
                fn(x, m, maxhits=bad)
    # a CPU torch tensor of the right shape and dtype is still no device tensor
    with pytest.raises(TypeError, match="must be a device tensor"):
        eng.hits(x, m)
    with pytest.raises(TypeError, match="uint8 or bool device tensor"):  # nor is a host array
        eng.hits(x, m.numpy())
    with pytest.raises(TypeError):
        eng.band_hits([x.double()], m)
    with pytest.raises(ValueError):
        eng.band_hits([], m)
    with pytest.raises(ValueError, match="mask"):  # the band's mask covers every bank
        eng.band_hits([x, x], m)
    with pytest.raises(ValueError, match="maxhits"):
        eng.band_hits([x, x], m, maxhits=-3)
    a = np.zeros((8, 2, 4), np.float32, order="F")
    for bad in (a.astype(np.float64), a.astype(np.uint8), a.astype(np.int8)):
        with pytest.raises(TypeError):
            eng.hits_host(bad, m.numpy())
    with pytest.raises(TypeError):
        eng.hits_host(a, m.numpy().astype(np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.hits_host(a, np.zeros((8, 2, 5), np.uint8))
    with pytest.raises(ValueError, match="maxhits"):
        eng.hits_host(a, m.numpy(), maxhits=-1)
    # the worker: before any file is touched
    with pytest.raises(ValueError, match="maxhits"):
        W.getflagged("/no/such/file.fil", mask=m.numpy(), maxhits=-1)
    with pytest.raises(TypeError):
        W.getflagged("/no/such/file.fil", mask=np.zeros((8, 2, 4), np.float32))
    with pytest.raises(TypeError):
        W.getflagged(a.astype(np.int8), mask=m.numpy())
    with pytest.raises(TypeError):
        W.getflagged(a.astype(np.uint8), mask=m.numpy())
    with pytest.raises(ValueError):
        W.gethits("/no/such/file.fil", axis=1)
    with pytest.raises(ValueError):
        W.gethits("/no/such/file.fil", nsigma=-1.0)
    with pytest.raises(ValueError, match="maxhits"):
        W.gethits("/no/such/file.fil", maxhits=-1)
    with pytest.raises(TypeError):
        W.gethits(a.astype(np.uint8), n=2)
    with pytest.raises(TypeError):
        W.gethits(a.astype(np.int8))


# ---- the symbols and the documents -----------------------------------------------
def test_symbols_everywhere(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    shim = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in NAMES:
        assert name in pkg._lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"BLDP_API int %s\(" % name, hdr)
        assert ":%s" % name in shim
    assert "gpu_hits" in shim and "gpu_band_hits" in shim
    assert int(re.search(r"#define BLDP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert pkg._lib.HITS_LOADS == {0: "byte", 1: "wide", 2: "row"}
    for fn in ("hits", "hits_plan", "band_hits", "hits_host", "hits_unravel", "hits_snr"):
        assert callable(getattr(pkg.engine, fn))
    assert callable(pkg.gethits) and callable(pkg.getflagged)
    assert callable(pkg.GBT.gethits) and callable(pkg.GBT.getflagged)
    mk = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "csrc", "Makefile")).read()
    assert "hits.hip" in mk
    assert "hits.hip" in open(os.path.join(REPO, "DESIGN.md")).read()
