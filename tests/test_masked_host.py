"""CPU: the masked reduce without a GPU: the NumPy restatement on blocks written
out by hand, the plan entry point with null pointers, every refusal of the rule
(include/bldp.h) with pointers that are never dereferenced, the Python argument
checks, and the symbols."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from masked_ref import masked_ref

NAMES = ("bldp_masked_reduce_plan_f32", "bldp_masked_reduce_f32", "bldp_band_masked_reduce_f32",
         "bldp_masked_reduce_host_f32")
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---- the restatement, on blocks written out by hand --------------------------------
def one_block(vals, flags):
    """A single F x 1 block."""
    a = np.array(vals, dtype=np.float32).reshape(-1, 1, 1)
    m = np.array(flags, dtype=np.uint8).reshape(-1, 1, 1)
    s, k, mean = masked_ref(a, m, len(vals), 1)
    return float(s[0, 0, 0]), int(k[0, 0, 0]), mean[0, 0, 0]


def test_restatement_by_hand():
    assert one_block([1, 2, 3, 4], [0, 0, 0, 0])[:2] == (10.0, 4)
    assert one_block([1, 2, 3, 4], [0, 0, 0, 0])[2] == np.float32(2.5)
    s, k, mean = one_block([1, 2, 3, 4], [1, 1, 1, 1])  # none kept: 0.0 and NaN
    assert (s, k) == (0.0, 0) and np.isnan(mean) and mean.dtype == np.float32
    # a flagged NaN and a flagged Inf beside finite kept samples
    s, k, mean = one_block([1, NAN, 3, INF, -INF, 5], [0, 1, 0, 1, 1, 0])
    assert (s, k) == (9.0, 3) and mean == np.float32(3.0)
    # a kept NaN propagates
    s, k, mean = one_block([1, NAN, 3], [0, 0, 1])
    assert np.isnan(s) and k == 2 and np.isnan(mean)
    # flags 2 and 255 flag like 1
    assert one_block([1, 2, 4, 8], [2, 0, 255, 0])[:2] == (10.0, 2)
    # the mean is the Float32 quotient
    assert one_block([1, 1, 0], [0, 0, 0])[2] == np.float32(2) / np.float32(3)


def test_restatement_blocks_and_broadcast():
    a = np.arange(4 * 2 * 6, dtype=np.float32).reshape(4, 2, 6, order="F")
    m = np.zeros((4, 1, 1), dtype=np.uint8)
    m[1] = 7  # a bad channel
    s, k, _ = masked_ref(a, m, 2, 3)
    assert s.shape == (2, 2, 2) and (k == [[[3, 3], [3, 3]], [[6, 6], [6, 6]]]).all()
    # block (0, 0, 0): channel 0 of spectra 0, 1, 2 = elements 0, 8, 16
    assert s[0, 0, 0] == 0 + 8 + 16 and s[1, 1, 1] == sum(a[2:4, 1, 3:6].ravel())
    # F = T = 1: data = kept ? x : 0
    s, k, _ = masked_ref(a, m, 1, 1)
    assert (s == np.where(np.broadcast_to(m, a.shape) != 0, 0, a)).all() and k.max() == 1


# ---- the plan call: null pointers, no GPU -----------------------------------------
def plan(pkg, L, nchan, nif, ntime, F, T, win=None, ptr=None, mask=None, ld=None):
    info = (ctypes.c_int64 * 10)(*([-1] * 10))
    keep, wp = pkg._lib.win_arg(win)
    mld = (ctypes.c_int64 * 3)(*ld) if ld is not None else None
    rc = L.bldp_masked_reduce_plan_f32(ptr, nchan, nif, ntime, wp, F, T, mask, mld, info)
    assert rc == 0, pkg._lib.last_error()
    d = dict(zip(["path", "lanes", "slices", "f4", "wgs", "ws", "nout", "vec", "mload", "rsv"],
                 [int(v) for v in info]))
    assert d["ws"] == 0 and d["rsv"] == 0
    d["path"] = pkg._lib.ARGEXT_PATHS[d["path"]]
    d["mload"] = pkg._lib.MASK_LOADS[d["mload"]]
    return d


# (F, T): path, lanes, slices, float4 per lane; on (3F, 2, 2T) arrays, (8, 1024) on 8 channels
PLANS = {(1, 1): ("lanes", 1, 1, 0), (4, 1): ("lanes", 1, 1, 1), (64, 16): ("lanes", 16, 1, 1),
         (5, 3): ("lanes", 8, 1, 0), (1024, 16): ("lanes", 64, 1, 4),
         (8, 1024): ("lanes_tsplit", 2, 64, 1), (2048, 1): ("block", 256, 1, 2),
         (4097, 3): ("block", 256, 1, 0)}


def plan_dims(F, T):
    return (8, 1, 2 * T) if (F, T) == (8, 1024) else (3 * F, 2, 2 * T)


@pytest.mark.parametrize("F,T", sorted(PLANS))
def test_plan_forms(pkg, L, F, T):
    path, lanes, slices, f4 = PLANS[(F, T)]
    nchan, nif, ntime = plan_dims(F, T)
    vec = int(F % 4 == 0)
    p = plan(pkg, L, nchan, nif, ntime, F, T)
    assert (p["path"], p["lanes"], p["slices"], p["f4"], p["vec"]) == (path, lanes, slices, f4, vec)
    assert p["nout"] == (nchan // F) * nif * 2
    # the mask load form: a dense mask rides on the float4 loads as dwords
    assert p["mload"] == ("dword" if vec else "byte")
    assert plan(pkg, L, nchan, nif, ntime, F, T, ld=[1, nchan, nchan * nif]) == p
    # a bad-channel list: the pitches are 0, so dwords where the data is float4
    assert plan(pkg, L, nchan, nif, ntime, F, T, ld=[1, 0, 0])["mload"] == p["mload"]
    # a bad-spectrum list: one flag a row
    q = plan(pkg, L, nchan, nif, ntime, F, T, ld=[0, 0, 1])
    assert q["mload"] == "row" and {**q, "mload": p["mload"]} == p
    # a time pitch that is no multiple of 4, a mask off the dword grid: bytes
    assert plan(pkg, L, nchan, nif, ntime, F, T, ld=[1, 0, nchan + 1])["mload"] == "byte"
    assert plan(pkg, L, nchan, nif, ntime, F, T, mask=(1 << 20) + 1)["mload"] == "byte"
    assert plan(pkg, L, nchan, nif, ntime, F, T, mask=(1 << 20) + 4) == p
    # a channel stride of 2 in the mask: bytes
    assert plan(pkg, L, nchan, nif, ntime, F, T, ld=[2, 2 * nchan, 2 * nchan * nif])["mload"] == "byte"
    # data off the dword grid: one dword per element, and so byte flags
    q = plan(pkg, L, nchan, nif, ntime, F, T, ptr=(1 << 20) + 2)
    assert q["vec"] == 0 and q["f4"] == 0 and q["mload"] == "byte"
    # a non-unit channel step: the same
    q = plan(pkg, L, 2 * nchan, nif, ntime, F, T, win=[0, nchan, 2, 0, nif, 1, 0, ntime, 1])
    assert (q["path"], q["vec"], q["f4"], q["mload"]) == (path, 0, 0, "byte")
    if nif == 2:  # an IF pitch that is no multiple of 4 matters only with a second IF
        assert plan(pkg, L, nchan, nif, ntime, F, T, ld=[1, nchan + 2, 4 * nchan])["mload"] == "byte"
        assert plan(pkg, L, nchan, 1, ntime, F, T, ld=[1, nchan + 2, 4 * nchan])["mload"] == p["mload"]


def test_plan_matches_argext(pkg, L):
    """The walk is argext's: the first eight entries are its plan's."""
    for (F, T) in PLANS:
        nchan, nif, ntime = plan_dims(F, T)
        info = (ctypes.c_int64 * 8)()
        assert L.bldp_argext_plan_f32(None, nchan, nif, ntime, None, F, T, 0, None, info) == 0
        p = plan(pkg, L, nchan, nif, ntime, F, T)
        got = [pkg._lib.ARGEXT_PATHS[info[0]]] + [int(v) for v in info[1:]]
        assert got == [p[k] for k in ("path", "lanes", "slices", "f4", "wgs", "ws", "nout", "vec")]
    # an empty window plans without a fault
    assert plan(pkg, L, 256, 1, 4, 8, 1, win=[0, 0, 1, 0, 1, 1, 0, 4, 1])["nout"] == 0


# ---- the refusals of rule 6, before any launch ---------------------------------------
def test_refusals(pkg, L):
    E = pkg._lib
    A, M, O, K = 1 << 20, 2 << 20, 3 << 20, 4 << 20  # never dereferenced
    info = (ctypes.c_int64 * 10)()

    def run(in_=A, dims=(64, 2, 4), F=4, T=2, op=0, mask=M, ld=None, out=O, kept=K, ld_i=16,
            ld_t=32, win=None):
        keep, wp = E.win_arg(win)
        mld = (ctypes.c_int64 * 3)(*ld) if ld is not None else None
        return L.bldp_masked_reduce_f32(in_, *dims, wp, F, T, op, mask, mld, out, kept, ld_i, ld_t,
                                        None)

    # rule 5: every op but sum and mean (the plan call has none)
    for op in (2, 3, 4, 5, 6, 7, 8, -1, 64):
        assert run(op=op) == E.BLDP_EINVAL and "sum" in E.last_error()
    # F * T = 2^31 is beyond Int32; 2^31 - 2^16 is not
    assert L.bldp_masked_reduce_plan_f32(None, 65536, 1, 32768, None, 65536, 32768, None, None,
                                         info) == E.BLDP_EINVAL and "2^31" in E.last_error()
    assert L.bldp_masked_reduce_plan_f32(None, 65536, 1, 32767, None, 65536, 32767, None, None,
                                         info) == 0
    assert L.bldp_masked_reduce_plan_f32(None, 64, 1, 4, None, 4, 1, None, None, None) == E.BLDP_EINVAL
    # both outputs null, a null mask, a null input
    assert run(out=None, kept=None) == E.BLDP_EINVAL and "both null" in E.last_error()
    assert run(mask=None) == E.BLDP_EINVAL and "null mask" in E.last_error()
    assert run(in_=None) == E.BLDP_EINVAL and "null input" in E.last_error()
    # negative mask strides
    for ld in ([-1, 64, 128], [1, -64, 128], [1, 64, -128]):
        assert run(ld=ld) == E.BLDP_EINVAL and "negative" in E.last_error()
    # outputs over each other, over the input window, over the mask's span
    nout_bytes = 4 * (16 * 2 * 2)
    assert run(kept=O + nout_bytes - 4) == E.BLDP_EINVAL and "out and kept" in E.last_error()
    assert run(out=A + 4 * (64 * 2 * 4) - 4) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(kept=A) == E.BLDP_EINVAL and "input window" in E.last_error()
    assert run(out=M + 64 * 2 * 4 - 1) == E.BLDP_EINVAL and "the mask" in E.last_error()
    assert run(kept=M - nout_bytes + 1) == E.BLDP_EINVAL and "the mask" in E.last_error()
    # ... the span of a broadcast mask is what its strides reach: 64 bytes here
    assert run(out=M + 63, ld=[1, 0, 0]) == E.BLDP_EINVAL and "the mask" in E.last_error()
    # output strides that overlap
    assert run(ld_i=15) == E.BLDP_EINVAL and "strides" in E.last_error()
    assert run(ld_t=31) == E.BLDP_EINVAL and "strides" in E.last_error()
    # factors that do not divide the window; a window outside the array
    assert run(F=3) == E.BLDP_EDIM and "fqavby=3" in E.last_error()
    assert run(T=3) == E.BLDP_EDIM and "tavby=3" in E.last_error()
    assert run(win=[60, 8, 1, 0, 2, 1, 0, 4, 1]) == E.BLDP_EBOUNDS
    # the band and host calls make the same checks
    ptrs = (ctypes.c_void_p * 2)(A, A + (1 << 16))
    band = L.bldp_band_masked_reduce_f32
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 2, M, None, O, K, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 0, None, None, O, K, None) == E.BLDP_EINVAL
    assert "null mask" in E.last_error()
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 0, M, None, None, None, None) == E.BLDP_EINVAL
    assert band(2, ptrs, 64, 2, 4, None, 5, 2, 0, M, None, O, K, None) == E.BLDP_EDIM
    assert band(0, ptrs, 64, 2, 4, None, 4, 2, 0, M, None, O, K, None) == E.BLDP_EINVAL
    # (the dense band mask spans both banks: 2 * 64 * 2 * 4 bytes)
    assert band(2, ptrs, 64, 2, 4, None, 4, 2, 0, M, None, M + 1023, K, None) == E.BLDP_EINVAL
    assert "the mask" in E.last_error()
    host = L.bldp_masked_reduce_host_f32
    assert host(0, A, 64, 2, 4, None, 4, 2, 3, M, None, O, K) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 3, 2, 0, M, None, O, K) == E.BLDP_EDIM
    assert host(0, A, 64, 2, 4, None, 4, 2, 0, None, None, O, K) == E.BLDP_EINVAL
    assert host(0, A, 64, 2, 4, None, 4, 2, 0, M, None, None, None) == E.BLDP_EINVAL
    neg = (ctypes.c_int64 * 3)(1, -1, 0)
    assert host(0, A, 64, 2, 4, None, 4, 2, 0, M, neg, O, K) == E.BLDP_EINVAL
    # an empty result launches nothing and needs no pointers
    assert run(in_=None, dims=(64, 2, 0), mask=None, out=None, kept=None) == 0
    assert host(0, None, 64, 2, 0, None, 4, 2, 0, None, None, None, None) == 0


# ---- Python: TypeError and ValueError before any GPU work -------------------------
def test_python_checks(pkg):
    import torch

    eng, W = pkg.engine, pkg.worker
    x = torch.zeros(8, 2, 4)
    m = torch.zeros(8, 2, 4, dtype=torch.uint8)
    with pytest.raises(TypeError):
        eng.masked_reduce(x.double(), m)
    with pytest.raises(TypeError):
        eng.masked_reduce(x.to(torch.int16), m)
    for bad in (m.float(), m.to(torch.int8), m.numpy(), None):
        with pytest.raises(TypeError):
            eng.masked_reduce(x, bad)
    for shape in ((8, 2, 3), (4, 2, 4), (8, 2), (8, 2, 4, 1), (2, 1, 1)):
        with pytest.raises(ValueError, match="mask"):
            eng.masked_reduce(x, torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):  # the window's shape, not the array's
        eng.masked_reduce(x, m, win=[0, 4, 1, 0, 2, 1, 0, 4, 1])
    for op in ("max", "min", "median", "var", "argmax", 0):
        with pytest.raises(ValueError, match="sum"):
            eng.masked_reduce(x, m, op=op)
        with pytest.raises(ValueError, match="sum"):
            eng.masked_reduce_host(np.zeros((8, 2, 4), np.float32, order="F"), m.numpy(), op=op)
    with pytest.raises(TypeError):  # a host mask of the right shape is still no device tensor
        eng.masked_reduce(x, m)
    with pytest.raises(TypeError):
        eng.band_masked_reduce([x.double()], m)
    with pytest.raises(ValueError, match="mask"):  # the band's mask covers every bank
        eng.band_masked_reduce([x, x], m)
    a = np.zeros((8, 2, 4), np.float32, order="F")
    with pytest.raises(TypeError):
        eng.masked_reduce_host(a.astype(np.float64), m.numpy())
    with pytest.raises(TypeError):
        eng.masked_reduce_host(a, m.numpy().astype(np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.masked_reduce_host(a, np.zeros((8, 2, 5), np.uint8))
    # the worker: before any file is touched
    with pytest.raises(ValueError):
        W.getmasked("/no/such/file.fil", mask=m.numpy(), func="max")
    with pytest.raises(TypeError):
        W.getmasked("/no/such/file.fil", mask=np.zeros((8, 2, 4), np.float32))
    with pytest.raises(TypeError):
        W.getmasked(a.astype(np.int8), mask=m.numpy())
    with pytest.raises(ValueError):
        W.getclean("/no/such/file.fil", axis=1)
    with pytest.raises(ValueError):
        W.getclean("/no/such/file.fil", nsigma=-1.0)
    with pytest.raises(ValueError):
        W.getclean("/no/such/file.fil", func="median")
    with pytest.raises(TypeError):
        W.getclean(a.astype(np.uint8), n=2)


# ---- the symbols and the documents -----------------------------------------------
def test_symbols_everywhere(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    shim = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in NAMES:
        assert name in pkg._lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"BLDP_API int %s\(" % name, hdr)
    for name in NAMES[1:]:
        assert ":%s" % name in shim
    assert "gpu_masked_reduce" in shim and "gpu_band_masked_reduce" in shim
    assert int(re.search(r"#define BLDP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert pkg._lib.MASK_LOADS == {0: "byte", 1: "dword", 2: "row"}
    for fn in ("masked_reduce", "masked_reduce_plan", "band_masked_reduce", "masked_reduce_host"):
        assert callable(getattr(pkg.engine, fn))
    assert callable(pkg.getmasked) and callable(pkg.getclean) and callable(pkg.GBT.getclean)
    assert "masked.hip" in open(os.path.join(REPO, "DESIGN.md")).read()
