"""CPU: fqavfunc "argmax" / "argmin" without a GPU: the op codes, the plan entry
point with null pointers, the argument checks of the ABI, the host rule for the
element types the kernels do not take (worker._host_argext) against literal
loops of Julia's rule, the worker / GBT routing errors, and the Julia shim."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def test_op_codes_and_paths(pkg):
    assert pkg._lib.ARG_OPS == {"argmax": 0, "argmin": 1}
    assert not set(pkg._lib.ARG_OPS) & set(pkg._lib.OPS)  # the output type differs
    assert pkg._lib.ARGEXT_PATHS == {0: "lanes", 1: "lanes_tsplit", 2: "block"}
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    assert re.search(r"enum bldp_argop \{ BLDP_ARG_MAX = 0, BLDP_ARG_MIN = 1 \}", hdr)
    assert "int32_t" not in re.sub(r"uint32_t", "", hdr)  # the index type is uint32_t
    assert int(re.search(r"#define BLDP_ABI_VERSION (\d+)", hdr).group(1)) == 5


def plan(pkg, L, nchan, nif, ntime, F, T, argop=0, win=None, ptr=None):
    info = (ctypes.c_int64 * 8)()
    keep, wp = pkg._lib.win_arg(win)
    rc = L.bldp_argext_plan_f32(ptr, nchan, nif, ntime, wp, F, T, argop, None, info)
    assert rc == 0, pkg._lib.last_error()
    return dict(zip(["path", "lanes", "slices", "f4", "wgs", "ws", "nout", "vec"],
                    [int(v) for v in info]))


@pytest.mark.parametrize("T", [1, 16, 1024])
@pytest.mark.parametrize("F", [2, 64, 1024, 4096])
def test_plan_needs_no_gpu(pkg, L, F, T):
    p = plan(pkg, L, 5 * F, 2, 3 * T, F, T)
    name = pkg._lib.ARGEXT_PATHS[p["path"]]
    assert p["nout"] == 5 * 2 * 3 and p["ws"] == 0
    if F <= 1024:
        assert name in ("lanes", "lanes_tsplit")
        assert p["lanes"] == (2 if F == 2 else min(64, F // 4))
        assert (p["slices"] > 1) == (name == "lanes_tsplit")
        # 30 blocks never fill the GPU: rows are split once T holds 16 rows a slice
        assert (name == "lanes_tsplit") == (T >= 32)
        assert p["wgs"] == -(-30 // (256 // (p["lanes"] * p["slices"])))
    else:
        assert name == "block" and p["lanes"] == 256 and p["slices"] == 1 and p["wgs"] == 30
    assert p["vec"] == (F % 4 == 0) and (p["f4"] > 0) == bool(p["vec"])
    # argmin plans the same launch; a pointer off the dword grid loses the float4 loads
    assert plan(pkg, L, 5 * F, 2, 3 * T, F, T, argop=1) == p
    assert plan(pkg, L, 5 * F, 2, 3 * T, F, T, ptr=(1 << 20) + 2)["vec"] == 0
    assert plan(pkg, L, 5 * F, 2, 3 * T, F, T, ptr=(1 << 20) + 4)["vec"] == p["vec"]


def test_plan_product_shapes(pkg, L):
    # one 0002 file at F = 64: 16 lanes of one float4, no split (278528 blocks)
    p = plan(pkg, L, 65536, 1, 272, 64, 1)
    assert (p["path"], p["lanes"], p["slices"], p["f4"], p["wgs"]) == (0, 16, 1, 1, 65536 * 272 // 64 // 16)
    # one 0001 bank at F = 8, T = 1024: 54976 blocks of 2 lanes, rows over the waves
    p = plan(pkg, L, 512, 1, 879616, 8, 1024)
    assert p["path"] == 1 and p["lanes"] == 2 and p["slices"] == 4
    # ... and T = nt: 64 blocks, 128 slices of a workgroup each
    p = plan(pkg, L, 512, 1, 879616, 8, 879616)
    assert p["path"] == 1 and p["slices"] == 128 and p["wgs"] == 64
    # blocks of one element: still a plan (index 0, the value copied)
    p = plan(pkg, L, 64, 2, 8, 1, 0)
    assert p["path"] == 0 and p["lanes"] == 1 and p["nout"] == 64 * 2 * 8
    # a stepped window: one dword per element
    assert plan(pkg, L, 256, 1, 4, 8, 1, win=[0, 128, 2, 0, 1, 1, 0, 4, 1])["vec"] == 0
    # an empty window plans without a fault
    assert plan(pkg, L, 256, 1, 4, 8, 1, win=[0, 0, 1, 0, 1, 1, 0, 4, 1])["nout"] == 0


def test_abi_errors(pkg, L):
    E = pkg._lib
    info = (ctypes.c_int64 * 8)()

    def call(nchan, nif, ntime, F, T, argop=0, win=None):
        keep, wp = E.win_arg(win)
        return L.bldp_argext_plan_f32(None, nchan, nif, ntime, wp, F, T, argop, None, info)

    assert call(100, 1, 10, 3, 1) == E.BLDP_EDIM and "fqavby=3" in E.last_error()
    assert call(100, 1, 10, 4, 3) == E.BLDP_EDIM and "tavby=3" in E.last_error()
    assert call(100, 1, 10, 4, 1, win=[90, 20, 1, 0, 1, 1, 0, 10, 1]) == E.BLDP_EBOUNDS
    for bad in (2, -1, 6):
        assert call(64, 1, 4, 4, 1, argop=bad) == E.BLDP_EINVAL and "argop" in E.last_error()
    # F * T = 2^31 is beyond the 31-bit offsets; 2^31 - 2^16 is not
    assert call(65536, 1, 32768, 65536, 32768) == E.BLDP_EINVAL and "2^31" in E.last_error()
    assert call(65536, 1, 32767, 65536, 32767) == 0
    assert L.bldp_argext_plan_f32(None, 64, 1, 4, None, 4, 1, 0, None, None) == E.BLDP_EINVAL
    # the launching entry points: the same checks first, then the pointers
    A = 1 << 20
    assert L.bldp_argext_f32(None, 64, 1, 4, None, 4, 1, 0, A, None, 16, 16, None) == E.BLDP_EINVAL
    assert "null input" in E.last_error()
    assert L.bldp_argext_f32(A, 64, 1, 4, None, 4, 1, 0, None, None, 16, 16, None) == E.BLDP_EINVAL
    assert "idx" in E.last_error()
    assert L.bldp_argext_f32(A, 64, 1, 4, None, 3, 1, 0, None, None, 16, 16, None) == E.BLDP_EDIM
    assert L.bldp_argext_f32(A, 64, 1, 4, None, 4, 1, 7, None, None, 16, 16, None) == E.BLDP_EINVAL
    # idx / val inside the input window, idx over val, overlapping rows
    assert L.bldp_argext_f32(A, 64, 1, 4, None, 4, 1, 0, A + 4 * 255, None, 16, 16, None) == \
        E.BLDP_EINVAL and "overlap" in E.last_error()
    assert L.bldp_argext_f32(A, 64, 1, 4, None, 4, 1, 0, A + 4096, A + 64, 16, 16, None) == \
        E.BLDP_EINVAL and "overlap" in E.last_error()
    assert L.bldp_argext_f32(A, 64, 1, 4, None, 4, 1, 0, A + 4096, A + 4096 + 252, 16, 16, None) \
        == E.BLDP_EINVAL and "idx and val" in E.last_error()
    assert L.bldp_argext_f32(A, 64, 2, 4, None, 4, 1, 0, A + 4096, None, 15, 32, None) == \
        E.BLDP_EINVAL and "strides" in E.last_error()
    # an empty result launches nothing and needs no pointers
    assert L.bldp_argext_f32(None, 64, 1, 0, None, 4, 1, 0, None, None, 16, 16, None) == 0
    ptrs = (ctypes.c_void_p * 2)(None, None)
    assert L.bldp_band_argext_f32(2, ptrs, 64, 1, 0, None, 4, 1, 1, None, None, None) == 0
    assert L.bldp_band_argext_f32(0, ptrs, 64, 1, 4, None, 4, 1, 1, None, None, None) == E.BLDP_EINVAL
    assert L.bldp_band_argext_f32(2, ptrs, 64, 1, 4, None, 4, 1, 1, A, None, None) == E.BLDP_EINVAL
    assert L.bldp_argext_host_f32(0, None, 64, 1, 0, None, 4, 1, 0, None, None) == 0
    assert L.bldp_argext_host_f32(0, None, 64, 1, 4, None, 4, 1, 0, None, None) == E.BLDP_EINVAL
    assert L.bldp_argext_host_f32(0, None, 64, 1, 4, None, 5, 1, 0, None, None) == E.BLDP_EDIM
    assert L.bldp_argext_host_f32(0, None, 64, 1, 4, None, 4, 1, 2, None, None) == E.BLDP_EINVAL


# ---------------------------------------------------------------------------
# the rule, as literal loops

def isless(a, b):
    """Julia's isless on numbers: NaN above everything, -0.0 < 0.0."""
    an, bn = a != a, b != b
    if an or bn:
        return (not an) and bn
    if a == 0 and b == 0:
        return bool(np.signbit(a)) and not np.signbit(b)
    return bool(a < b)


def arg_loop(block, op):
    """block in offset order; the first NaN, else the first isless-extreme element."""
    for off, x in enumerate(block):
        if x != x:
            return off
    best = 0
    for off in range(1, len(block)):
        better = isless(block[best], block[off]) if op == "argmax" else isless(block[off], block[best])
        if better:
            best = off
    return best


def ref_loops(a, F, T, op):
    nc, ni, nt = a.shape
    out = np.empty((nc // F, ni, nt // T), np.int32)
    for co in range(nc // F):
        for i in range(ni):
            for to in range(nt // T):
                blk = [a[co * F + k, i, to * T + tt] for tt in range(T) for k in range(F)]
                out[co, i, to] = arg_loop(blk, op)
    return out


def test_isless_loop_rules():
    nan = float("nan")
    assert arg_loop([1.0, 3.0, 3.0, 2.0], "argmax") == 1 and arg_loop([1.0, 3.0, 1.0], "argmin") == 0
    assert arg_loop([0.0, -0.0], "argmax") == 0 and arg_loop([-0.0, 0.0], "argmax") == 1
    assert arg_loop([0.0, -0.0], "argmin") == 1 and arg_loop([-0.0, 0.0], "argmin") == 0
    assert arg_loop([5.0, nan, 9.0, -nan], "argmax") == 1 == arg_loop([5.0, nan, 0.0], "argmin")
    assert arg_loop([np.inf, -np.inf, np.inf], "argmax") == 0
    assert arg_loop([np.inf, -np.inf, -np.inf], "argmin") == 1


@pytest.mark.parametrize("op", ["argmax", "argmin"])
def test_host_argext_against_loops(pkg, op):
    W = pkg.worker
    rng = np.random.default_rng(5)
    cases = []
    for dt in (np.int16, np.uint8):  # ties: 4 distinct values
        cases.append(np.asfortranarray(rng.integers(0, 4, (24, 2, 12)).astype(dt) * dt(7)))
    f = np.asfortranarray(rng.integers(-2, 2, (24, 2, 12)).astype(np.float64))
    f[0:2, 0, 0] = (0.0, -0.0)   # adjacent +-0 in both orders, block maxima / minima
    f[2:4, 0, 0] = 0.0
    f[4:6, 0, 1] = (-0.0, 0.0)
    f[6:8, 0, 1] = 0.0
    f[8, 1, 0] = np.nan          # NaN first, middle and last of a block of 8 x 4
    f[19, 1, 1] = -np.nan
    f[20, 1, 2] = 5.0
    f[23, 1, 3] = np.nan
    f[3, 1, 8] = np.inf
    f[5, 1, 9] = -np.inf
    cases.append(f)
    for a in cases:
        for F, T in ((8, 4), (4, 1), (1, 3), (24, 12), (3, 2)):
            got = W._host_argext(a, F, T, op)
            assert got.dtype == np.int32 and got.flags.f_contiguous
            assert np.array_equal(got, ref_loops(a, F, T, op)), (a.dtype, F, T)
    # the values are the elements at the offsets, bit for bit
    idx, val = W._host_argext(f, 8, 4, op, values=True)
    assert val.dtype == np.float64
    for (co, i, to), off in np.ndenumerate(idx):
        x = f[co * 8 + off % 8, i, to * 4 + off // 8]
        assert x.tobytes() == val[co, i, to].tobytes()
    # a window: channel step 2 reversed, one IF, time offset with a step
    win = [23, 12, -2, 1, 1, 1, 1, 4, 3]
    sub = f[23::-2][:12, 1:2, 1::3][:, :, :4]
    assert np.array_equal(W._host_argext(f, 4, 2, op, win), ref_loops(sub, 4, 2, op))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        W._host_argext(f, 5, 1, op)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        W._host_argext(f, 1, 5, op)


def test_worker_routing_errors(pkg):
    W, G = pkg.worker, pkg.GBT
    a = np.asfortranarray(np.arange(24, dtype=np.int16).reshape((8, 1, 3)))
    assert W.fqav(a, 1, "argmax") is a  # fqav(A, n <= 1) returns A, like every other f
    assert W.fqav(a, 0, "argmin") is a
    with pytest.raises(ValueError, match="mode"):
        W.fqav(a, 2, "mode")
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata(a, fqavby=2, fqavfunc="argmax", tavby=3, tavfunc="sum")
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata("nofile.fil", fqavby=2, fqavfunc="argmin", tavfunc="median")
    with pytest.raises(TypeError, match="tavfunc"):
        G.getband([0], ["nofile.fil"], fqavby=2, fqavfunc="argmax", tavfunc="sum")
    with pytest.raises(TypeError, match="despike"):
        G.getband([0], ["nofile.fil"], fqavby=2, fqavfunc="argmax", despike_nfpc=4)
    # integer data never touch the GPU: Julia's rule on the host, through every layer
    want = ref_loops(a, 4, 3, "argmax")
    assert np.array_equal(W.getdata(a, fqavby=4, fqavfunc="argmax", tavby=3), want)
    assert np.array_equal(W.fqav(a, 4, "argmin"), ref_loops(a, 4, 1, "argmin"))
    assert np.array_equal(W.fqav(a[:, 0, 0], 4, "argmax"), [3, 3])
    vals, idx = W.findmax(a, fqavby=4, tavby=3)
    assert np.array_equal(idx, want) and np.array_equal(vals[:, 0, 0], [11, 23])
    vals, idx = W.findmin(a, fqavby=4, tavby=3)
    assert np.array_equal(idx, np.zeros((2, 1, 1))) and np.array_equal(vals[:, 0, 0], [0, 12])
    assert W.getdata(a, fqavby=4, fqavfunc="argmax", tavby=3).dtype == np.int32
    # blocks of one element: fqav's n <= 1 rule, the window itself
    assert np.array_equal(W.getdata(a, fqavby=1, fqavfunc="argmax"), a)


def test_numpy_argmax_stays_a_host_callable(pkg):
    """Only the strings select Julia's rule: np.argmax goes to the host as a
    callable, with NumPy's (NaN is only the maximum, -0.0 == 0.0)."""
    W = pkg.worker
    a = np.asfortranarray(np.float32([[0.0, -0.0, 7.0, 7.0], [1.0, np.nan, -0.0, 0.0]]).T
                          .reshape((4, 1, 2)))
    got = W.fqav(a, 2, np.argmax)
    assert np.array_equal(got, np.argmax(a.reshape((2, 2, 1, 2), order="F"), axis=0))
    assert got.dtype == np.intp
    got = W.getdata(a, fqavby=4, fqavfunc=np.argmin)
    assert np.array_equal(got[0, 0], [0, 1])  # NumPy: the first zero; NaN wins argmin too
    assert W._opname(np.argmax) is None and W._argop(np.argmax) is None
    assert W._argop("argmax") == "argmax" and W._argop("max") is None


def test_julia_shim_argext():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    assert re.search(r"argcode\(f\) = f === argmax \? Cint\(0\) : f === argmin \? Cint\(1\) : nothing",
                     src)
    assert re.search(r"export[^\n]*\n[^\n]*gpu_argext", src)
    call = re.search(r"ccall\(\(:bldp_argext_host_f32, libbldp\), Cint,\s*\(([^()]*)\)", src, re.S)
    args = " ".join(call.group(1).split())
    assert args == ("Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, "
                    "Ptr{UInt32}, Ptr{Float32}")
    assert re.search(r"function gpu_argext\(A::Array\{Float32,3\}, fqavby::Integer, "
                     r"tavby::Integer=1;\s*f=argmax, idxs::Tuple=\(:, :, :\), dev::Integer=0, "
                     r"values::Bool=false\)", src)
    assert ".+ Int32(1)" in src  # 1-based offsets
    assert re.search(r"CartesianIndex\(Int\(offs\[I\]\), I\[1\], I\[2\], I\[3\]\)", src)
    assert "bldp_argext" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "argext.hip" in open(os.path.join(REPO, "DESIGN.md")).read()
