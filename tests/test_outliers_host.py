"""CPU: the host side of outliers -- the rule's NumPy restatement on blocks
written by hand, the pure host entry points of the bldp_outliers_* family (shape,
plan with the reads of the block; every refusal, without a GPU), the Python
layer's argument and element-type checks, and the Julia shim's ccalls."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from mad_ref import MAD_CONSTANT
from outliers_ref import outlier_blocks, outliers_ref

MAD = 8
NAN = float("nan")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# ---------------------------------------------------------------------------
# the restatement

def col(*v):
    return np.asfortranarray(np.float32(v).reshape((len(v), 1, 1)))


def test_restatement_on_hand_written_blocks():
    # a constant block with one spike: s = 0 flags exactly what differs from the median
    a = col(7, 7, 7, 7, 9, 7, 7)
    med, mad, count, mask = outliers_ref(a, 7, 5.0)
    assert med.ravel() == [7] and mad.ravel() == [0] and count.ravel() == [1]
    assert mask.dtype == np.uint8 and mask.ravel().tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert count.dtype == np.uint32 and med.dtype == mad.dtype == np.float32
    # [0, 1, 2, 3, 100]: c = 2, d = 2, 1, 0, 1, 98, m = 1, s = 1.4826, thr(3) = 4.4478
    a = col(0, 1, 2, 3, 100)
    med, mad, count, mask = outliers_ref(a, 5, 3.0)
    assert med.ravel() == [2] and mad.ravel() == [np.float32(MAD_CONSTANT)]
    assert count.ravel() == [1] and mask.ravel().tolist() == [0, 0, 0, 0, 1]
    assert outliers_ref(a, 5, 1.0)[2].ravel() == [2]  # thr = 1.4826: d = 2 and 98
    assert outliers_ref(a, 5, 1e300)[2].ravel() == [0]  # thr = +Inf flags nothing
    # the strict compare: d == thr is not flagged (s = 1.4826..., nsigma = 0 is thr = 0)
    c, s, thr, d, f = outlier_blocks(col(0, 1, 2, 3, 100)[:, :, 0], 0.0)
    assert thr == 0 and f.ravel().tolist() == [1, 1, 0, 1, 1]
    # a NaN block: NaN planes, nothing flagged; so for Inf - Inf deviations
    for blk in (col(1, NAN, 3, 50), col(np.inf, np.inf, 1, np.inf), col(-np.inf, np.inf)):
        med, mad, count, mask = outliers_ref(blk, blk.shape[0], 0.0)
        assert np.isnan(mad).all() and count.ravel() == [0] and not mask.any()
    assert np.isnan(outliers_ref(col(1, NAN, 3, 50), 4, 3.0)[0]).all()
    assert outliers_ref(col(np.inf, np.inf, 1, np.inf), 4, 3.0)[0].ravel() == [np.inf]
    # s = +Inf and nsigma = 0: the product is NaN, nothing is flagged
    assert outliers_ref(col(-np.inf, 0, np.inf), 3, 0.0)[2].ravel() == [0]
    # both axes, several blocks: the mask is the window's, count its block sums
    rng = np.random.default_rng(0)
    a = np.asfortranarray(rng.standard_normal((12, 2, 8)).astype(np.float32))
    a[5, 1, 3] = 40
    for axis, n in ((0, 4), (2, 8), (2, 4)):
        win = [11, 8, -1, 0, 2, 1, 0, 8, 1]
        for w in (None, win):
            med, mad, count, mask = outliers_ref(a, n, 3.0, w, axis)
            shape = list(a.shape if w is None else (8, 2, 8))
            assert list(mask.shape) == shape
            shape[axis] //= n
            assert list(med.shape) == list(mad.shape) == list(count.shape) == shape
            assert mask.sum() == count.sum() and mask.max() == 1
        assert mask[11 - 5, 1, 3] == 1


# ---------------------------------------------------------------------------
# the host-only C calls

def wptr(win):
    return ctypes.cast((ctypes.c_int64 * 9)(*win), ctypes.c_void_p) if win else None


def oshape(L, dims, axis, n, win=None):
    d, m = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    rc = L.bldp_outliers_shape(*dims, wptr(win), axis, n, d, m)
    return rc, list(d), list(m)


def oplan(L, dims, axis, n, mask, win=None):
    info = (ctypes.c_int64 * 10)()
    rc = L.bldp_outliers_plan_f32(None, *dims, wptr(win), axis, n, mask, info)
    return rc, list(info)


def test_header_and_abi_version(pkg, L):
    hdr = open(os.path.join(REPO, "include", "bldp.h")).read()
    assert re.search(r"#define BLDP_ABI_VERSION 5\b", hdr) and L.bldp_abi_version() == 5
    assert "the bldp_outliers_* entry points" in hdr
    for name in ("bldp_outliers_shape", "bldp_outliers_plan_f32", "bldp_outliers_f32",
                 "bldp_band_outliers_f32", "bldp_outliers_host_f32"):
        assert re.search(r"BLDP_API int %s\(" % name, hdr), name
        assert name in pkg._lib.SIGNATURES
    assert "1.4826022185056018" in hdr and "d_i > thr" in hdr


def test_shape(pkg, L):
    E = pkg._lib
    assert oshape(L, (64, 2, 12), 0, 8) == (E.BLDP_OK, [8, 2, 12], [64, 2, 12])
    assert oshape(L, (64, 2, 12), 2, 4) == (E.BLDP_OK, [64, 2, 3], [64, 2, 12])
    assert oshape(L, (64, 2, 12), 0, 8, [4, 32, 1, 1, 1, 1, 11, 6, -2]) == \
        (E.BLDP_OK, [4, 1, 6], [32, 1, 6])
    assert oshape(L, (64, 2, 12), 2, 3, [4, 32, 1, 1, 1, 1, 11, 6, -2]) == \
        (E.BLDP_OK, [32, 1, 2], [32, 1, 6])
    assert oshape(L, (64, 2, 12), 0, 5)[0] == E.BLDP_EDIM
    assert oshape(L, (64, 2, 12), 2, 5)[0] == E.BLDP_EDIM
    assert oshape(L, (64, 2, 12), 0, 8, [60, 8, 1, 0, 2, 1, 0, 12, 1])[0] == E.BLDP_EBOUNDS
    assert oshape(L, (64, 2, 12), 1, 4)[0] == E.BLDP_EINVAL and "axis" in E.last_error()
    for n in (1, 0, -4):
        assert oshape(L, (64, 2, 12), 0, n)[0] == E.BLDP_EINVAL and "n=" in E.last_error()
    d = (ctypes.c_int64 * 3)()
    assert L.bldp_outliers_shape(64, 2, 12, None, 0, 8, d, None) == E.BLDP_EINVAL
    assert L.bldp_outliers_shape(64, 2, 12, None, 0, 8, None, d) == E.BLDP_EINVAL


def test_plans_are_mads_with_the_reads(pkg, L):
    E, P, TP = pkg._lib, pkg._lib.PATHS, pkg._lib.TSTAT_PATHS
    mad = (ctypes.c_int64 * 8)()
    for F, path, reads in ((2, "median_sort", (1, 2)), (5, "median_sort", (1, 2)),
                           (64, "median_sort", (1, 2)), (65, "median_select", (1, 2)),
                           (4096, "median_select", (1, 2)), (4097, "median_stream", (9, 9)),
                           (8192, "median_stream", (9, 9))):
        dims = (2 * F, 2, 3)
        for win in (None, [0, F, 2, 0, 2, 1, 0, 3, 1]):
            assert L.bldp_reduce_plan_f32(None, *dims, wptr(win), F, 1, MAD, None, mad) == E.BLDP_OK
            for m in (0, 1):
                rc, q = oplan(L, dims, 0, F, m, win)
                assert rc == E.BLDP_OK, E.last_error()
                assert P[q[0]] == path and q[:8] == list(mad), (F, m)
                assert q[8:] == [reads[m], m], (F, m, q)
    for T in (2, 3, 16, 31, 32, 33, 34, 100, 1024):
        for nc in (264, 8, 6):
            dims = (nc, 2, 2 * T)
            assert L.bldp_tstat_plan_f32(None, *dims, None, T, MAD, None, mad) == E.BLDP_OK
            for m in (0, 1):
                rc, q = oplan(L, dims, 2, T, m)
                assert rc == E.BLDP_OK, E.last_error()
                assert q[:8] == list(mad), (T, nc, m)
                if T <= 32:
                    assert TP[q[0]] == "regs_median" and q[8:] == [1 + m, m], (T, nc, q)
                else:  # mad's 8 (odd n) or 10 (even n) reads, and the flag pass
                    assert TP[q[0]] == "split_median" and q[3] == (8 if T % 2 else 10)
                    assert q[8:] == [q[3] + 1, m], (T, nc, q)
    assert oplan(L, (64, 2, 12), 0, 8, 7)[1][9] == 1  # any non-zero want_mask


def test_every_refusal_without_a_gpu(pkg, L):
    E = pkg._lib
    info = (ctypes.c_int64 * 10)()
    ptrs = (ctypes.c_void_p * 2)(0, 0)
    banks = ctypes.cast(ptrs, ctypes.c_void_p)

    def entries(axis, n, nsigma, win=None):
        """Every entry point that takes nsigma, on null data."""
        return [L.bldp_outliers_f32(None, 64, 2, 12, win, axis, n, nsigma, None, None, None, None,
                                    64, 128, None),
                L.bldp_band_outliers_f32(2, banks, 64, 2, 12, win, axis, n, nsigma, None, None,
                                         None, None, None),
                L.bldp_outliers_host_f32(0, None, 64, 2, 12, win, axis, n, nsigma, None, None,
                                         None, None)]

    for axis in (0, 2):
        for bad in (-1.0, -1e-300, NAN, float("inf"), -float("inf")):
            for rc in entries(axis, 4, bad):
                assert rc == E.BLDP_EINVAL and "nsigma" in E.last_error(), (axis, bad)
        for n in (1, 0, -2):
            for rc in entries(axis, n, 5.0) + [
                    L.bldp_outliers_plan_f32(None, 64, 2, 12, None, axis, n, 0, info)]:
                assert rc == E.BLDP_EINVAL and "n=" in E.last_error(), (axis, n)
    for axis in (1, 3, -1):
        for rc in entries(axis, 4, 5.0) + [
                L.bldp_outliers_plan_f32(None, 64, 2, 12, None, axis, 4, 0, info)]:
            assert rc == E.BLDP_EINVAL and "axis" in E.last_error(), axis
    # good (axis, n, nsigma) pass those checks: the divisibility and window checks come next
    w = wptr([60, 8, 1, 0, 2, 1, 0, 12, 1])  # a window out of bounds
    for axis in (0, 2):
        for rc in entries(axis, 5, 5.0) + [
                L.bldp_outliers_plan_f32(None, 64, 2, 12, None, axis, 5, 0, info)]:
            assert rc == E.BLDP_EDIM, axis
        for rc in entries(axis, 4, 5.0, w) + [
                L.bldp_outliers_plan_f32(None, 64, 2, 12, w, axis, 4, 1, info)]:
            assert rc == E.BLDP_EBOUNDS, axis
    # ... then the null pointers (the plan takes them)
    for axis in (0, 2):
        assert L.bldp_outliers_plan_f32(None, 64, 2, 12, None, axis, 4, 1, info) == E.BLDP_OK
        for rc in entries(axis, 4, 5.0):
            assert rc == E.BLDP_EINVAL and "null" in E.last_error(), axis
    assert L.bldp_outliers_plan_f32(None, 64, 2, 12, None, 0, 4, 1, None) == E.BLDP_EINVAL
    assert L.bldp_band_outliers_f32(0, banks, 64, 2, 12, None, 2, 4, 5.0, None, None, None, None,
                                    None) == E.BLDP_EINVAL
    # four null outputs of a non-empty result, and overlapping outputs (the
    # addresses are never dereferenced: every check comes before any launch)
    x = 1 << 20  # the input: 64 * 2 * 12 floats = 6144 bytes
    far = x + (1 << 16)
    for axis in (0, 2):
        assert L.bldp_outliers_f32(x, 64, 2, 12, None, axis, 4, 5.0, None, None, None, None, 64,
                                   128, None) == E.BLDP_EINVAL
        assert "every output is null" in E.last_error()
        for outs, what in (((far, far, None, None), "med and mad"),
                           ((far, None, far + 8, None), "med and count"),
                           ((None, far, None, far + 100), "mad and mask"),
                           ((None, None, far + 1535, far), "count and mask"),
                           ((x + 6140, None, None, None), "med overlaps the input"),
                           ((None, None, None, x - 1535), "mask overlaps the input")):
            ld = (16, 32) if axis == 0 else (64, 128)
            assert L.bldp_outliers_f32(x, 64, 2, 12, None, axis, 4, 5.0, *outs, *ld, None) == \
                E.BLDP_EINVAL, (axis, what)
            assert "overlap" in E.last_error() and what in E.last_error(), E.last_error()
        # strides that fold the planes onto themselves
        assert L.bldp_outliers_f32(x, 64, 2, 12, None, axis, 4, 5.0, far, None, None, None, 8, 16,
                                   None) == E.BLDP_EINVAL and "strides" in E.last_error()
    bx = ctypes.cast((ctypes.c_void_p * 2)(x, x + 8192), ctypes.c_void_p)
    assert L.bldp_band_outliers_f32(2, bx, 64, 2, 12, None, 0, 4, 5.0, None, None, None, None,
                                    None) == E.BLDP_EINVAL and "null" in E.last_error()
    assert L.bldp_band_outliers_f32(2, bx, 64, 2, 12, None, 0, 4, 5.0, far, None, None,
                                    x + 8192 + 6000, None) == E.BLDP_EINVAL
    assert "mask overlaps the input (bank 1)" in E.last_error()
    # an empty window is nothing to do, whatever the pointers
    empty = wptr([0, 0, 1, 0, 2, 1, 0, 12, 1])
    assert L.bldp_outliers_f32(None, 64, 2, 12, empty, 2, 4, 5.0, None, None, None, None, 0, 0,
                               None) == E.BLDP_OK
    assert L.bldp_abi_version() == 5


# ---------------------------------------------------------------------------
# the Python layer

def test_python_checks_before_any_gpu_work(pkg):
    W, eng = pkg.worker, pkg.engine
    assert pkg.getoutliers is W.getoutliers and "getoutliers" in pkg.__all__
    assert callable(pkg.GBT.getoutliers)
    a = np.zeros((8, 1, 4), dtype=np.float32, order="F")
    for dt in (np.int16, np.uint8, np.float64):
        for kw in (dict(n=2, axis=0), dict(), dict(n=2, mask=True)):
            with pytest.raises(TypeError, match="getoutliers: element type %s is not supported; "
                               "outliers takes Float32" % np.dtype(dt).name):
                W.getoutliers(a.astype(dt), **kw)
        with pytest.raises(TypeError, match="outliers takes Float32"):
            eng.outliers_host(a.astype(dt), 2)
    for bad in (-1.0, NAN, float("inf"), "x", None):
        with pytest.raises(ValueError, match="nsigma"):
            W.getoutliers(a, nsigma=bad)
        with pytest.raises(ValueError, match="nsigma"):
            eng.outliers_host(a, 2, nsigma=bad)
    for axis in (1, 3, "t"):
        with pytest.raises(ValueError, match="axis"):
            W.getoutliers("nothing.fil", axis=axis)  # before any file is touched
    with pytest.raises(ValueError, match="which"):
        eng.outliers_host(a, 2, which=("median", "sigma"))
    with pytest.raises(ValueError, match="no output"):
        eng.outliers_host(a, 2, which=())
    # n=None is the whole selected time range, on axis 2 alone
    assert eng._outliers_n(None, 2, 8, 12) == 12 and eng._outliers_n(4, 0, 8, 12) == 4
    with pytest.raises(ValueError, match="axis 2"):
        eng._outliers_n(None, 0, 8, 12)
    for n in (1, 0):
        with pytest.raises(pkg._lib.ArgumentError, match="n="):
            eng.outliers_host(a, n)
    with pytest.raises(pkg._lib.ArgumentError, match="n="):
        W.getoutliers(np.zeros((8, 1, 1), np.float32, order="F"))  # n=None of one spectrum
    with pytest.raises(pkg._lib.DimensionMismatch):
        eng.outliers_host(a, 3, axis=2)
    with pytest.raises(pkg._lib.BoundsError):
        eng.outliers_host(a, 2, win=[6, 4, 1, 0, 1, 1, 0, 4, 1])
    assert eng.OUTLIER_PLANES == ("median", "mad", "count")


def test_eight_bit_sigproc_file_is_a_type_error(pkg, tmp_path):
    a = np.asfortranarray(np.arange(8 * 12, dtype=np.uint8).reshape((8, 1, 12), order="F"))
    fil = str(tmp_path / "u8.fil")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=8, nifs=1, tsamp=1.0, nbits=8,
                                    telescope_id=6, machine_id=10, data_type=1, tstart=59000.0,
                                    source_name="X"), a)
    with pytest.raises(TypeError, match="getoutliers: element type uint8"):
        pkg.WorkerFunctions.getoutliers(fil, n=4)


def test_julia_shim_and_docs():
    src = open(os.path.join(REPO, "bldistributeddataproducts.jl_amd", "julia", "BLDPHip.jl")).read()
    for name in ("bldp_outliers_shape", "bldp_outliers_plan_f32", "bldp_outliers_f32",
                 "bldp_band_outliers_f32", "bldp_outliers_host_f32"):
        assert re.search(r"ccall\(\(:%s, libbldp\)" % name, src), name
    for fn in ("gpu_outliers", "gpu_outliers_plan", "gpu_band_outliers"):
        assert re.search(r"^function %s\(" % fn, src, re.M) and re.search(r"\b%s\b" % fn,
                                                                          src.split("const libbldp")[0])
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert re.search(r"\bgetoutliers\b", open(os.path.join(REPO, doc)).read()), doc
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert re.search(r"^#+ .*[Oo]utliers", design, re.M)
    assert os.path.exists(os.path.join(REPO, "profiles", "outliers", "outliers_probe.json"))
