"""GPU parity of getmoments (mean, var, skewness, kurtosis from one read) against
the statement of tests/moments_ref.py, in the class of the path the plan
reports (engine.moments_plan), and against the calls it fuses:
  mean      the bits of oracle.mean_f32 widened, on every path
  var       NumPy's cm2 / n: the same bits on regs, nt 2^-53 relative on mid and
            two-pass, 3 2^-24 1.05 relative on leaf
  skewness  the bits of engine.skewness on the same tensor under the same plan
            options, and inside assert_skewness
  kurtosis  the bits of engine.kurtosis (with kurt_leaf_tile = 0, as moments
            plans), and inside assert_kurtosis
NaN and +-Inf positions equal the statement's on every path.  A plane that is
not asked for is not written; every subset gives the bits of the full call.

Data and shapes are tests/test_gpu_skewness.py's: integrated-power rows, and
the smallest windows at which each path can go wrong.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits
from moments_ref import (PLANES, assert_moments, block_win, moments_statement,
                         moments_statement_blocks)
from test_gpu_skewness import BLOCKS, NC, NI, NT, SHAPES, nonfinite_rows, power_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def dev(eng, a):
    return eng.fb_from_numpy(np.asfortranarray(a), device="cuda:0")


def host(eng, t):
    return None if t is None else eng.fb_to_numpy(t)


def planes(eng, m) -> dict:
    """A Moments of tensors or arrays as {name: host array or None}."""
    return {k: (v if v is None or isinstance(v, np.ndarray) else host(eng, v))
            for k, v in m._asdict().items()}


@pytest.fixture(scope="module")
def rows():
    """One array shared by the cases below (read-only): each takes a window."""
    a = power_rows(np.random.default_rng(20262), NC, NI, NT)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def xrows(eng, rows):
    return dev(eng, rows.copy(order="F"))  # (torch wants a writable source)


def fused_calls(pkg, eng, x, win, tblock=None):
    """(skewness, kurtosis) of the separate calls under the plan options in
    force; the kurtosis with kurt_leaf_tile = 0, the plan moments takes."""
    s = host(eng, eng.skewness(x, win, tblock=tblock))
    with pkg._lib.plan_option("kurt_leaf_tile", 0):
        k = host(eng, eng.kurtosis(x, win, tblock=tblock))
    return s, k


def check_window(pkg, eng, orc, rows, xrows, win, path, finite=True, msg=""):
    """engine.moments of a window against the statement and the fused calls."""
    plan = eng.moments_plan(xrows, win)
    assert plan["path"] == path and plan["blocks"] == 1, (msg, plan)
    splan = eng.skewness_plan(xrows, win)
    assert (plan["path"], plan["fused"]) == (splan["path"], splan["fused"])
    want = moments_statement(orc, rows, win)
    if finite and win[7] >= 16:  # (two equal values of the ulp row are 0 / 0)
        assert all(np.isfinite(want[k]).all() for k in PLANES), msg
    m = eng.moments(xrows, win)
    for t in m:
        assert tuple(t.shape) == (win[1], win[4]) and str(t.dtype) == "torch.float64"
    got = planes(eng, m)
    assert_moments(got, want, path, win[7], (msg, win))
    s, k = fused_calls(pkg, eng, xrows, win)
    assert same_bits(got["skewness"], s), (msg, win, "skewness bits")
    assert same_bits(got["kurtosis"], k), (msg, win, "kurtosis bits")
    return got


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("nt", [1, 2, 3, 16, 31, 32])
def test_regs_bit_for_bit(pkg, eng, orc, rows, xrows, nt, exact):
    """k_kurt_regs<., ., all>: the recipe in its own order (kurt_exact at both
    values; 32 spectra take the counted form either way); a single spectrum is
    0 / 0 in the two ratios, its own value as the mean and 0 as the variance."""
    with pkg._lib.plan_option("kurt_exact", exact):
        for nc, ni in SHAPES:
            got = check_window(pkg, eng, orc, rows, xrows, [0, nc, 1, 0, ni, 1, 0, nt, 1], "regs")
            if nt == 1:
                assert np.isnan(got["skewness"]).all() and np.isnan(got["kurtosis"]).all()
                assert (got["var"] == 0.0).all()
                assert same_bits(got["mean"], rows[:nc, :ni, 0].astype(np.float64))
        # channel 1: float4 columns on a dword boundary; a reversed time range
        w1 = [1, 256, 1, 0, 2, 1, 0, nt, 1]
        check_window(pkg, eng, orc, rows, xrows, w1, eng.kurtosis_plan(xrows, w1)["path"])
        check_window(pkg, eng, orc, rows, xrows, [0, 256, 1, 0, 2, 1, 40 + nt - 1, nt, -1], "regs")


@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("nt", [33, 64, 65, 384, 385, 512])
def test_mid(pkg, eng, orc, rows, xrows, nt, small):
    """k_kurt_mid2 (<= 384 spectra of float4 columns; kurt_mid_small at both
    values) and k_kurt_mid: the recipe's terms, partial sums in wave order."""
    with pkg._lib.plan_option("kurt_mid_small", small):
        for nc, ni in SHAPES:
            check_window(pkg, eng, orc, rows, xrows, [0, nc, 1, 0, ni, 1, 3, nt, 1], "mid")
        # no float4 columns: 6 channels, and a channel step of 2
        check_window(pkg, eng, orc, rows, xrows, [0, 6, 1, 0, 2, 1, 0, nt, 1], "mid")
        check_window(pkg, eng, orc, rows, xrows, [0, 130, 2, 0, 2, 1, 0, nt, 1], "mid")


@pytest.mark.parametrize("narrow", [0, 4])
@pytest.mark.parametrize("nt", [513, 1024, 1025, 2049, 4097])
def test_leaf(pkg, eng, orc, rows, xrows, nt, narrow):
    """k_kurt_leaf + the tree + k_kurt_final_*<., all> (kurt_leaf_narrow at both
    values): all four planes from the same merged moments.  With narrow = 4
    these windows are the ones engine.kurtosis gives to k_kurt_tile."""
    with pkg._lib.plan_option("kurt_leaf_narrow", narrow):
        for nc, ni in SHAPES:
            check_window(pkg, eng, orc, rows, xrows, [0, nc, 1, 0, ni, 1, 0, nt, 1], "leaf")


def test_leaf_with_a_tree_pass(pkg, eng, orc):
    """More than 131072 spectra: 128 blocks, so a k_kurt_tree pass runs before
    the final level."""
    nt = 140001
    a = power_rows(np.random.default_rng(3), 8, 1, nt)
    x = dev(eng, a)
    assert eng.kurtosis_plan(x)["K"] == 7
    check_window(pkg, eng, orc, a, x, [0, 8, 1, 0, 1, 1, 0, nt, 1], "leaf")


@pytest.mark.parametrize("nt", [600, 3000])
def test_twopass(pkg, eng, orc, rows, xrows, nt):
    """No float4 columns and more than 512 spectra: Julia's mean through the
    tree, then k_kurt_pass<all> with three partial sums per chunk (and
    k_kurt_fold<all> over its time chunks)."""
    check_window(pkg, eng, orc, rows, xrows, [0, 6, 1, 0, 2, 1, 0, nt, 1], "twopass")
    check_window(pkg, eng, orc, rows, xrows, [0, 6, 1, 1, 1, 1, 7, nt, 1], "twopass")


def test_integrated_power_rows_have_var_over_mean_squared_one_over_n(eng, rows, xrows):
    """What the mean and var planes are for: integrated power of N averaged
    chi^2(2) spectra has var / mean^2 = 1 / N = 1 / R^2 (within sampling noise
    over 4096 spectra: the relative error of a sample variance is about
    sqrt((kurtosis + 2) / n), taken at 6 sigma with kurtosis 6 / R^2 <= 3)."""
    m = planes(eng, eng.moments(xrows, [0, 5, 1, 0, 1, 1, 0, 4096, 1], which=("mean", "var")))
    assert m["skewness"] is None and m["kurtosis"] is None
    R = np.array([np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0])
    ratio = m["var"][:, 0] / m["mean"][:, 0] ** 2 * R ** 2
    assert np.abs(ratio - 1.0).max() < 6.0 * np.sqrt(5.0 / 4096)


@pytest.mark.parametrize("nt,path", [(16, "regs"), (100, "mid"), (1025, "leaf")])
def test_nonfinite_positions_and_signs(pkg, eng, orc, nt, path):
    """skewness_ref's overflow, underflow and non-finite rows: NaN and +-Inf
    positions (and signs) of all four planes are the statements'."""
    a, exp = nonfinite_rows(np.random.default_rng(50 + nt), nt)
    x = dev(eng, a)
    assert eng.moments_plan(x)["path"] == path
    want = moments_statement(orc, a)
    assert np.isinf(want["var"][1, 0]) and want["var"][5, 0] > 0  # z^2 overflows; squares survive
    assert np.isinf(want["kurtosis"][2:5, 0]).sum() + np.isnan(want["kurtosis"][2:5, 0]).sum() == 3
    got = planes(eng, eng.moments(x))
    ordinary = [0, 9, 10, 11]
    assert_moments({k: v[ordinary] for k, v in got.items()},
                   {k: v[ordinary] for k, v in want.items()}, path, nt, "ordinary rows")
    from skewness_ref import assert_positions

    for name in PLANES:
        assert_positions(got[name], want[name], (nt, path, name))
    assert same_bits(got["mean"], want["mean"])
    s, k = fused_calls(pkg, eng, x, None)
    assert same_bits(got["skewness"], s) and same_bits(got["kurtosis"], k)


def check_blocks(got, want, path, M, msg=""):
    for b in range(want["mean"].shape[2]):
        assert_moments({k: (None if v is None else v[:, :, b]) for k, v in got.items()},
                       {k: v[:, :, b] for k, v in want.items()}, path, M, (msg, "block", b))


@pytest.mark.parametrize("M,nb", BLOCKS, ids=[f"M{m}x{n}" for m, n in BLOCKS])
def test_block_forms(pkg, eng, orc, rows, xrows, M, nb):
    """tblock: registers (M <= 32, one launch), one streamed leaf (33..1024, one
    launch, no workspace), block by block above one leaf and without float4
    columns; every form the bits of the fused calls."""
    for nc, ni in SHAPES[1:] + [(6, 2)]:
        win = [0, nc, 1, 0, ni, 1, 5, M * nb, 1]
        plan = eng.moments_plan(xrows, win, tblock=M)
        splan = eng.skewness_plan(xrows, win, tblock=M)
        assert {k: plan[k] for k in ("path", "fused", "blocks")} == \
            {k: splan[k] for k in ("path", "fused", "blocks")}
        assert plan["blocks"] == nb
        if nc == 6 or M > 1024:
            assert plan["fused"] == 0, plan
        else:
            assert plan["fused"] == 1 and plan["workspace_bytes"] == 0, plan
            assert plan["path"] == ("regs" if M <= 32 else "leaf")
        want = moments_statement_blocks(orc, rows, win, M)
        m = eng.moments(xrows, win, tblock=M)
        assert all(tuple(t.shape) == (nc, ni, nb) for t in m)
        got = planes(eng, m)
        check_blocks(got, want, plan["path"], M, plan)
        s, k = fused_calls(pkg, eng, xrows, win, tblock=M)
        assert same_bits(got["skewness"], s) and same_bits(got["kurtosis"], k), (M, nc)
        if plan["fused"] and M <= 32:
            one = planes(eng, eng.moments(xrows, block_win(rows.shape, win, M, nb - 1)))
            for name in PLANES:
                assert same_bits(got[name][:, :, nb - 1], one[name]), (M, name)


@pytest.mark.parametrize("narrow", [0, 4])
def test_streamed_blocks_at_both_widths(pkg, eng, orc, rows, xrows, narrow):
    """k_kurtb_stream<4, 4, all> and <1, 16, all> (kurt_leaf_narrow)."""
    with pkg._lib.plan_option("kurt_leaf_narrow", narrow):
        win = [0, 256, 1, 0, 2, 1, 0, 3 * 100, 1]
        got = planes(eng, eng.moments(xrows, win, tblock=100))
        check_blocks(got, moments_statement_blocks(orc, rows, win, 100), "leaf", 100, narrow)
        s, k = fused_calls(pkg, eng, xrows, win, tblock=100)
        assert same_bits(got["skewness"], s) and same_bits(got["kurtosis"], k)


@pytest.mark.parametrize("M", [16, 64, 1030])
def test_nonfinite_values_stay_in_their_block(eng, orc, M):
    nb, nc = 4, 256
    rng = np.random.default_rng(900 + M)
    a = power_rows(rng, nc, 1, M * nb)
    blk = lambda b: slice(b * M, (b + 1) * M)  # noqa: E731
    a[3, 0, blk(1)] = np.float32(2.0 ** 19)  # constant in block 1 only: 0 / 0, var 0
    a[10, 0, 5] = np.nan
    a[20, 0, (nb - 1) * M + M // 2] = np.inf
    a[30, 0, blk(2)] = (1e30 * (1.0 + 0.1 * rng.standard_normal(M))).astype(np.float32)
    a[40, 0, M + 3] = 3e13  # only its cube and fourth power overflow, in block 1
    x = dev(eng, a)
    plan = eng.moments_plan(x, tblock=M)
    assert plan["fused"] == (1 if M <= 1024 else 0)
    want = moments_statement_blocks(orc, a, None, M)
    bad = np.zeros(want["var"].shape, bool)
    bad[10, 0, 0] = bad[20, 0, nb - 1] = bad[30, 0, 2] = True
    assert np.array_equal(~np.isfinite(want["var"]), bad) and want["var"][3, 0, 1] == 0.0
    bad[3, 0, 1] = bad[40, 0, 1] = True
    for name in ("skewness", "kurtosis"):
        assert np.array_equal(~np.isfinite(want[name]), bad), name
    got = planes(eng, eng.moments(x, tblock=M))
    check_blocks(got, want, plan["path"], M, M)


SUBSETS = [(p,) for p in PLANES] + [("skewness", "kurtosis")]


@pytest.mark.parametrize("M,win,path", [(None, [0, 256, 1, 0, 2, 1, 0, 16, 1], "regs"),
                                        (None, [0, 256, 1, 0, 2, 1, 0, 32, 1], "regs"),
                                        (None, [0, 256, 1, 0, 2, 1, 0, 200, 1], "mid"),
                                        (None, [0, 6, 1, 0, 2, 1, 0, 400, 1], "mid"),
                                        (None, [0, 256, 1, 0, 2, 1, 0, 1030, 1], "leaf"),
                                        (None, [0, 6, 1, 0, 2, 1, 0, 1030, 1], "twopass"),
                                        (16, [0, 256, 1, 0, 2, 1, 0, 48, 1], "regs"),
                                        (64, [0, 256, 1, 0, 2, 1, 0, 192, 1], "leaf"),
                                        (16, [0, 6, 1, 0, 2, 1, 0, 48, 1], "mid")],
                         ids=["regs16", "regs32", "mid2", "mid", "leaf", "twopass", "M16", "M64",
                              "M16-block-by-block"])
def test_every_subset_gives_the_bits_of_the_full_call(eng, xrows, M, win, path):
    assert eng.moments_plan(xrows, win, tblock=M)["path"] == path
    full = planes(eng, eng.moments(xrows, win, tblock=M))
    for sub in SUBSETS:
        got = planes(eng, eng.moments(xrows, win, tblock=M, which=sub))
        for name in PLANES:
            if name in sub:
                assert same_bits(got[name], full[name]), (sub, name)
            else:
                assert got[name] is None, (sub, name)


@pytest.mark.parametrize("M,win", [(0, None), (16, None), (64, None),
                                   (16, [0, 128, 2, 0, 2, 1, 0, 48, 1]),
                                   (0, [0, 128, 2, 0, 2, 1, 0, 48, 1]),
                                   (0, [0, 256, 1, 0, 2, 1, 0, 1030, 1])],
                         ids=["whole", "regs", "stream", "block-by-block", "whole-step", "leaf"])
@pytest.mark.parametrize("sub", [PLANES, ("var", "kurtosis"), ("skewness",)],
                         ids=["all", "var+kurt", "skew"])
def test_null_planes_and_strided_planes_through_the_abi(pkg, eng, M, win, sub):
    """bldp_moments_f32 itself: out_ld_i / out_ld_b larger than dense and some
    planes NULL.  The requested planes hold the values of the dense call, their
    padding and guards and the whole buffers of the planes not asked for keep
    the sentinel; overlapping strides are refused."""
    import torch

    nc, ni = 256, 2
    nt = 1030 if win is not None and win[7] == 1030 else 48 if M == 0 else 3 * M
    a = power_rows(np.random.default_rng(77 + M), nc, ni, nt)
    x = dev(eng, a)
    dense = planes(eng, eng.moments(x, win, tblock=M or None))
    if M == 0:
        dense = {k: v[:, :, None] for k, v in dense.items()}
    nco, nb = dense["mean"].shape[0], dense["mean"].shape[2]
    ld_i = nco + 3
    ld_b = ld_i * ni + 5
    guard = 16
    bufs = [torch.full((guard + nb * ld_b + guard,), -7.0, dtype=torch.float64, device="cuda:0")
            for _ in PLANES]
    ptrs = [b.data_ptr() + 8 * guard if name in sub else None for b, name in zip(bufs, PLANES)]
    L = pkg._lib.lib()
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    keep, wp = pkg._lib.win_arg(win)
    rc = L.bldp_moments_f32(ptr, nchan, nif, ntime, wp, M, *ptrs, ld_i, ld_b,
                            pkg._lib.stream_ptr())
    pkg._lib.check(rc, "bldp_moments_f32")
    for buf, name in zip(bufs, PLANES):
        o = buf.cpu().numpy()
        if name not in sub:
            assert (o == -7.0).all(), name
            continue
        used = np.zeros(o.shape, bool)
        for b in range(nb):
            for i in range(ni):
                s = slice(guard + b * ld_b + i * ld_i, guard + b * ld_b + i * ld_i + nco)
                assert same_bits(o[s], dense[name][:, i, b]), (name, b, i)
                used[s] = True
        assert (o[~used] == -7.0).all(), name
    rc = L.bldp_moments_f32(ptr, nchan, nif, ntime, wp, M, *ptrs, nco - 1, ld_b,
                            pkg._lib.stream_ptr())
    assert rc == pkg._lib.BLDP_EINVAL


@pytest.mark.parametrize("M,nt,win", [(None, 16, None), (None, 100, None), (None, 1030, None),
                                      (None, 600, [0, 6, 1, 0, 1, 1, 0, 600, 1]),
                                      (16, 64, None), (256, 768, None),
                                      (16, 64, [0, 256, 2, 0, 1, 1, 0, 64, 1]),
                                      (None, 100, [0, 256, 2, 0, 1, 1, 0, 100, 1])],
                         ids=["regs", "mid", "leaf", "twopass", "M16", "M256", "M16-channel-step",
                              "mid-channel-step"])
def test_band(eng, orc, M, nt, win):
    """Three banks in one set of launches: each bank's planes are the bits of
    its own single call, and in the class of the path."""
    rng = np.random.default_rng(31 * nt)
    arrs = [power_rows(rng, 512, 1, nt) for _ in range(3)]
    xs = [dev(eng, a) for a in arrs]
    ms = eng.band_moments(xs, win, tblock=M)
    assert len(ms) == 3
    plan = eng.moments_plan(xs[0], win, tblock=M)
    nc = 512 if win is None else win[1]
    for k, (a, x) in enumerate(zip(arrs, xs)):
        assert all(tuple(t.shape) == ((nc, 1) if M is None else (nc, 1, nt // M)) for t in ms[k])
        got = planes(eng, ms[k])
        one = planes(eng, eng.moments(x, win, tblock=M))
        for name in PLANES:
            assert same_bits(got[name], one[name]), (k, name)
        if M is None:
            assert_moments(got, moments_statement(orc, a, win), plan["path"], nt, k)
        else:
            check_blocks(got, moments_statement_blocks(orc, a, win, M), plan["path"], M, k)
    two = eng.band_moments(xs, win, tblock=M, which=("mean", "kurtosis"))
    for k in range(3):
        assert two[k].var is None and two[k].skewness is None
        assert same_bits(host(eng, two[k].kurtosis), host(eng, ms[k].kurtosis))
        assert same_bits(host(eng, two[k].mean), host(eng, ms[k].mean))
    if win is not None and win[2] == 2:
        # channel step 2: no float4 columns, so with tblock the block-by-block
        # form scatters into the per-plane band buffers; two planes are null
        vk = eng.band_moments(xs, win, tblock=M, which=("var", "kurtosis"))
        for k in range(3):
            assert vk[k].mean is None and vk[k].skewness is None
            assert same_bits(host(eng, vk[k].var), host(eng, ms[k].var))
            assert same_bits(host(eng, vk[k].kurtosis), host(eng, ms[k].kurtosis))


def test_whole_window_on_a_stream_without_scratch(eng):
    """The library's scratch is per stream and the regs path needs none: on a
    stream that has not leased any, a whole-window call still takes the one
    lease of its workspace (empty here) and gives the default stream's bits."""
    import torch

    x = dev(eng, power_rows(np.random.default_rng(8), 256, 2, 16))
    assert eng.moments_plan(x)["workspace_bytes"] == 0
    want, sk = planes(eng, eng.moments(x)), host(eng, eng.skewness(x))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    got, gs = eng.moments(x, stream=s), eng.skewness(x, stream=s)
    s.synchronize()
    got = planes(eng, got)
    for name in PLANES:
        assert same_bits(got[name], want[name]), name
    assert same_bits(host(eng, gs), sk)


def test_layers(pkg, eng, orc, tmp_path):
    """worker.getmoments on every source it handles (tensor, host array, raw
    SIGPROC file, raw and compressed FBH5 files) equals the tensor call, GBT's
    fan-out over two files equals the per-file calls, engine.moments_host
    equals the device call; with and without tblock, `which`, and a window."""
    W, C, J = pkg.WorkerFunctions, pkg.COLON, pkg.JRange
    nc, nt = 64, 128
    a = power_rows(np.random.default_rng(4), nc, 1, nt)
    x = dev(eng, a)
    fil, h5, raw5 = (str(tmp_path / n) for n in ("s.fil", "s.rawspec.0002.h5", "r.rawspec.0002.h5"))
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=nc, nifs=1, tsamp=1.0,
                                    nbits=32, telescope_id=6, machine_id=10, data_type=1,
                                    tstart=59000.0, source_name="X"), a)
    pkg.fbh5.write_bslz4(h5, dict(foff=-1.0, nfpc=64), a, (16, 1, nc),
                         lambda blk: orc.np_bslz4_encode(blk, 512, lz4=orc.lz4_compress))
    pkg.fbh5.write(raw5, dict(foff=-1.0, nfpc=64), a)
    assert pkg.fbh5.raw_layout(raw5) is not None and pkg.fbh5.needs_bslz4(h5)
    sources = (("tensor", x), ("host", a), ("fil", fil), ("raw fbh5", raw5), ("bslz4", h5))
    for M in (None, 16, 64):
        plan = eng.moments_plan(x, tblock=M)
        ref = planes(eng, eng.moments(x, tblock=M))
        want = moments_statement(orc, a) if M is None else moments_statement_blocks(orc, a, None, M)
        if M is None:
            assert_moments(ref, want, plan["path"], nt, "tensor call")
        else:
            check_blocks(ref, want, plan["path"], M, "tensor call")
        for name, src in sources:
            got = planes(eng, W.getmoments(src, tblock=M))
            for p in PLANES:
                assert same_bits(got[p], ref[p]), (name, M, p)
        hm = planes(eng, eng.moments_host(a, tblock=M))
        for p in PLANES:
            assert same_bits(hm[p], ref[p]), ("moments_host", M, p)
        g = pkg.GBT.getmoments([0, 0], [fil, h5], tblock=M)
        assert g.shape == (2,)
        for one, f in zip(g, (fil, h5)):
            assert isinstance(one, eng.Moments)
            per_file = W.getmoments(f, tblock=M)
            for p in PLANES:
                assert same_bits(getattr(one, p), getattr(per_file, p)), ("GBT", M, p)
                assert same_bits(getattr(one, p), ref[p]), ("GBT", M, p)
    # which, through the worker: the planes not asked for are None
    for name, src in sources:
        got = W.getmoments(src, which=("var", "skewness"))
        assert got.mean is None and got.kurtosis is None, name
        ref = planes(eng, eng.moments(x))
        assert same_bits(planes(eng, got)["var"], ref["var"]), name
    # a window through the file readers: channels 9..40, spectra 17..112
    idxs = (J(9, 40), C, J(17, 112))
    ww = [8, 32, 1, 0, 1, 1, 16, 96, 1]
    refw = planes(eng, eng.moments(x, ww))
    refwb = planes(eng, eng.moments(x, ww, tblock=8))
    assert_moments(refw, moments_statement(orc, a, ww), "mid", 96, "window")
    for src in (a, fil, raw5, h5):
        got, gotb = planes(eng, W.getmoments(src, idxs)), planes(eng, W.getmoments(src, idxs, tblock=8))
        for p in PLANES:
            assert same_bits(got[p], refw[p]) and same_bits(gotb[p], refwb[p]), p
    # an empty window: empty arrays, nothing launched
    e = eng.moments_host(a, [0, 0, 1, 0, 1, 1, 0, nt, 1])
    assert all(v.shape == (0, 1) for v in e)
    assert all(tuple(t.shape) == (0, 1, 8)
               for t in eng.moments(x, [0, 0, 1, 0, 1, 1, 0, nt, 1], tblock=16))
    # no spectra: NaN in every plane
    z = planes(eng, eng.moments(x, [0, 8, 1, 0, 1, 1, 0, 0, 1]))
    assert all(v.shape == (8, 1) and np.isnan(v).all() for v in z.values())


@pytest.mark.parametrize("win,path", [([0, 256, 1, 0, 2, 1, 0, 16, 1], "regs"),
                                      ([0, 256, 1, 0, 2, 1, 0, 200, 1], "mid"),
                                      ([0, 256, 1, 0, 2, 1, 0, 1030, 1], "leaf"),
                                      ([0, 6, 1, 0, 2, 1, 0, 1030, 1], "twopass")],
                         ids=["regs", "mid", "leaf", "twopass"])
def test_kurtosis_and_skewness_unchanged_by_a_moments_call(eng, xrows, win, path):
    """Shared scratch and plans: engine.kurtosis and engine.skewness return the
    same bits before and after a moments call on the same tensor (and the
    blocks too)."""
    assert eng.kurtosis_plan(xrows, win)["path"] == path
    M = win[7] // 2
    before = [host(eng, f(xrows, win, tblock=t)) for f in (eng.kurtosis, eng.skewness)
              for t in (None, M)]
    eng.moments(xrows, win)
    eng.moments(xrows, win, tblock=M)
    after = [host(eng, f(xrows, win, tblock=t)) for f in (eng.kurtosis, eng.skewness)
             for t in (None, M)]
    for b, a in zip(before, after):
        assert same_bits(a, b)
