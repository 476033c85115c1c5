"""GPU parity of getskewness against the statement of tests/skewness_ref.py
(StatsBase.skewness with Julia's Float32 mean), in the class of the path the
plan reports (engine.skewness_plan):
  regs     <= 32 spectra on float4-column windows: the same bits
  mid      33..512 spectra (and short windows without float4 columns):
           3 nt 2^-53 A
  leaf     > 512 spectra on float4-column windows, and blocks of 33..1024 in
           one launch: 9.5 2^-24 1.05 A
  twopass  > 512 spectra without float4 columns: 3 nt 2^-53 A
with A the absolute third moment over cm2^1.5 as the recipe forms it.  NaN and
+-Inf positions equal the statement's on every path.

Data: integrated-power rows, channel c with mean / sigma of {1.4, 30, 300, 3000,
30000}[c % 5], times 2^-10 so that every |z|^3 stays in Float32's normal range
(asserted: every expected value of the tolerance classes is finite), and
channel 5 of IF 0 one value plus an ulp.  The first 6 and 8 channels hold all
of them, so every path below sees every kind of row.  The overflow and
underflow rows are a test of their own and compare positions only.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits
from skewness_ref import (assert_positions, assert_skewness, block_win, skew_statement,
                          skew_statement_blocks)

pytestmark = pytest.mark.gpu

NC, NI, NT = 260, 2, 4104  # a partial 256-channel tile; the longest case takes 4097 spectra
SHAPES = [(8, 1), (256, 2), (260, 2)]


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def dev(eng, a):
    return eng.fb_from_numpy(np.asfortranarray(a), device="cuda:0")


def host(eng, t):
    return eng.fb_to_numpy(t)


def power_rows(rng, nc, ni, nt, nfpc=64):
    """Integrated-power filterbank (gamma with shape R^2, i.e. N_avg = R^2
    spectra of chi^2(2) power, skewness 2 / R) times a per-coarse-channel
    scallop and 2^-10; channel 5 of IF 0 is 2^20 with an ulp added at random."""
    R = np.array([np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0])[np.arange(nc) % 5]
    x = np.arange(nc) % nfpc
    bp = 0.2 + 0.8 * np.sin(np.pi * (x + 0.5) / nfpc) ** 2
    g = rng.gamma((R ** 2)[None, None, :], (1e9 / R ** 2 * bp)[None, None, :], (nt, ni, nc))
    a = np.asfortranarray(g.astype(np.float32).transpose(2, 1, 0) * np.float32(2.0 ** -10))
    if nc > 5:
        a[5, 0] = np.float32(2.0 ** 20) + np.float32(0.125) * rng.integers(0, 2, nt)
    return a


@pytest.fixture(scope="module")
def rows():
    """One array shared by the cases below (read-only): each takes a window."""
    a = power_rows(np.random.default_rng(20261), NC, NI, NT)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def xrows(eng, rows):
    return dev(eng, rows.copy(order="F"))  # (torch wants a writable source)


def check_window(eng, orc, rows, xrows, win, path, finite=True, msg=""):
    """engine.skewness of a window against the statement, on `path`."""
    plan = eng.skewness_plan(xrows, win)
    assert plan["path"] == path and plan["blocks"] == 1, (msg, plan)
    assert plan["path"] == eng.kurtosis_plan(xrows, win)["path"]
    want, A = skew_statement(orc, rows, win)
    if finite and win[7] >= 16:  # (two equal values of the ulp row are 0 / 0)
        assert np.isfinite(want).all(), msg
    s = eng.skewness(xrows, win)
    assert tuple(s.shape) == (win[1], win[4]) and str(s.dtype) == "torch.float64"
    got = host(eng, s)
    assert_skewness(got, want, A, path, win[7], (msg, win))
    return got


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("nt", [1, 2, 3, 16, 31, 32])
def test_regs_bit_for_bit(pkg, eng, orc, rows, xrows, nt, exact):
    """k_kurt_regs<., ., 3>: the recipe in its own order (kurt_exact at both
    values); a single spectrum is 0 / 0."""
    with pkg._lib.plan_option("kurt_exact", exact):
        for nc, ni in SHAPES:
            got = check_window(eng, orc, rows, xrows, [0, nc, 1, 0, ni, 1, 0, nt, 1], "regs")
            if nt == 1:
                assert np.isnan(got).all()
        # channel 1: float4 columns on a dword boundary; a reversed time range
        w1 = [1, 256, 1, 0, 2, 1, 0, nt, 1]
        check_window(eng, orc, rows, xrows, w1, eng.kurtosis_plan(xrows, w1)["path"])
        check_window(eng, orc, rows, xrows, [0, 256, 1, 0, 2, 1, 40 + nt - 1, nt, -1], "regs")


@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("nt", [33, 64, 65, 384, 385, 512])
def test_mid(pkg, eng, orc, rows, xrows, nt, small):
    """k_kurt_mid2 (<= 384 spectra of float4 columns; kurt_mid_small at both
    values) and k_kurt_mid: the recipe's terms, partial sums in wave order."""
    with pkg._lib.plan_option("kurt_mid_small", small):
        for nc, ni in SHAPES:
            check_window(eng, orc, rows, xrows, [0, nc, 1, 0, ni, 1, 3, nt, 1], "mid")
        # no float4 columns: 6 channels, and a channel step of 2
        check_window(eng, orc, rows, xrows, [0, 6, 1, 0, 2, 1, 0, nt, 1], "mid")
        check_window(eng, orc, rows, xrows, [0, 130, 2, 0, 2, 1, 0, nt, 1], "mid")


@pytest.mark.parametrize("narrow", [0, 4])
@pytest.mark.parametrize("nt", [513, 1024, 1025, 2049, 4097])
def test_leaf(pkg, eng, orc, rows, xrows, nt, narrow):
    """k_kurt_leaf + the tree + k_kurt_final_*<., 3> (kurt_leaf_narrow at both
    values): skew_ratio from the merged moments."""
    with pkg._lib.plan_option("kurt_leaf_narrow", narrow):
        for nc, ni in SHAPES:
            check_window(eng, orc, rows, xrows, [0, nc, 1, 0, ni, 1, 0, nt, 1], "leaf")


def test_leaf_with_a_tree_pass(eng, orc):
    """More than 131072 spectra: 128 blocks, so a k_kurt_tree pass runs before
    the final level."""
    nt = 140001
    a = power_rows(np.random.default_rng(3), 8, 1, nt)
    x = dev(eng, a)
    assert eng.kurtosis_plan(x)["K"] == 7
    check_window(eng, orc, a, x, [0, 8, 1, 0, 1, 1, 0, nt, 1], "leaf")


@pytest.mark.parametrize("nt", [600, 3000])
def test_twopass(eng, orc, rows, xrows, nt):
    """No float4 columns and more than 512 spectra: Julia's mean through the
    tree, then k_kurt_pass<3> (and k_kurt_fold<3> over its time chunks)."""
    check_window(eng, orc, rows, xrows, [0, 6, 1, 0, 2, 1, 0, nt, 1], "twopass")
    check_window(eng, orc, rows, xrows, [0, 6, 1, 1, 1, 1, 7, nt, 1], "twopass")


def test_integrated_power_rows_have_their_known_skewness(eng, orc, rows, xrows):
    """The 6 and 8 channel windows of the cases above hold every kind of row;
    over 4096 spectra the gamma rows sit at 2 / (mean / sigma) within sampling
    noise.  The one-value-plus-an-ulp row has no such value: its Float32 mean
    rounds onto one of the two values, so every z is 0 or one ulp of one sign
    and the recipe gives +-1 / sqrt(the other value's share)."""
    win = [0, 8, 1, 0, 1, 1, 0, 4096, 1]
    got = check_window(eng, orc, rows, xrows, win, "leaf")[:, 0]
    R = np.array([np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0])
    noise = 6.0 * np.sqrt(6.0 / 4096)  # 6 sigma of a Gaussian sample's skewness
    assert np.abs(got[:5] - 2.0 / R).max() < noise
    p = float((rows[5, 0, :4096] != rows[5, 0, :4096].min()).mean())
    assert min(abs(abs(got[5]) - 1 / np.sqrt(p)), abs(abs(got[5]) - 1 / np.sqrt(1 - p))) < 1e-5


def nonfinite_rows(rng, nt):
    """(array, expected) of 12 x 1 x nt: rows whose extremes make the Float32
    squares and cubes overflow or underflow, and non-finite inputs."""
    a = np.asfortranarray(rng.uniform(0.5, 1.5, (12, 1, nt)).astype(np.float32))
    exp = {}
    a[1, 0] = (1e30 * (1.0 + 0.1 * rng.standard_normal(nt))).astype(np.float32)
    exp[1] = np.nan  # z^2 overflows: cubes of both signs, Inf / Inf
    a[2, 0, nt // 2] = 3e13
    exp[2] = np.inf  # only z^3 overflows, at the maximum
    a[3, 0, nt // 3] = -3e13
    exp[3] = -np.inf  # ... at the minimum
    a[4, 0, 0], a[4, 0, nt - 1] = 3e13, -3e13
    exp[4] = np.nan  # ... at both: Inf - Inf
    a[5, 0] = (1e-17 * (1.0 + 0.5 * rng.uniform(-1, 1, nt))).astype(np.float32)
    exp[5] = 0.0  # every cube underflows, the squares do not
    a[6, 0, 1] = np.nan
    exp[6] = np.nan
    a[7, 0, nt - 2] = np.inf
    exp[7] = np.nan
    a[8, 0, 2] = -np.inf
    exp[8] = np.nan
    return a, exp


@pytest.mark.parametrize("nt,path", [(16, "regs"), (100, "mid"), (1025, "leaf")])
def test_nonfinite_positions_and_signs(eng, orc, nt, path):
    a, exp = nonfinite_rows(np.random.default_rng(50 + nt), nt)
    x = dev(eng, a)
    assert eng.skewness_plan(x)["path"] == path
    want, A = skew_statement(orc, a)
    for r, v in exp.items():  # the statement itself does what the rows are built for
        assert same_bits(want[r, 0:1], np.array([v])), (r, want[r, 0], v)
    ordinary = [0, 9, 10, 11]
    assert np.isfinite(want[ordinary]).all()
    got = host(eng, eng.skewness(x))
    assert_positions(got, want, (nt, path))
    assert got[5, 0] == 0.0
    assert_skewness(got[ordinary], want[ordinary], A[ordinary], path, nt, "ordinary rows")


def check_blocks(got, want, A, path, M, msg=""):
    assert got.shape == want.shape and got.dtype == np.float64, (msg, got.shape, want.shape)
    for b in range(want.shape[2]):
        assert_skewness(got[:, :, b], want[:, :, b], A[:, :, b], path, M, (msg, "block", b))


BLOCKS = [(1, 5), (2, 3), (16, 3), (32, 3), (33, 3), (64, 5), (1024, 2), (1025, 2), (2048, 2)]


@pytest.mark.parametrize("M,nb", BLOCKS, ids=[f"M{m}x{n}" for m, n in BLOCKS])
def test_block_forms(eng, orc, rows, xrows, M, nb):
    """tblock: registers (M <= 32, one launch, the bits of the windowed call of
    every block), one streamed leaf (33..1024, one launch, no workspace), block
    by block above one leaf and without float4 columns."""
    for nc, ni in SHAPES[1:] + [(6, 2)]:
        win = [0, nc, 1, 0, ni, 1, 5, M * nb, 1]
        plan = eng.skewness_plan(xrows, win, tblock=M)
        kplan = eng.kurtosis_blocks_plan(xrows, M, win)
        assert {k: plan[k] for k in ("path", "fused", "blocks")} == \
            {k: kplan[k] for k in ("path", "fused", "blocks")}
        assert plan["blocks"] == nb
        if nc == 6 or M > 1024:
            assert plan["fused"] == 0, plan
        else:
            assert plan["fused"] == 1 and plan["workspace_bytes"] == 0, plan
            assert plan["path"] == ("regs" if M <= 32 else "leaf")
        want, A = skew_statement_blocks(orc, rows, win, M)
        if M == 1:
            assert np.isnan(want).all()  # 0 / 0: the recipe of a single spectrum
        elif M >= 16:
            assert np.isfinite(want).all()
        s = eng.skewness(xrows, win, tblock=M)
        assert tuple(s.shape) == (nc, ni, nb)
        got = host(eng, s)
        check_blocks(got, want, A, plan["path"], M, plan)
        if plan["fused"] and M <= 32:
            for b in range(nb):
                one = host(eng, eng.skewness(xrows, block_win(rows.shape, win, M, b)))
                assert same_bits(got[:, :, b], one), (M, b)


@pytest.mark.parametrize("M", [16, 64, 1030])
def test_nonfinite_values_stay_in_their_block(eng, orc, M):
    nb, nc = 4, 256
    rng = np.random.default_rng(900 + M)
    a = power_rows(rng, nc, 1, M * nb)
    blk = lambda b: slice(b * M, (b + 1) * M)  # noqa: E731
    a[3, 0, blk(1)] = np.float32(2.0 ** 19)  # constant in block 1 only: 0 / 0
    a[10, 0, 5] = np.nan
    a[20, 0, (nb - 1) * M + M // 2] = np.inf
    a[30, 0, blk(2)] = (1e30 * (1.0 + 0.1 * rng.standard_normal(M))).astype(np.float32)
    a[40, 0, M + 3] = 3e13  # only its cube overflows: +Inf in block 1
    a[50, 0, 2 * M + 1] = -3e13  # -Inf in block 2
    x = dev(eng, a)
    plan = eng.skewness_plan(x, tblock=M)
    assert plan["fused"] == (1 if M <= 1024 else 0)
    want, A = skew_statement_blocks(orc, a, None, M)
    nan = np.zeros(want.shape, bool)
    nan[3, 0, 1] = nan[10, 0, 0] = nan[20, 0, nb - 1] = nan[30, 0, 2] = True
    assert np.array_equal(np.isnan(want), nan)
    assert want[40, 0, 1] == np.inf and want[50, 0, 2] == -np.inf and np.isinf(want).sum() == 2
    got = host(eng, eng.skewness(x, tblock=M))
    check_blocks(got, want, A, plan["path"], M, M)


@pytest.mark.parametrize("M,win", [(0, None), (16, None), (64, None),
                                   (16, [0, 128, 2, 0, 2, 1, 0, 48, 1]),
                                   (0, [0, 128, 2, 0, 2, 1, 0, 48, 1])],
                         ids=["whole", "regs", "stream", "block-by-block", "whole-step"])
def test_strided_out_through_the_abi(pkg, eng, M, win):
    """bldp_skewness_f32 itself: out_ld_i / out_ld_b larger than dense: the
    values of the dense call, the padding untouched; overlapping strides are
    refused."""
    import torch

    nc, ni = 256, 2
    nt = 48 if M == 0 else 3 * M
    a = power_rows(np.random.default_rng(77 + M), nc, ni, nt)
    x = dev(eng, a)
    dense = host(eng, eng.skewness(x, win, tblock=M or None))
    if M == 0:
        dense = dense[:, :, None]
    nco, nb = dense.shape[0], dense.shape[2]
    ld_i = nco + 3
    ld_b = ld_i * ni + 5
    out = torch.full((nb * ld_b + 7,), -7.0, dtype=torch.float64, device="cuda:0")
    L = pkg._lib.lib()
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    keep, wp = pkg._lib.win_arg(win)
    rc = L.bldp_skewness_f32(ptr, nchan, nif, ntime, wp, M, out.data_ptr(), ld_i, ld_b,
                             pkg._lib.stream_ptr())
    pkg._lib.check(rc, "bldp_skewness_f32")
    o = out.cpu().numpy()
    used = np.zeros(o.shape, bool)
    for b in range(nb):
        for i in range(ni):
            s = slice(b * ld_b + i * ld_i, b * ld_b + i * ld_i + nco)
            assert same_bits(o[s], dense[:, i, b]), (b, i)
            used[s] = True
    assert (o[~used] == -7.0).all()
    rc = L.bldp_skewness_f32(ptr, nchan, nif, ntime, wp, M, out.data_ptr(), nco - 1, ld_b,
                             pkg._lib.stream_ptr())
    assert rc == pkg._lib.BLDP_EINVAL


@pytest.mark.parametrize("M,nt,win", [(None, 16, None), (None, 100, None), (None, 1030, None),
                                      (None, 600, [0, 6, 1, 0, 1, 1, 0, 600, 1]),
                                      (16, 64, None), (256, 768, None),
                                      (16, 64, [0, 256, 2, 0, 1, 1, 0, 64, 1])],
                         ids=["regs", "mid", "leaf", "twopass", "M16", "M256", "M16-channel-step"])
def test_band(eng, orc, M, nt, win):
    """Three banks in one set of launches: each bank's results are the bits of
    its own single call, and in the class of the path."""
    rng = np.random.default_rng(31 * nt)
    arrs = [power_rows(rng, 512, 1, nt) for _ in range(3)]
    xs = [dev(eng, a) for a in arrs]
    ss = eng.band_skewness(xs, win, tblock=M)
    assert len(ss) == 3
    plan = eng.skewness_plan(xs[0], win, tblock=M)
    nc = 512 if win is None else win[1]
    for k, (a, x) in enumerate(zip(arrs, xs)):
        assert tuple(ss[k].shape) == ((nc, 1) if M is None else (nc, 1, nt // M))
        got = host(eng, ss[k])
        assert same_bits(got, host(eng, eng.skewness(x, win, tblock=M))), k
        if M is None:
            want, A = skew_statement(orc, a, win)
            assert_skewness(got, want, A, plan["path"], nt, k)
        else:
            want, A = skew_statement_blocks(orc, a, win, M)
            check_blocks(got, want, A, plan["path"], M, k)


def test_layers(pkg, eng, orc, tmp_path):
    """worker.getskewness on every source it handles (tensor, host array, raw
    SIGPROC file, compressed FBH5 file), GBT's fan-out, engine.skewness_host,
    with and without tblock and through a window."""
    W, C, J = pkg.WorkerFunctions, pkg.COLON, pkg.JRange
    nc, nt = 64, 128
    a = power_rows(np.random.default_rng(4), nc, 1, nt)
    x = dev(eng, a)
    fil, h5 = str(tmp_path / "s.fil"), str(tmp_path / "s.rawspec.0002.h5")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=nc, nifs=1, tsamp=1.0,
                                    nbits=32, telescope_id=6, machine_id=10, data_type=1,
                                    tstart=59000.0, source_name="X"), a)
    pkg.fbh5.write_bslz4(h5, dict(foff=-1.0, nfpc=64), a, (16, 1, nc),
                         lambda blk: orc.np_bslz4_encode(blk, 512, lz4=orc.lz4_compress))
    sources = (("tensor", x), ("host", a), ("fil", fil), ("bslz4", h5))
    want, A = skew_statement(orc, a)
    path = eng.skewness_plan(x)["path"]
    assert path == "mid"
    for name, src in sources:
        got = W.getskewness(src)
        got = host(eng, got) if name == "tensor" else got
        assert got.shape == (nc, 1) and got.dtype == np.float64, name
        assert_skewness(got, want, A, path, nt, name)
    assert_skewness(eng.skewness_host(a), want, A, path, nt, "skewness_host")
    for M in (16, 64):
        plan = eng.skewness_plan(x, tblock=M)
        wantb, Ab = skew_statement_blocks(orc, a, None, M)
        for name, src in sources:
            got = W.getskewness(src, tblock=M)
            got = host(eng, got) if name == "tensor" else got
            check_blocks(np.asarray(got), wantb, Ab, plan["path"], M, (name, M))
        check_blocks(eng.skewness_host(a, tblock=M), wantb, Ab, plan["path"], M, "host")
        ks = pkg.GBT.getskewness([0, 0], [fil, h5], tblock=M)
        assert ks.shape == (2,)
        for k in ks:
            check_blocks(k, wantb, Ab, plan["path"], M, ("GBT", M))
    # a window through the file readers: channels 9..40, spectra 17..112
    idxs = (J(9, 40), C, J(17, 112))
    ww = [8, 32, 1, 0, 1, 1, 16, 96, 1]
    wantw, Aw = skew_statement(orc, a, ww)
    wantwb, Awb = skew_statement_blocks(orc, a, ww, 8)
    for src in (a, fil, h5):
        assert_skewness(W.getskewness(src, idxs), wantw, Aw, "mid", 96, "window")
        check_blocks(W.getskewness(src, idxs, tblock=8), wantwb, Awb, "regs", 8, "window")
    for k in pkg.GBT.getskewness([0, 0], [fil, h5]):
        assert_skewness(k, want, A, path, nt, "GBT")
    # an empty window: an empty array, nothing launched
    assert eng.skewness_host(a, [0, 0, 1, 0, 1, 1, 0, nt, 1]).shape == (0, 1)
    assert tuple(eng.skewness(x, [0, 0, 1, 0, 1, 1, 0, nt, 1], tblock=16).shape) == (0, 1, 8)


@pytest.mark.parametrize("win,path", [([0, 256, 1, 0, 2, 1, 0, 16, 1], "regs"),
                                      ([0, 256, 1, 0, 2, 1, 0, 200, 1], "mid"),
                                      ([0, 256, 1, 0, 2, 1, 0, 1030, 1], "leaf"),
                                      ([0, 6, 1, 0, 2, 1, 0, 1030, 1], "twopass")],
                         ids=["regs", "mid", "leaf", "twopass"])
def test_kurtosis_unchanged_by_a_skewness_call(eng, xrows, win, path):
    """Shared scratch and plans: engine.kurtosis returns the same bits before
    and after a skewness call on the same tensor (and the blocks too)."""
    assert eng.kurtosis_plan(xrows, win)["path"] == path
    k0 = host(eng, eng.kurtosis(xrows, win))
    b0 = host(eng, eng.kurtosis(xrows, win, tblock=win[7] // 2))
    eng.skewness(xrows, win)
    eng.skewness(xrows, win, tblock=win[7] // 2)
    assert same_bits(host(eng, eng.kurtosis(xrows, win)), k0)
    assert same_bits(host(eng, eng.kurtosis(xrows, win, tblock=win[7] // 2)), b0)
