"""GPU parity of getkurtosis(...; tblock = M): the kurtosis of every block of M
selected spectra, (nc, ni, nt / M), against the oracle block by block.

Element [c, i, b] is what the whole-window getkurtosis gives for block b
alone, so the classes are those of tests/conftest.py assert_kurtosis, by the
path the plan reports (engine.kurtosis_blocks_plan):
  regs   M <= 32 on float4-column windows, one launch: bit-exact
  leaf   32 < M <= 1024 on float4-column windows, one launch: the moments exact
         in Float64 (KURT_LEAF_TOL); the mean is Julia's bits
  other  M > 1024, or no float4 columns: block by block inside the library on
         the whole-window paths (fused == 0), the class of that path
NaN and +-Inf positions match the recipe exactly on every form.

Data: the integrated-power rows of tests/test_gpu_kurtosis.py (mean / sigma
up to 3e4) times 2^-10.  At their own scale (1e9) the recipe's Float32 z^4
overflows in blocks of some hundred spectra of the mean / sigma = 1.4 channels
(z > 4.3e9), so expected values would be +Inf there; the power of two moves
every value's exponent and no mantissa bit, the kurtosis is the same number,
and every expected value is finite: asserted here, so that the finite-only
comparison of assert_kurtosis hides nothing.  The long blocks also run at the
rows' own scale, where the +Inf positions must match.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from conftest import assert_kurtosis, same_bits

pytestmark = pytest.mark.gpu

NC, NI, NT = 260, 2, 2060  # a partial 256-channel tile; the longest case takes 2050 spectra


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def dev(eng, a):
    return eng.fb_from_numpy(a, device="cuda:0")


def host(eng, t):
    return eng.fb_to_numpy(t)


def power_rows(rng, nc, ni, nt, nfpc=64):
    """Integrated-power filterbank: channel c has mean/sigma R[c % 5] of
    {1.4, 30, 300, 3000, 30000} (gamma with shape R^2, i.e. N_avg = R^2
    spectra of chi^2(2) power), times a per-coarse-channel scallop."""
    R = np.array([np.sqrt(2.0), 30.0, 300.0, 3000.0, 30000.0])[np.arange(nc) % 5]
    x = np.arange(nc) % nfpc
    bp = 0.2 + 0.8 * np.sin(np.pi * (x + 0.5) / nfpc) ** 2
    g = rng.gamma((R ** 2)[None, None, :], (1e9 / R ** 2 * bp)[None, None, :], (nt, ni, nc))
    return np.asfortranarray(g.astype(np.float32).transpose(2, 1, 0))


def finite_rows(rng, nc, ni, nt):
    """power_rows times 2^-10 (exact): no z^4 overflows, every kurtosis is finite."""
    return np.asfortranarray(power_rows(rng, nc, ni, nt) * np.float32(2.0 ** -10))


@pytest.fixture(scope="module")
def rows():
    """One array shared by the cases below (read-only): each takes a window."""
    a = finite_rows(np.random.default_rng(20260), NC, NI, NT)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def xrows(eng, rows):
    return dev(eng, rows.copy(order="F"))  # (torch wants a writable source)


def block_win(shape, win, M, b):
    w = list(win) if win is not None else [0, shape[0], 1, 0, shape[1], 1, 0, shape[2], 1]
    w[6] += b * M * w[8]
    w[7] = M
    return w


def oracle_blocks(orc, a, win, M):
    """np.stack of the oracle's whole-window kurtosis of every block."""
    nt = orc.window_shape(a.shape, win)[2]
    assert nt % M == 0
    return np.stack([orc.kurtosis(a, block_win(a.shape, win, M, b)) for b in range(nt // M)],
                    axis=2)


def check_blocks(got, want, path, M, msg=""):
    assert got.shape == want.shape and got.dtype == np.float64, (msg, got.shape, want.shape)
    for b in range(want.shape[2]):
        assert_kurtosis(got[:, :, b], want[:, :, b], path, M, (msg, "block", b))


CASES = [(1, 5), (2, 3), (7, 5), (16, 3), (32, 3), (33, 3), (64, 5), (100, 3), (512, 2), (1024, 2),
         (1025, 2), (2049, 1)]


@pytest.mark.parametrize("M,nb", CASES, ids=[f"M{m}x{n}" for m, n in CASES])
def test_forms_and_edges(eng, orc, rows, xrows, M, nb):
    """Every form: registers (M <= 32, bit-exact, and equal to the windowed
    whole-window call of each block), one streamed leaf (33..1024), block by
    block above one leaf; 260 channels leave a partial 256-channel tile."""
    win = [0, NC, 1, 0, NI, 1, 0, M * nb, 1]
    plan = eng.kurtosis_blocks_plan(xrows, M, win)
    assert plan["blocks"] == nb
    if M <= 32:
        assert (plan["fused"], plan["path"]) == (1, "regs"), plan
    elif M <= 1024:
        assert plan["fused"] == 1 and plan["workspace_bytes"] == 0, plan
    else:
        assert plan["fused"] == 0, plan
        assert plan["path"] == eng.kurtosis_plan(xrows, block_win(rows.shape, win, M, 0))["path"]
    want = oracle_blocks(orc, rows, win, M)
    if M == 1:
        assert np.isnan(want).all()  # 0 / 0: the recipe of a single spectrum
    else:
        assert np.isfinite(want).all()
    k = eng.kurtosis(xrows, win, tblock=M)
    assert tuple(k.shape) == (NC, NI, nb)
    got = host(eng, k)
    check_blocks(got, want, plan["path"], M, plan)
    if plan["path"] == "regs":
        for b in range(nb):
            one = host(eng, eng.kurtosis(xrows, block_win(rows.shape, win, M, b)))
            assert same_bits(got[:, :, b], one), (M, b)
    if M >= 512:  # the rows' own scale: z^4 overflows in the widest channels, +Inf there
        big = np.asfortranarray(rows[:, :, :M * nb] * np.float32(1024.0))
        wantb = oracle_blocks(orc, big, None, M)
        assert np.isinf(wantb).any() and not np.isnan(wantb).any()
        assert np.array_equal(wantb[np.isfinite(wantb)], want[np.isfinite(wantb)])
        check_blocks(host(eng, eng.kurtosis(dev(eng, big), tblock=M)), wantb, plan["path"], M, "1e9")


WINDOWS = [
    # (window without its spectrum count, float4 columns)
    ("channels 4..255", [4, 252, 1, 0, 2, 1, 0, None, 1], True),
    ("time offset 3 step 2", [0, 260, 1, 0, 2, 1, 3, None, 2], True),
    ("IF 1 only", [0, 260, 1, 1, 1, 1, 0, None, 1], True),
    ("all three", [4, 252, 1, 1, 1, 1, 3, None, 2], True),
    ("channel start 1 count 257", [1, 257, 1, 0, 2, 1, 0, None, 1], False),
    ("channel step 2", [0, 130, 2, 0, 2, 1, 3, None, 2], False),
]


@pytest.mark.parametrize("name,w,vec", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_windows(eng, orc, rows, xrows, name, w, vec):
    """The blocks cut the window's selected spectra (after a time offset and
    step); windows without float4 columns run block by block, in the class of
    the path the plan reports."""
    for M, nb in ((16, 3), (64, 3)):
        win = list(w)
        win[7] = M * nb
        plan = eng.kurtosis_blocks_plan(xrows, M, win)
        assert plan["fused"] == (1 if vec else 0), (name, plan)
        assert plan["blocks"] == nb
        if not vec:
            assert plan["path"] == "mid", plan  # the whole-window path of <= 512 spectra
        want = oracle_blocks(orc, rows, win, M)
        assert np.isfinite(want).all()
        got = host(eng, eng.kurtosis(xrows, win, tblock=M))
        check_blocks(got, want, plan["path"], M, (name, M))


@pytest.mark.parametrize("M", [16, 64, 1030])
def test_no_leakage_between_blocks(eng, orc, M):
    """Non-finite values stay in their block: a row constant in block 1 only
    (NaN there), a NaN in block 0, +Inf in the last block, a block near 1e30
    (z^2 overflows Float32: Inf / Inf) and one near 1e12 (only z^4 overflows:
    +Inf).  Everything else stays finite and within the class."""
    nb, nc = 4, 256
    rng = np.random.default_rng(900 + M)
    a = finite_rows(rng, nc, 1, M * nb)
    blk = lambda b: slice(b * M, (b + 1) * M)  # noqa: E731
    a[3, 0, blk(1)] = np.float32(2.0 ** 19)  # (its sums are exact: mean == value, z == 0)
    a[10, 0, 5] = np.nan
    a[20, 0, (nb - 1) * M + M // 2] = np.inf
    a[30, 0, blk(2)] = (1e30 * (1.0 + 0.1 * rng.standard_normal(M))).astype(np.float32)
    a[40, 0, blk(1)] = (1e12 * (1.0 + 0.1 * rng.standard_normal(M))).astype(np.float32)
    x = dev(eng, a)
    plan = eng.kurtosis_blocks_plan(x, M)
    assert plan["fused"] == (1 if M <= 1024 else 0)
    want = oracle_blocks(orc, a, None, M)
    nan = np.zeros(want.shape, bool)
    nan[3, 0, 1] = nan[10, 0, 0] = nan[20, 0, nb - 1] = nan[30, 0, 2] = True
    assert np.array_equal(np.isnan(want), nan)
    assert want[40, 0, 1] == np.inf and np.isinf(want).sum() == 1
    got = host(eng, eng.kurtosis(x, tblock=M))
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(np.isinf(got), np.isinf(want)) and got[40, 0, 1] == np.inf
    check_blocks(got, want, plan["path"], M, M)


@pytest.mark.parametrize("M,nb,win", [(16, 4, None), (256, 3, None),
                                      (16, 4, [0, 256, 2, 0, 1, 1, 0, 64, 1])],
                         ids=["M16", "M256", "M16-channel-step"])
def test_band(eng, orc, M, nb, win):
    """Three banks in one set of launches: each bank equals its own single
    call bit for bit (also block by block, where the results are scattered
    into the band's product)."""
    rng = np.random.default_rng(31 * M + nb)
    arrs = [finite_rows(rng, 512, 1, M * nb) for _ in range(3)]
    xs = [dev(eng, a) for a in arrs]
    ks = eng.band_kurtosis(xs, win, tblock=M)
    assert len(ks) == 3
    plan = eng.kurtosis_blocks_plan(xs[0], M, win)
    assert plan["fused"] == (1 if win is None else 0)
    nc = 512 if win is None else win[1]
    for k, (a, x) in enumerate(zip(arrs, xs)):
        assert tuple(ks[k].shape) == (nc, 1, nb)
        got = host(eng, ks[k])
        assert same_bits(got, host(eng, eng.kurtosis(x, win, tblock=M))), k
        check_blocks(got, oracle_blocks(orc, a, win, M), plan["path"], M, k)


def test_layers(pkg, eng, orc, tmp_path):
    """worker.getkurtosis with tblock on every source it handles, GBT's
    fan-out, tblock=None (today's 2-D result) and tblock = nt (one block)."""
    W, C, J = pkg.WorkerFunctions, pkg.COLON, pkg.JRange
    nc, nt = 64, 128
    rng = np.random.default_rng(4)
    a = finite_rows(rng, nc, 1, nt)
    x = dev(eng, a)
    fil, h5 = str(tmp_path / "k.fil"), str(tmp_path / "k.rawspec.0002.h5")
    pkg.readers.write_fil(fil, dict(fch1=8000.0, foff=-1.0, nchans=nc, nifs=1, tsamp=1.0,
                                    nbits=32, telescope_id=6, machine_id=10, data_type=1,
                                    tstart=59000.0, source_name="X"), a)
    pkg.fbh5.write_bslz4(h5, dict(foff=-1.0, nfpc=64), a, (16, 1, nc),
                         lambda blk: orc.np_bslz4_encode(blk, 512, lz4=orc.lz4_compress))
    whole = host(eng, eng.kurtosis(x))
    for M in (16, 64):
        plan = eng.kurtosis_blocks_plan(x, M)
        assert plan["fused"] == 1
        want = oracle_blocks(orc, a, None, M)
        assert np.isfinite(want).all()
        for name, src in (("tensor", x), ("host", a), ("fil", fil), ("bslz4", h5)):
            got = W.getkurtosis(src, tblock=M)
            got = host(eng, got) if name == "tensor" else got
            check_blocks(np.asarray(got), want, plan["path"], M, (name, M))
        # a window through the file readers: channels 9..40, spectra 17..112
        idxs = (J(9, 40), C, J(17, 112))
        ww = [8, 32, 1, 0, 1, 1, 16, 96, 1]
        wantw = oracle_blocks(orc, a, ww, M // 2)
        for src in (a, fil, h5):
            check_blocks(W.getkurtosis(src, idxs, tblock=M // 2), wantw,
                         "regs" if M // 2 <= 32 else "leaf", M // 2, (src is a, M))
        ks = pkg.GBT.getkurtosis([0, 0], [fil, h5], tblock=M)
        assert ks.shape == (2,)
        for k in ks:
            check_blocks(k, want, plan["path"], M, ("GBT", M))
    # tblock=None: the 2-D result, the bits of the whole-window call
    for name, src in (("tensor", x), ("host", a), ("fil", fil), ("bslz4", h5)):
        k, k0 = W.getkurtosis(src, tblock=None), W.getkurtosis(src)
        if name == "tensor":
            k, k0 = host(eng, k), host(eng, k0)
        assert k.shape == (nc, 1) and same_bits(k, k0), name
        assert_kurtosis(k, orc.kurtosis(a), eng.kurtosis_plan(x)["path"], nt, name)
    assert same_bits(host(eng, W.getkurtosis(x)), whole)
    # tblock = nt: one block, the whole window's kurtosis within the class
    one = host(eng, eng.kurtosis(x, tblock=nt))
    assert one.shape == (nc, 1, 1)
    assert_kurtosis(one[:, :, 0], orc.kurtosis(a), eng.kurtosis_blocks_plan(x, nt)["path"], nt)
    # 16-bit rows: the existing typed calls, stacked
    a16 = np.asfortranarray(rng.integers(-2000, 2000, (nc, 1, nt)).astype(np.int16))
    got = W.getkurtosis(a16, tblock=16)
    assert got.shape == (nc, 1, 8) and got.dtype == np.float64
    for b in range(8):
        assert same_bits(got[:, :, b], W.getkurtosis(a16, (C, C, J(16 * b + 1, 16 * b + 16)))), b
    t16 = eng.kurtosis(__import__("torch").from_numpy(
        np.ascontiguousarray(a16.transpose(2, 1, 0))).to("cuda:0").permute(2, 1, 0), tblock=16)
    assert same_bits(host(eng, t16), got)


@pytest.mark.parametrize("M,win", [(16, None), (64, None), (16, [0, 128, 2, 0, 2, 1, 0, 48, 1])],
                         ids=["regs", "stream", "block-by-block"])
@pytest.mark.parametrize("pad_i,pad_b", [(8, 5), (3, 0)], ids=["even", "odd"])
def test_strided_out_through_the_abi(pkg, eng, M, win, pad_i, pad_b):
    """out_ld_i / out_ld_b larger than dense (16-byte aligned rows and not):
    the values of the dense call, the padding untouched."""
    import torch

    nc, ni, nb = 256, 2, 3
    a = finite_rows(np.random.default_rng(77 + M), nc, ni, M * nb)
    x = dev(eng, a)
    dense = host(eng, eng.kurtosis(x, win, tblock=M))
    nco = dense.shape[0]
    ld_i = nco + pad_i
    ld_b = ld_i * ni + pad_b
    out = torch.full((nb * ld_b + 7,), -7.0, dtype=torch.float64, device="cuda:0")
    L = pkg._lib.lib()
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    keep, wp = pkg._lib.win_arg(win)
    rc = L.bldp_kurtosis_blocks_f32(ptr, nchan, nif, ntime, wp, M, out.data_ptr(), ld_i, ld_b,
                                    pkg._lib.stream_ptr())
    pkg._lib.check(rc, "bldp_kurtosis_blocks_f32")
    o = out.cpu().numpy()
    used = np.zeros(o.shape, bool)
    for b in range(nb):
        for i in range(ni):
            s = slice(b * ld_b + i * ld_i, b * ld_b + i * ld_i + nco)
            assert same_bits(o[s], dense[:, i, b]), (b, i)
            used[s] = True
    assert (o[~used] == -7.0).all()
    # strides that would overlap are refused
    rc = L.bldp_kurtosis_blocks_f32(ptr, nchan, nif, ntime, wp, M, out.data_ptr(), nco - 1, ld_b,
                                    pkg._lib.stream_ptr())
    assert rc == pkg._lib.BLDP_EINVAL
