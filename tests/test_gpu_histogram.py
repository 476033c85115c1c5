"""The histogram on the GPU (csrc/hist.hip) against the NumPy restatement of its
rule (tests/histogram_ref.py).  Counts are integers: every plane of every block
is compared for equality, the planes of a block add up to F * T, and a second
call gives the same bits.  Every plan path and load width runs (the table of
histogram_ref.PLAN_CASES), each case asserting its plan first."""
from __future__ import annotations

import numpy as np
import pytest

from histogram_ref import PLAN_CASES, hist_edges_ref, hist_planes, histogram_ref
from mad_ref import window

pytestmark = pytest.mark.gpu

LO, HI = -60.0, 150.0  # inside the range of signed(): both tails are populated


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def put(eng, a):
    return eng.fb_from_numpy(np.asfortranarray(a), device="cuda:0")


def signed(shape, seed):
    """Gamma-like, peaked and signed: about -100 .. 900, the median near -16."""
    return (np.random.default_rng(seed).gamma(2.0, 50.0, shape) - 100.0).astype(np.float32)


def check(eng, a, B, lo, hi, F, T, win=None, x=None):
    """One window on the GPU against the restatement; returns the counts."""
    import torch

    x = put(eng, a) if x is None else x
    w = window(a, win)
    Fe = max(w.shape[0], 1) if F is None else F
    Te = max(w.shape[2], 1) if T is None else T
    want = histogram_ref(w, B, lo, hi, Fe, Te)
    got = eng.histogram(x, B, lo, hi, F, T, win)
    g = eng.planes_to_numpy(got)
    assert got.dtype == torch.int32 and g.shape == want.shape, (g.shape, want.shape)
    bad = np.argwhere(g != want)
    assert bad.size == 0, (B, F, T, win, bad[:5], g[tuple(bad[0])], want[tuple(bad[0])])
    assert (g.sum(axis=-1) == Fe * Te).all()
    again = eng.histogram(x, B, lo, hi, F, T, win)
    assert torch.equal(got, again)
    return g


# ---- every plan path x load width ---------------------------------------------------
@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_every_plan_path(eng, name):
    dims, F, T, B, win, (path, vec, chunks, bpw) = PLAN_CASES[name]
    a = signed(dims, sum(map(ord, name)))
    x = put(eng, a)
    p = eng.histogram_plan(x, B, LO, HI, F, T, win)
    assert (p["path"], p["vector_loads"], p["chunks_per_block"], p["blocks_per_workgroup"]) == \
        (path, vec, chunks, bpw), p
    g = check(eng, a, B, LO, HI, F, T, win, x=x)
    if a.size >= 64:  # both tails and the bins hold samples
        assert g[..., B].sum() > 0 and g[..., B + 1].sum() > 0 and g[..., :B].sum() > 0


# ---- the rule's edges, planted at known positions in several blocks ---------------------
@pytest.mark.parametrize("lo,hi,B", [(-1.0, 1.0, 7), (-5.0, 5.0, 100), (0.0, 1.0, 4)])
@pytest.mark.parametrize("F,T", [(4, 3), (16, 12), (1, 1), (1, 12)])
def test_rule_edges(eng, lo, hi, B, F, T):
    lo32, hi32 = np.float32(lo), np.float32(hi)
    ninf = np.float32(-np.inf)
    planted = [(lo32, 0), (np.nextafter(lo32, ninf), B), (hi32, B + 1),
               (np.nextafter(hi32, ninf), B - 1), (np.float32(np.inf), B + 1), (ninf, B),
               (np.float32(np.nan), B + 2), (-np.float32(np.nan), B + 2),
               (np.float32(1e-45), None), (np.float32(-1e-45), None),
               (np.float32(1.2e-38) / np.float32(4), None), (np.float32(-0.0), None)]
    for v, q in planted:  # the restatement itself, by hand
        if q is not None:
            assert hist_planes([v], B, lo, hi)[0] == q, (v, q)
    if lo == 0.0:  # -0.0 and the positive subnormal are in bin 0; the negative one is below
        assert list(hist_planes([-0.0, 1e-45, -1e-45], B, lo, hi)) == [0, 0, B]
    mid = np.float32(0.25 * lo + 0.75 * hi)
    a = np.full((16, 2, 12), mid, dtype=np.float32)
    rng = np.random.default_rng(B)
    pos = rng.permutation(a.size)[:3 * len(planted)]
    for n, p in enumerate(pos):  # each value three times, in blocks of its own
        a[np.unravel_index(p, a.shape)] = planted[n % len(planted)][0]
    assert np.signbit(a[np.isnan(a)]).any() and not np.signbit(a[np.isnan(a)]).all()
    g = check(eng, a, B, lo, hi, F, T)
    assert g[..., B + 2].sum() == 6                                   # NaNs of both signs
    assert g[..., B + 1].sum() == 6                                   # hi and +Inf
    below = 6 + (3 if lo == 0.0 else 0)                               # pred(lo), -Inf (and -1e-45)
    assert g[..., B].sum() == below
    assert g[..., B - 1].sum() >= 3                                   # pred(hi) is clamped


# ---- one hot bin ----------------------------------------------------------------------------
def test_hot_bin(eng):
    n = 512 * 160
    assert n > 65535
    a = np.full((512, 1, 160), 0.5, dtype=np.float32)
    for F, T in ((512, 160), (None, None)):
        g = check(eng, a, 64, 0.0, 1.0, F, T)
        assert g.shape == (1, 1, 1, 67) and g[0, 0, 0, 32] == n and g.sum() == n
    g = check(eng, a, 1, 0.0, 1.0, 512, 160)
    assert list(g[0, 0, 0]) == [n, 0, 0, 0]
    a[:] = np.nan
    g = check(eng, a, 64, 0.0, 1.0, 512, 160)
    assert g[0, 0, 0, 66] == n and g.sum() == n
    # ... and as the one hot bin of each of 512 channels (lanes own the channels)
    a[:] = 0.5
    g = check(eng, a, 64, 0.0, 1.0, 1, None)
    assert g.shape == (512, 1, 1, 67) and (g[..., 32] == 160).all()


# ---- bin counts -----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 256, 1000, 4096])
def test_bin_counts(eng, B):
    a = signed((96, 2, 40), B)
    x = put(eng, a)
    for F, T in ((96, 40), (8, 8), (1, 40), (3, 1)):
        check(eng, a, B, LO, HI, F, T, x=x)
    big = signed((512, 1, 200), B + 1)  # shared by workgroups at every B
    assert eng.histogram_plan(put(eng, big), B, LO, HI, 512, 200)["chunks_per_block"] >= 2
    check(eng, big, B, LO, HI, 512, 200)


# ---- blocks of one, many small blocks ------------------------------------------------------
def test_blocks_of_one(eng):
    a = signed((64, 2, 8), 3)
    g = check(eng, a, 16, LO, HI, 1, 1)
    assert g.shape == (64, 2, 8, 19) and (g.sum(axis=-1) == 1).all() and g.max() == 1


@pytest.mark.parametrize("shape", [(64, 2, 8), (1028, 3, 5)])
def test_many_small_blocks(eng, shape):
    a = signed(shape, 4)
    x = put(eng, a)
    for B in (64, 256):
        g = check(eng, a, B, LO, HI, 4, 1, x=x)
        assert g.shape == (shape[0] // 4, shape[1], shape[2], B + 3)


# ---- windows ----------------------------------------------------------------------------------
WINDOWS = {"channel_start_3": [3, 64, 1, 0, 3, 1, 0, 40, 1],
           "channel_step_2": [1, 32, 2, 0, 3, 1, 0, 40, 1],
           "reversed_time": [0, 64, 1, 0, 3, 1, 39, 40, -1],
           "two_ifs": [0, 64, 1, 1, 2, 1, 0, 40, 1],
           "reversed_channels_time_step_3": [66, 64, -1, 2, 2, -2, 2, 12, 3]}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows(eng, name):
    win = WINDOWS[name]
    a = signed((70, 3, 40), 5)
    x = put(eng, a)
    nc, nt = win[1], win[7]
    for F, T in ((8, 4), (nc, nt), (1, None), (None, None), (4, 1), (nc, 1), (1, 1)):
        check(eng, a, 64, LO, HI, F, T, win, x=x)


def test_window_of_a_split_block(eng):
    """Every form takes every window: the shared block with a channel start off
    the 16-byte grid, a channel step, and reversed time."""
    a = signed((530, 2, 1000), 6)
    x = put(eng, a)
    for win in ([3, 512, 1, 1, 1, 1, 999, 1000, -1], [1, 264, 2, 0, 2, 1, 0, 1000, 1]):
        p = eng.histogram_plan(x, 64, LO, HI, None, None, win)
        assert p["path"] == "block_split" and p["chunks_per_block"] >= 2
        check(eng, a, 64, LO, HI, None, None, win, x=x)
        p = eng.histogram_plan(x, 64, LO, HI, 1, None, win)
        assert p["path"] == "lanes_tsplit"
        check(eng, a, 64, LO, HI, 1, None, win, x=x)


# ---- a caller's out: strided, and holding anything ---------------------------------------------
@pytest.mark.parametrize("shape,F,T", [((64, 2, 48), 8, 16), ((512, 1, 200), 512, 200),
                                       ((64, 1, 4000), 1, 4000)])
def test_strided_poisoned_out(eng, shape, F, T):
    import torch

    B = 64
    a = signed(shape, 7)
    x = put(eng, a)
    want = histogram_ref(a, B, LO, HI, F, T)
    nco, ni, nto, K = want.shape
    # the middle third of a three-bank product, 0xFF everywhere beforehand
    big = torch.full((K, nto, ni, 3 * nco), -1, dtype=torch.int32, device="cuda:0").permute(3, 2, 1, 0)
    assert (eng.planes_to_numpy(big).view(np.uint32) == 0xFFFFFFFF).all()
    out = big[nco:2 * nco]
    got = eng.histogram(x, B, LO, HI, F, T, out=out)
    assert got.data_ptr() == out.data_ptr()
    h = eng.planes_to_numpy(big)
    assert np.array_equal(h[nco:2 * nco], want)
    assert (h[:nco] == -1).all() and (h[2 * nco:] == -1).all()
    # a dense poisoned out
    dense = eng.hist_empty(nco, ni, nto, K, device="cuda:0")
    dense.fill_(-1)
    eng.histogram(x, B, LO, HI, F, T, out=dense)
    assert np.array_equal(eng.planes_to_numpy(dense), want)


# ---- the band ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,T", [(8, 16), (64, 48), (1, 48), (1, 1)])
def test_band_is_the_vcat(eng, F, T):
    import torch

    banks = [signed((64, 2, 48), 20 + b) for b in range(3)]
    xs = [put(eng, a) for a in banks]
    got = eng.band_histogram(xs, 64, LO, HI, F, T)
    want = np.concatenate([histogram_ref(a, 64, LO, HI, F, T) for a in banks])
    assert got.dtype == torch.int32 and np.array_equal(eng.planes_to_numpy(got), want)
    singles = [eng.planes_to_numpy(eng.histogram(x, 64, LO, HI, F, T)) for x in xs]
    assert np.array_equal(eng.planes_to_numpy(got), np.concatenate(singles))
    if (F, T) == (64, 48):  # banks whose blocks are shared by workgroups
        big = [signed((512, 1, 200), 30 + b) for b in range(3)]
        got = eng.band_histogram([put(eng, a) for a in big], 64, LO, HI, None, None)
        want = np.concatenate([histogram_ref(a, 64, LO, HI, 512, 200) for a in big])
        assert np.array_equal(eng.planes_to_numpy(got), want)


# ---- the host entry point and the worker -----------------------------------------------------------
def test_host_entry_point(eng):
    a = np.asfortranarray(signed((40, 2, 12), 60))
    for win in (None, [3, 32, 1, 0, 2, 1, 11, 12, -1], [1, 16, 2, 1, 1, 1, 0, 12, 1]):
        w = window(a, win)
        for F, T in ((8, 4), (1, None), (None, None)):
            Fe, Te = F or w.shape[0], T or w.shape[2]
            r = eng.histogram_host(a, 64, LO, HI, F, T, win)
            assert r.flags.f_contiguous and r.dtype == np.int32
            assert np.array_equal(r, histogram_ref(w, 64, LO, HI, Fe, Te))


def test_worker_gethistogram(eng, pkg, tmp_path):
    import torch

    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = signed((64, 2, 40), 50)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=64), data)
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    x = put(eng, data)
    B = 100
    for src in (data, x, fil, raw):
        dev = isinstance(src, torch.Tensor)
        for F, T, Fe, Te in ((8, 4, 8, 4), (1, None, 1, 32), (None, None, 32, 32)):
            got = W.gethistogram(src, idxs, nbins=B, lo=LO, hi=HI, fqavby=F, tavby=T)
            assert sorted(got) == ["above", "below", "counts", "edges", "nan"]
            want = histogram_ref(window(data, win), B, LO, HI, Fe, Te)
            for k in ("counts", "below", "above", "nan"):
                assert isinstance(got[k], torch.Tensor if dev else np.ndarray), (k, type(got[k]))
                assert (got[k].is_cuda if dev else got[k].dtype == np.int32)
            host = (lambda t: t.cpu().numpy()) if dev else (lambda t: t)
            assert np.array_equal(host(got["counts"]), want[..., :B])
            assert np.array_equal(host(got["below"]), want[..., B])
            assert np.array_equal(host(got["above"]), want[..., B + 1])
            assert np.array_equal(host(got["nan"]), want[..., B + 2])
            assert np.array_equal(got["edges"], hist_edges_ref(B, LO, HI))
            if dev:  # views of the one output
                assert got["below"].data_ptr() > got["counts"].data_ptr()
    got = W.gethistogram(data, nbins=16, lo=LO, hi=HI)  # the defaults: a channel over all time
    assert got["counts"].shape == (64, 2, 1, 16)
    assert np.array_equal(got["counts"], histogram_ref(data, 16, LO, HI, 1, 40)[..., :16])
    parts = pkg.GBT.gethistogram([0, 0], [fil, raw], idxs, nbins=B, lo=LO, hi=HI, fqavby=8, tavby=4)
    assert len(parts) == 2
    for p in parts:
        assert np.array_equal(p["counts"], histogram_ref(window(data, win), B, LO, HI, 8, 4)[..., :B])
