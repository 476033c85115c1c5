"""GPU: outliers (the median's kernels of csrc/stats.hip and csrc/tstats.hip with
SEL_OUTLIERS) against the rule restated in NumPy (outliers_ref.py), bit for
bit: every step of the rule is exactly specified, so no tolerance applies.
NaN planes compare as NaN (conftest.same_bits).

Every block size is run on data with whole blocks planted with: a NaN, a
minority, exactly half and a majority of +Inf, +-floatmax (the differences
overflow), subnormals with odd significands, +-0.0, one value, and the integers
0..3 (heavy ties); the planting is test_gpu_mad.py's, restated here."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits
from mad_ref import blocks, mad_ref, median_ref
from outliers_ref import outlier_blocks, outliers_ref

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NPLANT = 10
NSIGMAS = (0.0, 3.0, 5.0, 1e300)
KEYS = ("median", "mad", "count", "mask")


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def put(eng, a):
    return eng.fb_from_numpy(a, device="cuda:0")


# ---------------------------------------------------------------------------
# data: B blocks of n values as the columns of an (n, B) matrix

def make_blocks(n, B, seed):
    assert B >= NPLANT
    rng = np.random.default_rng(seed)
    M = rng.gamma(2.0, 5e8, (n, B)).astype(np.float32)
    M[:, 1::2] = (rng.standard_normal((n, (B + 0) // 2)) * 1e3).astype(np.float32)

    def some(k):  # k places of a block
        return rng.permutation(n)[:k]

    j = iter(range(B - 1, -1, -1))  # planted from the last block down
    M[some(1), next(j)] = np.nan
    M[some((n - 1) // 2), next(j)] = np.inf  # a minority: finite
    M[some(n // 2), next(j)] = np.inf        # half (even n): the median is Inf, Inf - Inf
    M[some(n // 2 + 1), next(j)] = np.inf    # a majority: NaN
    M[:, next(j)] = rng.permutation(np.where(np.arange(n) % 2, FMAX, -FMAX).astype(np.float32))
    M[:, next(j)] = rng.permutation(np.resize(np.float32([FMAX, FMAX, 3e38, 1.0]), n))
    sub = (2 * rng.integers(0, 1 << 22, n) + 1).astype(np.uint32)  # odd significands
    sub |= rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    M[:, next(j)] = sub.view(np.float32)
    M[:, next(j)] = rng.choice(np.float32([0.0, -0.0]), n)
    M[:, next(j)] = np.float32(1234.5)
    M[:, next(j)] = rng.integers(0, 4, n).astype(np.float32)
    return M


def chan_array(F, nco, ni, nt, seed):
    """(F * nco, ni, nt): the blocks along the channels."""
    M = make_blocks(F, nco * ni * nt, seed)
    return np.asfortranarray(M.reshape((F * nco, ni, nt), order="F"))


def time_array(T, nc, ni, nb, seed):
    """(nc, ni, T * nb): the blocks along time."""
    M = make_blocks(T, nc * ni * nb, seed).reshape((T, nb, nc, ni), order="F")
    return np.asfortranarray(np.transpose(M, (2, 3, 1, 0)).reshape((nc, ni, nb * T)))


SORT_F = [2, 3, 4, 5, 63, 64]
SELECT_F = [65, 100, 4096]
STREAM_F = [4097, 8192]
PATH_OF = {**{F: "median_sort" for F in SORT_F}, **{F: "median_select" for F in SELECT_F},
           **{F: "median_stream" for F in STREAM_F}}
REGS_T = [2, 3, 16, 31, 32]
SPLIT_T = [33, 34, 100, 1024]


def chan_shape(F):
    nco = max(2, min(512, 32768 // F))  # >= 24 blocks, <= 3072; 200k values at most
    return F, nco, 2, 3


def chan_windows(F, nco):
    nch = F * nco
    rest = [0, 2, 1, 0, 3, 1]
    return [None,                                    # float4 loads where 4 divides F
            [0, F * (nco // 2), 2] + rest,           # channel step 2: one dword per element
            [nch - 1, nch, -1] + rest,               # reversed
            [3, F * (nco - 2), 1] + rest]            # from channel 3: off a 16-byte boundary


def time_shape(T, nc):
    return T, nc, 2, max(8, min(128, 8192 // T))


# ---------------------------------------------------------------------------
# what keeps a test from passing on an empty case, asserted on the restatement

def check_conditions(a, n, axis):
    R = blocks(a, n, None, axis).reshape((n, -1), order="F")
    c, s, thr, d, f = outlier_blocks(R, 3.0)
    cnt = f.sum(axis=0)
    if n >= 3:
        assert ((cnt > 0) & (cnt < n)).any(), n  # some block is partly flagged
    assert ((d == thr[None]) & ~f).any(), n  # the unflagged tie d_i == thr
    assert (np.isnan(c) & np.isnan(s) & (cnt == 0)).sum() >= 1
    assert (np.isnan(s) & (cnt == 0)).sum() >= 2  # NaN planes, nothing flagged
    c, s, thr, d, f = outlier_blocks(R, 0.0)
    ok = ~np.isnan(s) & (thr == 0)
    same = (R == c[None]).sum(axis=0)
    assert (ok & (f.sum(axis=0) == n - same) & (same < n)).any(), n


def test_conditions_on_the_restatement():
    for F in SORT_F + SELECT_F + STREAM_F:
        _, nco, ni, nt = chan_shape(F)
        assert nco * ni * nt >= 24
        check_conditions(chan_array(F, nco, ni, nt, F), F, 0)
    for T in REGS_T + SPLIT_T:
        for nc in (8, 6):
            _, _, ni, nb = time_shape(T, nc)
            check_conditions(time_array(T, nc, ni, nb, 100 * T + nc), T, 2)


# ---------------------------------------------------------------------------
# calls

def host(eng, r):
    return {k: eng.fb_to_numpy(t) for k, t in r.items()}


def run(eng, x, n, axis, nsigma, win=None, mask=True, which=KEYS[:3]):
    return host(eng, eng.outliers(x, n, axis=axis, nsigma=nsigma, win=win, mask=mask, which=which))


def matches(got, want):
    """A dict of results against outliers_ref's tuple, bit for bit."""
    med, mad, count, mask = want
    assert got["median"].dtype == got["mad"].dtype == np.float32
    assert got["count"].dtype == np.int32 and got["mask"].dtype == np.uint8
    return (same_bits(got["median"], med) and same_bits(got["mad"], mad) and
            np.array_equal(got["count"], count.astype(np.int32)) and
            np.array_equal(got["mask"], mask))


def same_results(a, b):
    assert set(a) == set(b)
    return all(same_bits(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k])
               for k in a)


def block_sums(mask, n, axis):
    return np.moveaxis(blocks(mask.astype(np.int32), n, None, axis).sum(axis=0), 0, axis)


def raw_call(pkg, x, n, axis, nsigma, med, mad, count, mask_ptr, ld_i, ld_t):
    """bldp_outliers_f32 itself: strided planes and a caller's mask address."""
    eng = pkg.engine
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    keep, wp = pkg._lib.win_arg(eng._full_win(None, tuple(x.shape)))
    rc = pkg._lib.lib().bldp_outliers_f32(ptr, nchan, nif, ntime, wp, axis, n, nsigma,
                                          *[None if t is None else t.data_ptr()
                                            for t in (med, mad, count)], mask_ptr, ld_i, ld_t, None)
    pkg._lib.check(rc, "bldp_outliers_f32")


def check_everything(eng, pkg, a, n, axis, windows, others):
    """Every check of one shape: a is the array, others two more banks of its shape."""
    import torch

    x = put(eng, a)
    whole = {}
    for ns in NSIGMAS:
        for w in windows:
            got = run(eng, x, n, axis, ns, w)
            assert matches(got, outliers_ref(a, n, ns, w, axis)), (n, axis, ns, w)
            assert np.array_equal(block_sums(got["mask"], n, axis), got["count"]), (n, ns, w)
            if w is None:
                whole[ns] = got
    assert same_bits(eng.fb_to_numpy(x), a)  # the input is read only
    # the planes are the statistics' own bits on the same tensor
    if axis == 0:
        med, mad = eng.reduce(x, n, 1, "median"), eng.reduce(x, n, 1, "mad")
    else:
        med, mad = eng.tstat(x, n, "median"), eng.tstat(x, n, "mad")
    assert same_bits(whole[3.0]["median"], eng.fb_to_numpy(med))
    assert same_bits(whole[3.0]["mad"], eng.fb_to_numpy(mad))
    assert same_bits(whole[3.0]["median"], median_ref(a, n, axis=axis))
    assert same_bits(whole[3.0]["mad"], mad_ref(a, n, axis=axis))
    assert whole[3.0]["count"].sum() < whole[0.0]["count"].sum()
    assert n == 2 or whole[3.0]["count"].sum() > 0  # (two values are never 3 sigmas apart)
    # (thr = +Inf flags nothing; where s == 0 the threshold is 0 whatever nsigma is)
    assert (whole[1e300]["count"][whole[1e300]["mad"] != 0] == 0).all()
    assert (whole[1e300]["count"] <= whole[5.0]["count"]).all()
    # any subset of the outputs null
    ref = whole[3.0]
    for which, mask in ((("count",), False), ((), True), (("median",), True),
                        (("mad", "count"), False), (("median", "mad"), False)):
        got = run(eng, x, n, axis, 3.0, None, mask, which)
        assert set(got) == set(which) | ({"mask"} if mask else set())
        assert same_results(got, {k: ref[k] for k in got}), (n, axis, which, mask)
    # strided planes: the middle slot of a three-bank product, and a mask between guards
    d0, d1, d2 = ref["count"].shape
    bigs = [eng.fb_empty(3 * d0, d1, d2, device="cuda:0", dtype=dt)
            for dt in (torch.float32, torch.float32, torch.int32)]
    for b in bigs:
        b.fill_(-7)
    nm = a.size
    for guard in (64, 61):  # (61: no dword of the mask is aligned)
        buf = torch.full((nm + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda:0")
        raw_call(pkg, x, n, axis, 3.0, *[b[d0:2 * d0] for b in bigs], buf.data_ptr() + guard,
                 3 * d0, 3 * d0 * d1)
        torch.cuda.synchronize()
        for b, k in zip(bigs, KEYS):
            h = eng.fb_to_numpy(b)
            assert (h[:d0] == -7).all() and (h[2 * d0:] == -7).all(), (n, axis, k)
            mid = h[d0:2 * d0]
            assert same_bits(mid, ref[k]) if k != "count" else np.array_equal(mid, ref[k])
        hb = buf.cpu().numpy()
        assert (hb[:guard] == 0xAB).all() and (hb[guard + nm:] == 0xAB).all(), (n, axis, guard)
        assert np.array_equal(hb[guard:guard + nm], ref["mask"].ravel(order="F")), (n, axis, guard)
    # a band of three banks is the banks' results one after the other
    band = host(eng, eng.band_outliers([x] + [put(eng, b) for b in others], n, axis=axis,
                                       nsigma=3.0, mask=True))
    parts = [ref] + [run(eng, put(eng, b), n, axis, 3.0) for b in others]
    assert same_results(band, {k: np.concatenate([p[k] for p in parts], axis=0) for k in KEYS})
    # a pageable host array through the GPU
    for ns in (3.0, 0.0):
        got = eng.outliers_host(a, n, axis=axis, nsigma=ns, mask=True)
        assert all(v.flags.f_contiguous for v in got.values())
        assert same_results(got, whole[ns]), (n, axis, ns)
    w = windows[-1]
    got = eng.outliers_host(a, n, axis=axis, nsigma=3.0, win=w, mask=True)
    assert matches(got, outliers_ref(a, n, 3.0, w, axis))
    # permuting every block permutes the mask and nothing else
    L = a.shape[axis]
    rng = np.random.default_rng(n + 1)
    idx = (np.arange(L) // n) * n + np.tile(rng.permutation(n), L // n)
    got = run(eng, put(eng, np.asfortranarray(np.take(a, idx, axis=axis))), n, axis, 3.0)
    assert same_results({k: got[k] for k in KEYS[:3]}, {k: ref[k] for k in KEYS[:3]})
    assert np.array_equal(got["mask"], np.take(ref["mask"], idx, axis=axis))
    # an exact scaling (a power of two; finite data that stay normal) keeps the flags
    rng = np.random.default_rng(n + 2)
    g = rng.gamma(2.0, 5e8, a.shape).astype(np.float32)
    g[rng.random(a.shape) < 0.02] *= np.float32(64)
    g = np.asfortranarray(g)
    base = run(eng, put(eng, g), n, axis, 3.0)
    assert matches(base, outliers_ref(g, n, 3.0, None, axis))
    assert base["count"].sum() < g.size and (n == 2 or base["count"].sum() > 0)
    for k in (-100, 30, 80):
        s = run(eng, put(eng, np.asfortranarray(np.ldexp(g, k))), n, axis, 3.0)
        assert np.array_equal(s["count"], base["count"]), (n, axis, k)
        assert np.array_equal(s["mask"], base["mask"]), (n, axis, k)
        assert same_bits(s["mad"], np.ldexp(base["mad"], k))


# ---------------------------------------------------------------------------
# the channel axis, every form

@pytest.mark.parametrize("F", SORT_F + SELECT_F + STREAM_F)
def test_fqav_outliers_bits(eng, pkg, F):
    _, nco, ni, nt = chan_shape(F)
    a = chan_array(F, nco, ni, nt, F)
    x = put(eng, a)
    for mask in (False, True):
        plan = eng.outliers_plan(x, F, axis=0, mask=mask)
        reads = 9 if F > 4096 else 2 if mask else 1
        assert plan["path"] == PATH_OF[F] and plan["reads"] == reads and plan["mask"] == mask
        assert plan["float4_per_lane"] == (1 if F % 4 == 0 else 0)
        mad = eng.plan(x, F, 1, "mad")
        assert {k: v for k, v in plan.items() if k not in ("reads", "mask")} == mad
    others = [chan_array(F, nco, ni, nt, F + 1), np.asfortranarray(a[:, ::-1, ::-1])]
    check_everything(eng, pkg, a, F, 0, chan_windows(F, nco), others)


# ---------------------------------------------------------------------------
# the time axis, both forms

@pytest.mark.parametrize("nc", [8, 6])  # float4 columns, and one dword per lane
@pytest.mark.parametrize("T", REGS_T + SPLIT_T)
def test_tav_outliers_bits(eng, pkg, T, nc):
    _, _, ni, nb = time_shape(T, nc)
    a = time_array(T, nc, ni, nb, 100 * T + nc)
    x = put(eng, a)
    for mask in (False, True):
        plan = eng.outliers_plan(x, T, axis=2, mask=mask)
        reads = (1 + mask) if T <= 32 else (9 if T % 2 else 11)
        assert plan["path"] == ("regs_median" if T <= 32 else "split_median")
        assert plan["reads"] == reads and plan["mask"] == mask, (T, nc, plan)
        assert plan["channels_per_lane"] == (4 if nc == 8 else 1)
        mad = eng.tstat_plan(x, T, "mad")
        assert {k: v for k, v in plan.items() if k not in ("reads", "mask")} == mad
    # a window: channels reversed (dword loads), the spectra of half the blocks from the second
    w = [nc - 1, nc, -1, 0, ni, 1, T, T * (nb // 2), 1]
    others = [time_array(T, nc, ni, nb, 100 * T + nc + 1), np.asfortranarray(a[::-1])]
    check_everything(eng, pkg, a, T, 2, [None, w], others)


# ---------------------------------------------------------------------------
# the rule's special cases

def test_special_cases(eng):
    inf, nan = np.inf, np.nan
    rows = np.float32([[7, 7, 9, 7], [0, 1, 3, 100], [1, nan, 3, 50], [inf, inf, 1, inf],
                       [-inf, 0, 5, inf], [0.0, -0.0, -0.0, 0.0], [-FMAX, FMAX, FMAX, -FMAX],
                       [1, 2, 4, 7]])
    a = np.asfortranarray(rows.reshape((32, 1, 1)))
    t = np.asfortranarray(rows.reshape((8, 1, 4)))
    for x, axis in ((put(eng, a), 0), (put(eng, t), 2)):
        src = a if axis == 0 else t
        for ns in NSIGMAS + (-0.0, 1.0, 2.5):
            got = run(eng, x, 4, axis, ns)
            assert matches(got, outliers_ref(src, 4, ns, None, axis)), (axis, ns)
        c = run(eng, x, 4, axis, 5.0)["count"].ravel()
        assert c.tolist()[:4] == [1, 1, 0, 0]  # s = 0 flags the spike; NaN blocks flag nothing
        c0 = run(eng, x, 4, axis, 0.0)["count"].ravel()
        # [-Inf, 0, 5, Inf]: c = 2.5, s = Inf, 0 * Inf is NaN: nothing; +-0.0 all equal the median
        assert c0.tolist() == [1, 4, 0, 0, 0, 0, 0, 4]  # (+-floatmax: s = Inf again)
        assert run(eng, x, 4, axis, -0.0)["count"].ravel().tolist() == c0.tolist()


# ---------------------------------------------------------------------------
# layers

def test_engine_layers(eng, pkg):
    import torch

    a = chan_array(8, 8, 2, 12, 5)  # (64, 2, 12)
    x = put(eng, a)
    for axis, n, dims in ((0, 8, (8, 2, 12)), (2, 4, (64, 2, 3)), (2, None, (64, 2, 1))):
        r = eng.outliers(x, n, axis=axis, mask=True)
        assert list(r) == ["median", "mad", "count", "mask"]
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in r.values())
        assert r["median"].dtype == r["mad"].dtype == torch.float32
        assert r["count"].dtype == torch.int32 and r["mask"].dtype == torch.uint8
        assert all(tuple(r[k].shape) == dims for k in KEYS[:3])
        assert tuple(r["mask"].shape) == (64, 2, 12)
        assert matches(host(eng, r), outliers_ref(a, n or 12, 5.0, None, axis))
        assert list(eng.outliers(x, n, axis=axis)) == ["median", "mad", "count"]
        b = eng.band_outliers([x, x], n, axis=axis, mask=True)
        assert tuple(b["count"].shape) == (2 * dims[0],) + dims[1:]
        assert tuple(b["mask"].shape) == (128, 2, 12) and b["count"].dtype == torch.int32
    w = pkg.worker.getoutliers(x, n=4, mask=True)  # a device tensor stays on the device
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in w.values())
    assert matches(host(eng, w), outliers_ref(a, 4, 5.0, None, 2))
    h = pkg.worker.getoutliers(a, (pkg.JRange(5, 36), pkg.COLON, pkg.COLON), n=16, axis=0,
                               nsigma=3.0, mask=True)  # a host array goes through the GPU
    assert all(isinstance(v, np.ndarray) for v in h.values())
    assert matches(h, outliers_ref(a, 16, 3.0, [4, 32, 1, 0, 2, 1, 0, 12, 1], 0))
    with pytest.raises(TypeError, match="outliers takes Float32"):
        eng.outliers(x.to(torch.int16), 4)
    with pytest.raises(TypeError, match="outliers takes Float32"):
        pkg.worker.getoutliers(x.to(torch.float64), n=4)
    with pytest.raises(pkg._lib.ArgumentError):
        eng.outliers(x, 1)


def test_getoutliers_files_and_fan_out(eng, pkg, orc, tmp_path):
    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = chan_array(8, 8, 2, 40, 4)  # (64, 2, 40)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    bs = str(tmp_path / "bs.rawspec.0002.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=64), data)
    pkg.fbh5.write_bslz4(bs, dict(foff=-1.0, nfpc=64), data, (8, 1, 64),
                         lambda blk: orc.np_bslz4_encode(blk, 512, lz4=orc.lz4_compress))
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    for src in (fil, raw, bs):
        got = W.getoutliers(src, mask=True)  # n=None: the whole time range
        assert all(isinstance(v, np.ndarray) for v in got.values())
        assert matches(got, outliers_ref(data, 40, 5.0, None, 2)), src
        got = W.getoutliers(src, idxs, n=16, nsigma=3.0, mask=True)
        assert matches(got, outliers_ref(data, 16, 3.0, win, 2)), src
        got = W.getoutliers(src, idxs, n=8, axis=0, nsigma=3.0, mask=True)
        assert matches(got, outliers_ref(data, 8, 3.0, win, 0)), src
        assert list(W.getoutliers(src, n=8)) == ["median", "mad", "count"]
    parts = pkg.GBT.getoutliers([0, 0], [fil, bs], idxs, n=16, nsigma=3.0, mask=True)
    assert len(parts) == 2
    for p in parts:
        assert matches(p, outliers_ref(data, 16, 3.0, win, 2))
