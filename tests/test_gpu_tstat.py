"""GPU: tavfunc "median" / "var" / "std" over blocks of spectra
(csrc/tstats.hip) against Julia's Statistics restated in NumPy below.

median is compared bit for bit.  The restatement orders by the uint32 image of
the float (isless: -0.0 < 0.0), takes the middle element of an odd block and
a/2 + b/2 in Float32 of an even one, and gives NaN for a block holding a NaN.

var / std are compared with a Float64 two-pass oracle (ddof = 1) at
rtol = 1e-5, atol = 0: the project's Float32 bound (test_gpu_stats.py).  The
register form adds <= 32 Float32 terms in sequence (at most 32 * 2^-24 = 1.9e-6
relative on a sum of nonnegative terms, plus the rounding of the mean); the
split and chunked forms accumulate in Float64 and round once, so the same
bound holds at T = 65536."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu

RTOL = 1e-5
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


# ---------------------------------------------------------------------------
# Julia's rules in NumPy, along time

def window(a, win):
    if win is None:
        return a
    return a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1]) for k in range(3)])]


def tblocks(a, T, win=None):
    """(T, nc, ni, nb): block b holds the window's spectra b T .. b T + T - 1."""
    w = np.asfortranarray(window(a, win))
    nc, ni, nt = w.shape
    assert nt % T == 0
    return np.moveaxis(w.reshape((nc, ni, T, nt // T), order="F"), 2, 0)


def key32(x):
    u = np.ascontiguousarray(x).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def median_ref(a, T, win=None):
    R = tblocks(a, T, win)
    S = np.take_along_axis(R, np.argsort(key32(R), axis=0, kind="stable"), axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        r = S[T // 2] if T % 2 else S[T // 2 - 1] / np.float32(2) + S[T // 2] / np.float32(2)
    assert r.dtype == np.float32
    return np.asfortranarray(np.where(np.isnan(R).any(axis=0), np.float32(np.nan), r))


def var_ref(a, T, win=None, std=False):
    R = tblocks(a, T, win).astype(np.float64)
    m = R.sum(axis=0) / T
    v = ((R - m) ** 2).sum(axis=0) / (T - 1)
    return np.asfortranarray(np.sqrt(v) if std else v)


def test_restatement_rules():
    a = np.array([3e38, 3e38, 0.0, -0.0, -0.0, 0.0, 1.0, np.nan], np.float32).reshape((1, 1, 8))
    m = median_ref(a, 2)[0, 0]
    assert m.shape == (4,)
    assert m[0] == np.float32(3e38) and np.isnan(m[3]) and m[1] == 0 and not np.signbit(m[1])
    z = np.array([0.0, -0.0, -0.0], np.float32).reshape((1, 1, 3))
    assert np.signbit(median_ref(z, 3)[0, 0, 0])  # sorted -0, -0, 0
    s = np.array([1e-45, 1e-45], np.float32).reshape((1, 1, 2))
    assert median_ref(s, 2)[0, 0, 0] == 0  # a/2 + a/2 of the smallest subnormal
    b = np.arange(24, dtype=np.float32).reshape((2, 1, 12), order="F")  # [c, 0, t] = c + 2 t
    assert np.array_equal(median_ref(b, 4)[:, 0, :], [[3, 11, 19], [4, 12, 20]])
    assert np.array_equal(median_ref(b, 3, [1, 1, 1, 0, 1, 1, 11, 6, -2])[0, 0], [19, 7])
    np.testing.assert_allclose(var_ref(np.array([1, 2, 4, 7], np.float32).reshape((1, 1, 4)), 4),
                               np.var([1, 2, 4, 7], ddof=1))


# ---------------------------------------------------------------------------
# data

def ties(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).integers(0, 8, shape).astype(np.float32))


def specials(shape, T, seed):
    """Signed normals with some zeros and subnormals everywhere, and whole
    blocks (along time) of: a floatmax pair in the middle (the a/2 + b/2 rule),
    +-0.0 only, +-Inf and subnormals, one value; and one NaN."""
    rng = np.random.default_rng(seed)
    a = np.asfortranarray((rng.standard_normal(shape) * 1e3).astype(np.float32))
    small = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -2e-40], np.float32)
    hit = rng.random(shape) < 0.05
    a[hit] = rng.choice(small, int(hit.sum()))
    nc, ni, nt = shape
    R = a.reshape((nc, ni, T, nt // T), order="F")  # a view: [c, i, :, b] is a block
    assert np.shares_memory(R, a)
    where = [(c, i, b) for b in range(nt // T) for i in range(ni) for c in range(nc)]
    lo = (T - 2) // 2  # values below the pair
    pair = np.concatenate([np.sort(R[0, 0, :lo, 0]) - np.float32(1e6), np.float32([3e38, 3.3e38]),
                           np.full(T - 2 - lo, np.inf, np.float32)])
    fills = [rng.permutation(pair),
             rng.choice(np.float32([0.0, -0.0]), T),
             rng.choice(np.concatenate([small, np.float32([np.inf, -np.inf, FMAX, -FMAX])]), T),
             np.full(T, 1234.5, np.float32)]
    for (c, i, b), fill in zip(where[::-1], fills):
        R[c, i, :, b] = fill
    c, i, b = where[len(where) // 2]
    R[c, i, int(rng.integers(T)), b] = np.nan
    return a


def put(eng, a):
    return eng.fb_from_numpy(a, device="cuda:0")


REG_T = [2, 3, 4, 5, 8, 12, 16, 31, 32]
SPLIT_T = [33, 64, 100, 1024, 4096]


def shape_of(T):
    # float4 columns, a lane tail and several blocks; 72 channels = 3 tiles of the split median
    return (264, 2, 3 * T) if T <= 32 else (72, 2, 2 * T)


def path_of(T, op):
    return ("regs_" if T <= 32 else "split_") + ("median" if op == "median" else "moments")


# ---------------------------------------------------------------------------
# median, bit for bit

@pytest.mark.parametrize("T", REG_T + SPLIT_T)
def test_median_bits(eng, T):
    shape = shape_of(T)
    synth = eng.fb_to_numpy(eng.synth(*shape, nfpc=4, seed=T, kind=0, device="cuda:0"))
    for name, a in (("ties", ties(shape, T)), ("synth", synth), ("specials", specials(shape, T, T))):
        x = put(eng, a)
        plan = eng.tstat_plan(x, T, "median")
        assert plan["path"] == path_of(T, "median") and plan["channels_per_lane"] == 4, (T, plan)
        assert (plan["time_split_lanes"] > 1) == (T > 32)
        got = eng.fb_to_numpy(eng.tstat(x, T, "median"))
        want = median_ref(a, T)
        assert got.dtype == np.float32 and same_bits(got, want), (T, name)
        if name == "specials":
            assert np.isnan(want).sum() == 1
            if T % 2 == 0:  # the floatmax pair sits in the middle of its block
                assert np.isin(np.float32(3e38) / 2 + np.float32(3.3e38) / 2, want)


# ---------------------------------------------------------------------------
# var / std

@pytest.mark.parametrize("T", REG_T + SPLIT_T)
@pytest.mark.parametrize("kind", [0, 1])
def test_var_std(eng, T, kind):
    shape = shape_of(T)
    x = eng.synth(*shape, nfpc=4, seed=10 * T + kind, kind=kind, device="cuda:0")
    a = eng.fb_to_numpy(x)
    assert np.isfinite(a).all()
    assert eng.tstat_plan(x, T, "var")["path"] == path_of(T, "var")
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.tstat(x, T, op))
        want = var_ref(a, T, std=op == "std")
        err = np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)
        print(f"T={T} kind={kind} {op}: max rel err {err.max():.3g}")
        assert got.dtype == np.float32 and not np.isnan(got).any() and (got >= 0).all()
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


@pytest.fixture(scope="module")
def long_column(eng):
    x = eng.synth(8, 1, 65536, nfpc=4, seed=3, kind=0, device="cuda:0")
    return eng.fb_to_numpy(x), x


@pytest.mark.parametrize("T", [65536, 8192])
def test_long_column(eng, long_column, T):
    """(8, 1, 65536): the same bound at T = 65536, which a Float32 running sum
    would not keep."""
    a, x = long_column
    assert eng.tstat_plan(x, T, "var")["path"] == "chunk_moments"  # time chunks over workgroups
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.tstat(x, T, op))
        want = var_ref(a, T, std=op == "std")
        err = np.abs(got - want) / np.abs(want)
        print(f"T={T} {op}: max rel err {err.max():.3g}")
        assert not np.isnan(got).any() and (got >= 0).all()
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


@pytest.mark.parametrize("T", [2, 16, 33, 4096, 16384])
def test_constant_block_is_exactly_zero(eng, T):
    a = np.full((12, 2, 2 * T), 1e9, dtype=np.float32, order="F")
    a[:, 0, :T] = 3.0000001  # another constant, inexact in binary
    x = put(eng, a)
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.tstat(x, T, op))
        assert got.shape == (12, 2, 2)
        assert (got == 0).all() and not np.signbit(got).any(), (T, op)


@pytest.mark.parametrize("T", [16, 64])
def test_huge_finite_values_give_inf_not_nan(eng, T):
    a = np.full((8, 1, T), FMAX, dtype=np.float32, order="F")
    a[:, :, ::2] = np.float32(3e38)
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.tstat(put(eng, a), T, op))
        assert np.isposinf(got).all(), (T, op, got)


# ---------------------------------------------------------------------------
# windows

WIN_SHAPE = (203, 3, 40)
WINDOWS = {
    "c0=3": [3, 200, 1, 0, 3, 1, 0, 40, 1],
    "channel step 2": [1, 100, 2, 0, 3, 1, 0, 40, 1],
    "reversed channels": [202, 203, -1, 0, 3, 1, 0, 40, 1],
    "nc % 4 != 0": [0, 203, 1, 0, 3, 1, 0, 40, 1],
    "IF pick": [0, 200, 1, 1, 1, 1, 0, 40, 1],
    "time offset 1 step 2": [0, 200, 1, 0, 3, 1, 1, 20, 2],
    "negative time step": [0, 200, 1, 0, 3, 1, 39, 40, -1],
    "single channel": [7, 1, 1, 0, 3, 1, 0, 40, 1],
}
WIN_VEC = {"c0=3", "IF pick", "time offset 1 step 2", "negative time step"}  # float4 columns


@pytest.fixture(scope="module")
def win_data(eng):
    a = specials(WIN_SHAPE, 8, 99)
    # var / std: finite, of moderate size, and no subnormals (the variance of
    # two of them, ~1e-78, is below Float32's range: no relative bound applies)
    b = a.copy(order="F")
    b[~np.isfinite(b)] = 7.0
    b[np.abs(b) > 1e6] = -3.0
    b[np.abs(b) < 1e-30] = 0.5
    return a, put(eng, a), b, put(eng, b)


# T = 40: one block of the whole window, the split form
@pytest.mark.parametrize("T", [2, 5, 8, 20, 40])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows(eng, win_data, name, T):
    a, x, b, y = win_data
    w = WINDOWS[name]
    if w[7] % T:
        with pytest.raises(ValueError, match="DimensionMismatch"):
            eng.tstat(x, T, "median", w)
        return
    plan = eng.tstat_plan(x, T, "median", w)
    assert plan["channels_per_lane"] == (4 if name in WIN_VEC else 1), (name, plan)
    got = eng.fb_to_numpy(eng.tstat(x, T, "median", w))
    assert same_bits(got, median_ref(a, T, w)), (name, T)
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.tstat(y, T, op, w))
        want = var_ref(b, T, w, std=op == "std")
        assert got.dtype == np.float32 and got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=f"{name} {T} {op}")


# ---------------------------------------------------------------------------
# few columns, long T: the lanes of a workgroup split T

@pytest.mark.parametrize("T", [65536, 1024])
def test_few_columns_long_blocks(eng, T):
    x = eng.synth(4, 1, 65536, nfpc=4, seed=11, kind=0, device="cuda:0")
    a = eng.fb_to_numpy(x)
    for op in ("median", "std"):
        plan = eng.tstat_plan(x, T, op)
        assert plan["time_split_lanes"] == 256 and plan["channel_lanes"] == 1, plan
        if op == "std" and T == 65536:  # ... and time chunks split it over workgroups
            assert plan["path"] == "chunk_moments" and plan["workgroups"] == 16
        else:
            assert plan["path"] == path_of(T, op) and plan["workgroups"] == 65536 // T
    assert same_bits(eng.fb_to_numpy(eng.tstat(x, T, "median")), median_ref(a, T))
    np.testing.assert_allclose(eng.fb_to_numpy(eng.tstat(x, T, "std")), var_ref(a, T, std=True),
                               rtol=RTOL, atol=0)


def test_every_path_is_planned_for_a_shape_that_runs(eng, pkg):
    seen = set()
    for T in REG_T + SPLIT_T:  # test_median_bits, test_var_std
        x = eng.fb_empty(*shape_of(T), device="cuda:0")
        seen |= {eng.tstat_plan(x, T, op)["path"] for op in ("median", "var", "std")}
    x = eng.fb_empty(8, 1, 65536, device="cuda:0")  # test_long_column
    seen.add(eng.tstat_plan(x, 8192, "var")["path"])
    assert seen == set(pkg._lib.TSTAT_PATHS.values())
    assert eng.tstat_plan(x, 1, "median")["path"] == "copy"


# ---------------------------------------------------------------------------
# layers

def test_strided_out_into_a_slot(eng):
    import torch

    a = ties((64, 2, 48), 5)
    x = put(eng, a)
    for T, op in ((16, "median"), (48, "median"), (16, "var"), (1, "median")):
        want = eng.fb_to_numpy(eng.tstat(x, T, op))
        big = eng.fb_empty(3 * 64, 2, 48 // T, device="cuda:0")
        big.fill_(-7.0)
        slot = big[64:128]
        r = eng.tstat(x, T, op, out=slot)
        assert r is slot
        torch.cuda.synchronize()
        h = eng.fb_to_numpy(big)
        assert same_bits(h[64:128], want), (T, op)
        assert (h[:64] == -7.0).all() and (h[128:] == -7.0).all()


def test_chunked_moments_band_and_slot(eng):
    """The chunked form (T = 8192 of few columns) through the band entry point
    and into a strided slot: the bits of the per-bank dense calls."""
    banks = [eng.synth(12, 2, 16384, nfpc=4, seed=40 + k, kind=0, device="cuda:0") for k in (0, 1)]
    assert eng.tstat_plan(banks[0], 8192, "std")["path"] == "chunk_moments"
    parts = [eng.fb_to_numpy(eng.tstat(x, 8192, "std")) for x in banks]
    np.testing.assert_allclose(parts[1], var_ref(eng.fb_to_numpy(banks[1]), 8192, std=True),
                               rtol=RTOL, atol=0)
    band = eng.fb_to_numpy(eng.band_tstat(banks, 8192, "std"))
    assert same_bits(band, np.concatenate(parts, axis=0))
    big = eng.fb_empty(36, 2, 2, device="cuda:0")
    big.fill_(-7.0)
    eng.tstat(banks[0], 8192, "std", out=big[12:24])
    h = eng.fb_to_numpy(big)
    assert same_bits(h[12:24], parts[0]) and (h[:12] == -7.0).all() and (h[24:] == -7.0).all()


def test_band_tstat_is_the_concatenation(eng):
    banks = [specials((72, 2, 128), 64, 20), specials((72, 2, 128), 64, 21)]
    xs = [put(eng, b) for b in banks]
    for T, op in ((16, "median"), (64, "median"), (16, "var"), (64, "std")):
        band = eng.fb_to_numpy(eng.band_tstat(xs, T, op))
        parts = [eng.fb_to_numpy(eng.tstat(x, T, op)) for x in xs]
        assert same_bits(band, np.concatenate(parts, axis=0)), (T, op)
        if op == "median":
            assert same_bits(parts[1], median_ref(banks[1], T))


def test_tstat_host_matches_device(eng):
    a = np.asfortranarray(np.random.default_rng(8).gamma(2.0, 5e8, (200, 2, 96)).astype(np.float32))
    x = put(eng, a)
    for T, op in ((16, "std"), (96, "std"), (16, "median"), (48, "median")):
        host = eng.tstat_host(a, T, op)  # a pageable host array
        assert host.dtype == np.float32
        assert same_bits(host, eng.fb_to_numpy(eng.tstat(x, T, op))), (T, op)
    win = [5, 100, 1, 1, 1, 1, 95, 48, -2]  # a reversed time range: staged reversed
    assert same_bits(eng.tstat_host(a, 16, "median", win), median_ref(a, 16, win))
    np.testing.assert_allclose(eng.tstat_host(a, 16, "std", win), var_ref(a, 16, win, std=True),
                               rtol=RTOL, atol=0)


def test_bad_out_raises_before_any_launch(eng, pkg):
    import torch

    x = put(eng, ties((64, 2, 32), 1))
    good = eng.fb_empty(64, 2, 2, device="cuda:0")
    good.fill_(-1.0)
    bad = [torch.empty((2, 2, 64), dtype=torch.float64, device="cuda:0").permute(2, 1, 0),
           eng.fb_empty(64, 2, 4, device="cuda:0"),
           torch.empty((64, 2, 2), dtype=torch.float32, device="cuda:0"),  # row-major
           torch.empty((2, 2, 64), dtype=torch.float32, device="cpu").permute(2, 1, 0)]
    for out in bad:
        with pytest.raises((TypeError, ValueError)):
            eng.tstat(x, 16, "median", out=out)
    with pytest.raises(pkg._lib.ArgumentError, match="reduce"):
        eng.tstat(x, 16, "sum")
    with pytest.raises(ValueError, match="DimensionMismatch"):
        eng.tstat(x, 5, "median")
    with pytest.raises(IndexError):
        eng.tstat(x, 2, "median", [0, 65, 1, 0, 2, 1, 0, 32, 1])
    # overlapping strides are refused by the ABI itself
    L = pkg._lib.lib()
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    rc = L.bldp_tstat_f32(ptr, nchan, nif, ntime, None, 16, 6, good.data_ptr(), 63, 128,
                          pkg._lib.stream_ptr())
    assert rc == pkg._lib.BLDP_EINVAL and "overlap" in pkg._lib.last_error()
    torch.cuda.synchronize()
    assert (good == -1.0).all()


def test_two_stage_getdata(eng, pkg):
    import torch

    W = pkg.worker
    a = ties((256, 2, 24), 3)
    x = put(eng, a)
    stage1 = eng.fb_to_numpy(eng.reduce(x, 8, 1, "sum"))
    r = W.getdata(x, fqavby=8, fqavfunc="sum", tavby=4, tavfunc="median")
    assert isinstance(r, torch.Tensor) and r.is_cuda
    assert same_bits(eng.fb_to_numpy(r), median_ref(stage1, 4))
    assert same_bits(W.getdata(a, fqavby=8, fqavfunc="sum", tavby=4, tavfunc="median"),
                     median_ref(stage1, 4))
    two = eng.fb_to_numpy(eng.reduce(eng.reduce(x, 8, 1, "sum"), 1, 4, "max"))
    assert same_bits(eng.fb_to_numpy(W.getdata(x, fqavby=8, fqavfunc="sum", tavby=4,
                                               tavfunc="max")), two)
    # a stat op in stage 1, and stage 2 skipped
    med1 = eng.fb_to_numpy(eng.reduce(x, 8, 1, "median"))
    assert same_bits(W.getdata(a, fqavby=8, fqavfunc="median", tavby=4, tavfunc="std"),
                     eng.fb_to_numpy(eng.tstat(put(eng, med1), 4, "std")))
    assert same_bits(W.getdata(a, fqavby=8, fqavfunc="median", tavby=1, tavfunc="std"), med1)
    # tavfunc=None: today's result, today's error
    assert same_bits(W.getdata(a, fqavby=8, tavby=4, tavfunc=None), W.getdata(a, fqavby=8, tavby=4))
    with pytest.raises(TypeError, match="tavby"):
        W.getdata(a, fqavby=8, fqavfunc="median", tavby=4)


def test_getdata_files_and_getband(eng, pkg, orc, tmp_path):
    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = specials((64, 2, 40), 8, 4)
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
        got = W.getdata(src, tavby=8, tavfunc="median")
        assert got.dtype == np.float32 and same_bits(got, median_ref(data, 8)), src
        assert same_bits(W.getdata(src, idxs, tavby=16, tavfunc="median"),
                         median_ref(data, 16, win)), src
    s1 = eng.fb_to_numpy(eng.reduce(put(eng, data), 4, 1, "max"))
    want = median_ref(s1, 8)
    for src in (fil, raw, bs):
        assert same_bits(W.getdata(src, fqavby=4, fqavfunc="max", tavby=8, tavfunc="median"), want)
    band = pkg.GBT.getband([0, 0], [fil, raw], fqavby=4, fqavfunc="max", tavby=8,
                           tavfunc="median")
    assert same_bits(band, np.concatenate([want, want], axis=0))
    parts = pkg.GBT.getdata([0, 0], [fil, bs], tavby=8, tavfunc="median")
    assert all(same_bits(p, median_ref(data, 8)) for p in parts)
    staged = pkg.GBT.getband([0, 0], [fil, bs], tavby=8, tavfunc="median", staged=True)
    assert same_bits(staged, np.concatenate([median_ref(data, 8)] * 2, axis=0))


def test_two_host_threads_give_the_single_thread_bits(eng):
    rng = np.random.default_rng(32)
    arrs = [np.asfortranarray(rng.gamma(2.0, 5e8, (96, 1, 128 + 64 * k)).astype(np.float32))
            for k in range(2)]
    jobs = [(a, T, op) for a in arrs for T, op in ((16, "median"), (64, "median"), (64, "std"))]
    single = [eng.tstat_host(a, T, op) for a, T, op in jobs]
    with ThreadPoolExecutor(2) as ex:
        both = list(ex.map(lambda j: eng.tstat_host(*j), jobs * 2))
    for got, want in zip(both, single * 2):
        assert same_bits(got, want)
