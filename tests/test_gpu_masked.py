"""GPU: the masked reduce (csrc/masked.hip) against the NumPy restatement of its
rule (masked_ref.py), on every form of the walk and of the mask stream.

Integer-valued data in 0 .. 255: while 255 * F * T < 2^24 every partial sum is an
exact Float32, so ``data`` equals the reference in any order of the adds, and
the mean is the Float32 quotient bit for bit.  Gamma data: within RTOL = 1e-5 of
the Float64 sum (the bound of test_gpu_parity.py for Float32 sums; the data is
positive).  ``kept`` is always exact.  NaN, +Inf and -Inf lie under every flag,
so each result also shows that a flagged sample never reaches the sum."""
from __future__ import annotations

import numpy as np
import pytest

from mad_ref import window
from masked_ref import masked_ref
from outliers_ref import outliers_ref

pytestmark = pytest.mark.gpu

RTOL = 1e-5
POISON = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
LANES_F = [1, 2, 3, 4, 5, 8, 63, 64, 65, 100, 256, 1024]
LANES_T = [1, 2, 3, 5, 15, 16, 17, 33]
BLOCK_F = [1028, 2048, 4097]


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def put(eng, a):
    return eng.fb_from_numpy(np.asfortranarray(a), device="cuda:0")


def dmask(m, odd=False):
    """A host mask on the device with channel-fastest strides; ``odd``: as a view
    one byte into a larger byte tensor."""
    import torch

    m = np.asarray(m)
    if m.dtype == np.bool_:
        t = torch.from_numpy(np.asfortranarray(m)).to("cuda:0")
        assert t.dtype == torch.bool
        return t
    if not odd:
        t = torch.from_numpy(np.asfortranarray(m)).to("cuda:0")
        assert t.stride()[0] == 1 or m.shape[0] == 1
        return t
    nc, ni, nt = m.shape
    buf = torch.zeros(m.size + 1, dtype=torch.uint8, device="cuda:0")
    buf[1:] = torch.from_numpy(m.ravel(order="F").copy()).to("cuda:0")
    v = torch.as_strided(buf, (nc, ni, nt), (1, nc, nc * ni), storage_offset=1)
    assert v.data_ptr() % 2 == 1
    return v


def int_data(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.float32)


def gamma_data(shape, seed):
    return np.random.default_rng(seed).gamma(2.0, 50.0, shape).astype(np.float32)


def view(a, win):
    """The window of ``a`` as a view (mad_ref.window copies)."""
    if win is None:
        return a
    sl = []
    for k in range(3):
        st, ct, sp = win[3 * k: 3 * k + 3]
        stop = st + ct * sp
        sl.append(slice(st, stop if stop >= 0 else None, sp))
    return a[tuple(sl)]


def poison(a, win, m):
    """A copy of ``a`` with NaN, +Inf and -Inf under every flag of the window."""
    a = a.copy()
    w = view(a, win)
    f = np.broadcast_to(np.asarray(m) != 0, w.shape)
    w[f] = POISON[np.arange(int(f.sum())) % 3]
    return a


def masks(shape, F, T, seed):
    """name -> host mask, over a window of ``shape`` with >= 3 blocks along the channels."""
    nc, ni, nt = shape
    rng = np.random.default_rng(seed)
    vals = np.array([1, 2, 255], dtype=np.uint8)

    def rand(shp, p=0.3):
        return np.where(rng.random(shp) < p, vals[rng.integers(0, 3, shp)], 0).astype(np.uint8)

    out = {"zero": np.zeros(shape, np.uint8), "all": vals[rng.integers(0, 3, shape)],
           "random": rand(shape), "odd_address": rand(shape)}
    one = np.zeros(shape, np.uint8)
    one[F:2 * F, 0, :T] = 1  # block (1, 0, 0) between unflagged neighbours
    out["one_block"] = one
    first = np.full(shape, 2, np.uint8)
    first[::F, :, ::T] = 0   # only sample (0, 0) of every block kept
    last = np.full(shape, 255, np.uint8)
    last[F - 1::F, :, T - 1::T] = 0
    out["first_kept"], out["last_kept"] = first, last
    out["bad_channels"] = rand((nc, 1, 1))
    out["bad_spectra"] = rand((1, 1, nt))
    out["bad_ifs"] = np.array([0, 1], np.uint8)[:ni].reshape(1, ni, 1)
    out["bool"] = rand(shape) != 0
    return out


def same(got, want):
    """Values equal, NaN where NaN is wanted (+0 and -0 are equal)."""
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def close(got, s):
    nan = np.isnan(s)
    return (got.shape == s.shape and np.array_equal(np.isnan(got), nan) and
            bool(np.all(np.abs(got[~nan].astype(np.float64) - s[~nan]) <= RTOL * np.abs(s[~nan]))))


def check(eng, a, m, F, T, win=None, exact=True, odd=False, ops=("sum", "mean"), poisoned=True):
    """One window and one mask on the GPU against the restatement; returns the plan."""
    ap = poison(a, win, m) if poisoned else a
    x, md = put(eng, ap), dmask(m, odd)
    s, k, mean = masked_ref(window(ap, win), m, F, T)
    assert 255 * max(F, 1) * max(T, 1) < 2 ** 24 or not exact
    for op in ops:
        r = eng.masked_reduce(x, md, F, T, op, win)
        data, kept = eng.fb_to_numpy(r["data"]), eng.fb_to_numpy(r["kept"])
        assert kept.dtype == np.int32 and np.array_equal(kept, k), (op, F, T)
        if op == "sum":
            assert poisoned is False or np.isfinite(data[~np.isnan(s)]).all()
            assert (same(data, s.astype(np.float32)) if exact else close(data, s)), (op, F, T)
        elif exact:  # the Float32 quotient, bit for bit (NaN where nothing is kept)
            assert same(data, mean) and np.array_equal(np.isnan(data), k == 0), (op, F, T)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                assert close(data, s / k), (op, F, T)
    return eng.masked_reduce_plan(x, md, F, T, win)


def kept_nan(eng, a, F, T, win=None):
    """One kept NaN gives NaN in exactly its block."""
    a = a.copy()
    w = view(a, win)
    w[F + F // 2, w.shape[1] - 1, T - 1] = np.nan  # in block (1, ni - 1, 0)
    m = np.zeros(w.shape, np.uint8)
    x = put(eng, a)
    for op in ("sum", "mean"):
        d = eng.fb_to_numpy(eng.masked_reduce(x, dmask(m), F, T, op, win)["data"])
        want = np.zeros(d.shape, bool)
        want[1, w.shape[1] - 1, 0] = True
        assert np.array_equal(np.isnan(d), want), (op, F, T)


# ---- lanes: 1 .. 64 lanes of a wave, both batch sizes and their tails -----------------
@pytest.mark.parametrize("F", LANES_F)
def test_lanes(eng, F):
    for T in LANES_T:
        shape = (3 * F, 2, 2 * T)
        a = int_data(shape, 100 * F + T)
        for name, m in masks(shape, F, T, F + T).items():
            p = check(eng, a, m, F, T, odd=name == "odd_address",
                      ops=("sum", "mean") if name in ("random", "all", "bool") else ("sum",))
            # (so few blocks never fill the GPU: the rows are split once a slice holds 16)
            assert p["path"] == ("lanes_tsplit" if T >= 32 else "lanes"), (name, T)
            assert p["vector_loads"] == (F % 4 == 0), (name, T)
            want = ("row" if name in ("bad_spectra", "bad_ifs") else
                    "byte" if F % 4 or name == "odd_address" else "dword")
            assert p["mask_loads"] == want, (name, F, T)
        kept_nan(eng, a, F, T)
        check(eng, gamma_data(shape, F * T), masks(shape, F, T, 1)["random"], F, T, exact=False)
        # all-zero mask: the plain reduce's sum exactly, and every sample kept
        x = put(eng, a)
        r = eng.masked_reduce(x, dmask(np.zeros((1, 1, 1), np.uint8)), F, T)
        assert same(eng.fb_to_numpy(r["data"]), eng.fb_to_numpy(eng.reduce(x, F, T, "sum")))
        assert (eng.fb_to_numpy(r["kept"]) == F * T).all()


def test_lanes_unsplit_at_33_rows(eng):
    """Enough blocks to fill the GPU keep T = 33 unsplit: two dword batches of 16
    rows and a tail of one."""
    shape = (4096, 1, 64 * 33)
    a = int_data(shape, 33)
    m = np.where(np.random.default_rng(34).random(shape) < 0.3, 255, 0).astype(np.uint8)
    p = check(eng, a, m, 1, 33)
    assert p["path"] == "lanes" and p["time_slices"] == 1 and p["outputs"] == 4096 * 64


@pytest.mark.parametrize("F", LANES_F)
def test_lanes_windows(eng, F):
    """A channel offset of 3, a channel step of 2, a reversed time range."""
    for T in (3, 16):
        nc, nt = 3 * F, 2 * T
        a = int_data((2 * nc + 3, 2, nt + 1), 7 * F + T)
        for win in ([3, nc, 1, 0, 2, 1, 0, nt, 1], [1, nc, 2, 0, 2, 1, 1, nt, 1],
                    [0, nc, 1, 1, 1, 1, nt, nt, -1], [2 * nc + 2, nc, -2, 0, 2, 1, nt - 1, nt, -1]):
            shape = (win[1], win[4], win[7])
            ms = masks(shape, F, T, F)
            for name in ("random", "bad_channels", "bad_spectra", "odd_address"):
                p = check(eng, a, ms[name], F, T, win, odd=name == "odd_address")
                assert p["path"] == "lanes"
                assert p["vector_loads"] == (F % 4 == 0 and win[2] == 1)
            kept_nan(eng, a, F, T, win)


# ---- lanes_tsplit: time slices of a workgroup meet through LDS ------------------------
@pytest.mark.parametrize("nc,F", [(8, 8), (6, 2)])
@pytest.mark.parametrize("T", [64, 100, 1024])
def test_lanes_tsplit(eng, nc, F, T):
    shape = (nc, 1, 2 * T)
    a = int_data(shape, nc * T)
    nco = nc // F
    for name, m in masks(shape, F, T, T).items():
        if name == "one_block" and nco < 2:
            m = np.zeros(shape, np.uint8)
            m[:, :, T:] = 1  # block (0, 0, 1) beside the unflagged (0, 0, 0)
        p = check(eng, a, m, F, T, odd=name == "odd_address")
        assert p["path"] == "lanes_tsplit" and p["time_slices"] > 1, name
    check(eng, gamma_data(shape, T), masks(shape, F, T, 2)["random"], F, T, exact=False)
    b = a.copy()
    b[nc - 1, 0, 2 * T - 1] = np.nan  # kept: the last block alone is NaN
    d = eng.fb_to_numpy(eng.masked_reduce(put(eng, b), dmask(np.zeros(shape, np.uint8)), F, T)["data"])
    want = np.zeros(d.shape, bool)
    want[-1, 0, -1] = True
    assert np.array_equal(np.isnan(d), want)


# ---- block: one workgroup per block --------------------------------------------------
@pytest.mark.parametrize("F", BLOCK_F)
@pytest.mark.parametrize("T", [1, 3])
def test_block(eng, F, T):
    shape = (3 * F, 2, 2 * T)
    a = int_data(shape, F + T)
    for name, m in masks(shape, F, T, F - T).items():
        p = check(eng, a, m, F, T, odd=name == "odd_address")
        assert p["path"] == "block" and p["lanes_per_block"] == 256, name
        want = ("row" if name in ("bad_spectra", "bad_ifs") else
                "byte" if F % 4 or name == "odd_address" else "dword")
        assert p["mask_loads"] == want, name
    kept_nan(eng, a, F, T)
    check(eng, gamma_data(shape, F), masks(shape, F, T, 3)["random"], F, T, exact=False)
    win = [3, 3 * F, 2, 0, 2, 1, 2 * T - 1, 2 * T, -1]  # offset 3, step 2, time reversed
    big = int_data((6 * F + 5, 2, 2 * T), F)
    check(eng, big, masks(shape, F, T, 4)["random"], F, T, win)


def test_blocks_of_one(eng):
    """F = T = 1: data = kept ? x : 0."""
    a = int_data((37, 2, 5), 1) - 100.0
    m = masks(a.shape, 1, 1, 9)["random"]
    ap = poison(a, None, m)
    r = eng.masked_reduce(put(eng, ap), dmask(m))
    assert np.array_equal(eng.fb_to_numpy(r["data"]), np.where(m != 0, 0, a))
    assert np.array_equal(eng.fb_to_numpy(r["kept"]), (m == 0).astype(np.int32))


# ---- layout ------------------------------------------------------------------------------
def raw_call(pkg, x, md, F, T, op, out_ptr, kept_ptr, ld_i, ld_t):
    eng = pkg.engine
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    mptr, ld = eng._mask_arg(md, tuple(x.shape), x.device, "test")
    rc = pkg._lib.lib().bldp_masked_reduce_f32(ptr, nchan, nif, ntime, None, F, T, op, mptr, ld,
                                               out_ptr, kept_ptr, ld_i, ld_t, None)
    pkg._lib.check(rc, "bldp_masked_reduce_f32")


@pytest.mark.parametrize("F,T", [(8, 4), (5, 3), (2048, 1)])
def test_strided_outputs_and_single_outputs(eng, pkg, F, T):
    import torch

    shape = (3 * F, 2, 2 * T)
    a, m = int_data(shape, 11), masks(shape, F, T, 12)["random"]
    x, md = put(eng, a), dmask(m)
    s, k, mean = masked_ref(a, m, F, T)
    nco, ni, nto = s.shape
    # the middle slot of a three-bank product, guard values around it
    out = eng.fb_empty(3 * nco, ni, nto, device="cuda:0")
    kept = eng.fb_empty(3 * nco, ni, nto, device="cuda:0", dtype=torch.int32)
    out.fill_(-7.0)
    kept.fill_(-7)
    raw_call(pkg, x, md, F, T, 0, out.data_ptr() + 4 * nco, kept.data_ptr() + 4 * nco, 3 * nco,
             3 * nco * ni)
    o, kk = eng.fb_to_numpy(out), eng.fb_to_numpy(kept)
    assert same(o[nco:2 * nco], s.astype(np.float32)) and np.array_equal(kk[nco:2 * nco], k)
    for g in (o[:nco], o[2 * nco:], kk[:nco], kk[2 * nco:]):
        assert (g == -7).all()
    # out only, kept only
    out.fill_(-7.0)
    kept.fill_(-7)
    raw_call(pkg, x, md, F, T, 1, out.data_ptr(), None, 3 * nco, 3 * nco * ni)
    raw_call(pkg, x, md, F, T, 0, None, kept.data_ptr() + 8 * nco, 3 * nco, 3 * nco * ni)
    o, kk = eng.fb_to_numpy(out), eng.fb_to_numpy(kept)
    assert same(o[:nco], mean) and (o[nco:] == -7).all()
    assert np.array_equal(kk[2 * nco:], k) and (kk[:2 * nco] == -7).all()


@pytest.mark.parametrize("F,T", [(8, 4), (3, 5), (1028, 1), (8, 64)])
def test_band_is_the_vcat(eng, F, T):
    nc = 8 if T == 64 else 3 * F
    shape = (nc, 2, 2 * T)
    banks = [int_data(shape, 20 + b) for b in range(3)]
    for name in ("random", "bad_channels", "bad_spectra", "odd_address"):
        m = masks((3 * nc, 2, 2 * T), F, T, 30)[name]
        pb = [poison(a, None, m[b * nc:(b + 1) * nc] if m.shape[0] > 1 else m)
              for b, a in enumerate(banks)]
        xs = [put(eng, a) for a in pb]
        for op in ("sum", "mean"):
            r = eng.band_masked_reduce(xs, dmask(m, name == "odd_address"), F, T, op)
            parts = [masked_ref(a, m[b * nc:(b + 1) * nc] if m.shape[0] > 1 else m, F, T)
                     for b, a in enumerate(pb)]
            want = np.concatenate([p[0].astype(np.float32) if op == "sum" else p[2] for p in parts])
            assert same(eng.fb_to_numpy(r["data"]), want), (name, op)
            assert np.array_equal(eng.fb_to_numpy(r["kept"]), np.concatenate([p[1] for p in parts]))
            # ... and of the per-bank calls
            for b, x in enumerate(xs):
                mb = m[b * nc:(b + 1) * nc] if m.shape[0] > 1 else m
                one = eng.masked_reduce(x, dmask(mb), F, T, op)
                assert same(eng.fb_to_numpy(one["data"]), want[b * (nc // F):(b + 1) * (nc // F)])


# ---- composition ---------------------------------------------------------------------------
def spiky(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(100, 110, shape).astype(np.float32)
    a[rng.random(shape) < 0.02] = 255.0
    return a


@pytest.mark.parametrize("axis,n", [(0, 16), (2, 8), (2, None)])
def test_outliers_mask_goes_straight_in(eng, axis, n):
    a = spiky((64, 2, 24), 40 + axis)
    x = put(eng, a)
    o = eng.outliers(x, n, axis=axis, nsigma=3.0, mask=True, which=("count",))
    m = eng.fb_to_numpy(o["mask"])
    assert m.any() and np.array_equal(m, outliers_ref(a, n or 24, 3.0, None, axis)[3])
    for F, T in ((16, 8), (4, 1), (1, 24), (64, 3)):
        s, k, mean = masked_ref(a, m, F, T)
        r = eng.masked_reduce(x, o["mask"], F, T)
        assert same(eng.fb_to_numpy(r["data"]), s.astype(np.float32))
        assert np.array_equal(eng.fb_to_numpy(r["kept"]), k)
        assert int(r["kept"].sum()) + int(o["count"].sum()) == a.size
    b = eng.band_outliers([x, x], n, axis=axis, nsigma=3.0, mask=True, which=("count",))
    r = eng.band_masked_reduce([x, x], b["mask"], 16, 8)
    s, k, _ = masked_ref(a, m, 16, 8)
    assert same(eng.fb_to_numpy(r["data"]), np.concatenate([s, s]).astype(np.float32))
    assert np.array_equal(eng.fb_to_numpy(r["kept"]), np.concatenate([k, k]))


def clean_ref(data, win, F, T, n, axis, nsigma, op):
    w = np.asfortranarray(window(data, win))
    _, _, count, m = outliers_ref(w, n, nsigma, None, axis)
    s, k, mean = masked_ref(w, m, F, T)
    return {"data": s.astype(np.float32) if op == "sum" else mean, "kept": k, "count": count}


def matches(got, want):
    return (sorted(got) == sorted(want) and
            all(same(np.asarray(got[k]), np.asarray(want[k]).astype(got[k].dtype)) for k in want))


def test_getmasked_and_getclean(eng, pkg, orc, tmp_path):
    import torch

    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = spiky((64, 2, 40), 50)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=64), data)
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    m = masks((32, 2, 32), 8, 4, 51)["random"]
    bad = masks((32, 2, 32), 8, 4, 52)["bad_channels"]
    x = put(eng, data)
    for src in (data, x, fil, raw):
        dev = isinstance(src, torch.Tensor)
        host = (lambda r: {k: eng.fb_to_numpy(t) for k, t in r.items()}) if dev else (lambda r: r)
        for mk in (m, bad, m != 0, dmask(m)):
            for func in ("sum", "mean"):
                got = W.getmasked(src, idxs, mask=mk, fqavby=8, tavby=4, func=func)
                assert all(isinstance(v, torch.Tensor if dev else np.ndarray) for v in got.values())
                mh = mk.cpu().numpy() if isinstance(mk, torch.Tensor) else mk
                s, k, mean = masked_ref(window(data, win), mh, 8, 4)
                assert matches(host(got), {"data": s.astype(np.float32) if func == "sum" else mean,
                                           "kept": k})
        for axis, n in ((2, 16), (0, 8), (2, None)):
            got = W.getclean(src, idxs, fqavby=8, tavby=4, n=n, axis=axis, nsigma=3.0, func="mean")
            assert all(isinstance(v, torch.Tensor if dev else np.ndarray) for v in got.values())
            want = clean_ref(data, win, 8, 4, n or 32, axis, 3.0, "mean")
            assert matches(host(got), want), (axis, n)
            assert int(want["kept"].sum()) + int(want["count"].sum()) == 32 * 2 * 32
        got = W.getclean(src, fqavby=64)  # the defaults: the whole time range, 5 mads, the sum
        assert matches(host(got), clean_ref(data, None, 64, 1, 40, 2, 5.0, "sum"))
    parts = pkg.GBT.getclean([0, 0], [fil, raw], idxs, fqavby=8, tavby=4, n=16, nsigma=3.0)
    assert len(parts) == 2
    for p in parts:
        assert matches(p, clean_ref(data, win, 8, 4, 16, 2, 3.0, "sum"))


def test_host_entry_point(eng):
    a = int_data((40, 2, 12), 60)
    win = [3, 32, 1, 0, 2, 1, 11, 12, -1]
    for name, m in masks((32, 2, 12), 8, 4, 61).items():
        ap = poison(a, win, m)
        s, k, mean = masked_ref(window(ap, win), m, 8, 4)
        r = eng.masked_reduce_host(np.asfortranarray(ap), m, 8, 4, "mean", win)
        assert r["data"].flags.f_contiguous and r["kept"].dtype == np.int32
        assert same(r["data"], mean) and np.array_equal(r["kept"], k), name
