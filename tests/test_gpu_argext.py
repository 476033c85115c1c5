"""GPU: fqavfunc "argmax" / "argmin" (csrc/argext.hip) against Julia's rule
restated in NumPy below.  Every comparison is exact: offsets with array_equal,
the winners' bits with same_bits.

The restatement maps every element to the canonical uint32 key (isless as
unsigned order, inverted for argmin, 0xffffffff for any NaN) and takes
np.argmax along the block axis, which returns the first occurrence on integers;
the block axis is Julia's column-major order of reshape(A, (F, :, ni, T, :)),
off = k + F * tt.  It is cross-checked against a literal loop on a small case."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu

OPS = ("argmax", "argmin")


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


# ---------------------------------------------------------------------------
# Julia's rule in NumPy

def window(a, win):
    if win is None:
        return a
    return a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1]) for k in range(3)])]


def blocks(a, F, T, win=None):
    """(F*T, nco, ni, nto): axis 0 walks a block in offset order k + F * tt."""
    w = np.asfortranarray(window(a, win))
    nc, ni, nt = w.shape
    assert nc % F == 0 and nt % T == 0
    R = w.reshape((F, nc // F, ni, T, nt // T), order="F")
    return np.asfortranarray(np.moveaxis(R, 3, 1)).reshape((F * T, nc // F, ni, nt // T), order="F")


def key32(x, op):
    u = x.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000) != 0, ~u, u | np.uint32(0x80000000))
    if op == "argmin":
        k = ~k
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k)


def arg_ref(a, F, T, op, win=None):
    B = blocks(a, F, T, win)
    idx = np.argmax(key32(B, op), axis=0)
    val = np.take_along_axis(B, idx[None], axis=0)[0]
    return np.asfortranarray(idx.astype(np.int32)), np.asfortranarray(val)


def test_restatement_against_a_literal_loop():
    nan = np.float32(np.nan)
    rows = {  # block (in offset order): (argmax, argmin)
        (1.0, 3.0, 3.0, -2.0, -2.0, 0.5): (1, 3),
        (0.0, -0.0, -1.0, -1.0, -0.0, 0.0): (0, 2),
        (-0.0, 0.0, 1.0, 1.0, 0.0, -0.0): (2, 0),
        (5.0, 0.0, -0.0, 9.0, nan, -nan): (4, 4),
        (np.inf, -np.inf, np.inf, -np.inf, 1.0, 2.0): (0, 1),
        (-0.0, 0.0, 0.0, -0.0, 0.0, -0.0): (1, 0),
    }
    for blk, (imax, imin) in rows.items():
        a = np.asfortranarray(np.float32(blk).reshape((2, 1, 3), order="F"))  # F = 2, T = 3
        assert arg_ref(a, 2, 3, "argmax")[0][0, 0, 0] == imax, blk
        assert arg_ref(a, 2, 3, "argmin")[0][0, 0, 0] == imin, blk
    # the offset order itself: [c, 0, t] = c + 10 t, the greatest is the last row's last channel
    b = np.asfortranarray((np.arange(6)[:, None, None] + 10.0 * np.arange(4)[None, None, :])
                          .astype(np.float32))
    idx, val = arg_ref(b, 3, 2, "argmax")
    assert np.array_equal(idx[:, 0, :], [[5, 5], [5, 5]]) and np.array_equal(val[:, 0, :],
                                                                              [[12, 32], [15, 35]])
    assert np.array_equal(arg_ref(b, 3, 2, "argmin", [5, 6, -1, 0, 1, 1, 3, 4, -1])[0][:, 0, 0],
                          [5, 5])  # reversed: the least is again the block's last element


# ---------------------------------------------------------------------------
# data

def ties(shape, seed):
    """4 distinct values: every block has many maxima and minima."""
    v = np.float32([-3.5, -0.0, 0.0, 1e30])
    return np.asfortranarray(v[np.random.default_rng(seed).integers(0, 4, shape)])


def set_block(a, F, T, blk, vec):
    co, i, to = blk
    a[co * F:(co + 1) * F, i, to * T:(to + 1) * T] = np.asarray(vec, np.float32).reshape(
        (F, T), order="F")


def nan_bits(bits):
    return np.uint32(bits).view(np.float32)


def specials(shape, F, T, seed):
    """Signed normals, and whole blocks of: adjacent +-0 in both orders over a
    lower and over a higher fill, +-Inf twice each, NaNs of both signs and
    different payloads at the first offset, at the last, and in a later row than
    an earlier maximum, and a block that is all NaN."""
    rng = np.random.default_rng(seed)
    a = np.asfortranarray((rng.standard_normal(shape) * 1e3).astype(np.float32))
    n = F * T
    nco, ni, nto = shape[0] // F, shape[1], shape[2] // T
    where = [(c, i, t) for t in range(nto) for i in range(ni) for c in range(nco)]
    def noise():
        return (rng.standard_normal(n) * 10).astype(np.float32)

    fills = []
    v = noise()
    if n > 2:  # an early maximum and minimum, then two NaNs in the last row
        v[0], v[1] = 1e6, -1e6
        v[F * (T - 1) + (F - 1) // 2] = nan_bits(0xFFFFFFFF)
        v[n - 1] = nan_bits(0x7F800001)
    fills.append(v)
    m = (n - 2) // 2
    for fill, pair in ((-5.0, (0.0, -0.0)), (5.0, (-0.0, 0.0)), (-5.0, (-0.0, 0.0)),
                       (5.0, (0.0, -0.0))):
        v = np.full(n, fill, np.float32)
        v[m:m + 2] = pair
        fills.append(v)
    v = noise()
    v[0] = 1e6
    v[n - 1] = nan_bits(0xFFC00123)  # the last offset, after the extremes
    fills.insert(2, v)
    v = noise()
    v[0] = nan_bits(0x7FC00001)      # the first offset, and another at the last
    v[n - 1] = nan_bits(0xFFC00123)
    fills.insert(3, v)
    v = noise()
    pos = rng.permutation(n)[:4]
    v[pos] = np.float32([np.inf, -np.inf, np.inf, -np.inf])[:len(pos)]
    fills.append(v)
    # all NaN, every payload different from its neighbours'
    fills.append((np.uint32(0x7FC00007) + np.arange(n, dtype=np.uint32) % np.uint32(1000))
                 .view(np.float32))
    for blk, vec in zip(where[::-1], fills):
        set_block(a, F, T, blk, vec)
    return a


def put(eng, a):
    return eng.fb_from_numpy(a, device="cuda:0")


def check(eng, a, F, T, win=None, x=None, msg=""):
    """argmax and argmin of one array, with and without the value output."""
    x = put(eng, a) if x is None else x
    for op in OPS:
        want_i, want_v = arg_ref(a, F, T, op, win)
        idx, val = eng.argext(x, F, T, op, win, values=True)
        got_i, got_v = eng.fb_to_numpy(idx), eng.fb_to_numpy(val)
        assert got_i.dtype == np.int32 and got_v.dtype == np.float32
        assert np.array_equal(got_i, want_i), (msg, op, F, T)
        # the winner's own bits, NaN payloads included
        assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), (msg, op, F, T)
        assert same_bits(got_v, want_v)
        only = eng.fb_to_numpy(eng.argext(x, F, T, op, win))  # val NULL
        assert np.array_equal(only, want_i), (msg, op, F, T, "val NULL")


# ---------------------------------------------------------------------------
# every form and boundary

SWEEP_F = [2, 3, 4, 12, 64, 68, 1024, 1028, 4096]
SWEEP_T = [1, 2, 3, 16]
EXTRA = [(65536, 1, (131072, 1, 2)), (65536, 2, (131072, 1, 2)),  # a workgroup on a long block
         (8, 1024, (16, 1, 2048)),                                # the time-split form
         (64, 48, (320, 2, 48)), (4096, 6, (8192, 1, 6))]          # T = nt


def path_of(F, T):
    return "block" if F > 1024 else "lanes_tsplit" if T >= 32 else "lanes"


@pytest.mark.parametrize("T", SWEEP_T)
@pytest.mark.parametrize("F", SWEEP_F)
def test_sweep(eng, F, T):
    shape = (5 * F, 2, 3 * T)
    plan = eng.argext_plan(eng.fb_empty(*shape, device="cuda:0"), F, T, "argmax")
    assert plan["path"] == path_of(F, T) and plan["outputs"] == 30, plan
    assert plan["vector_loads"] == (F % 4 == 0) and plan["workspace_bytes"] == 0
    synth = eng.synth(*shape, nfpc=4, seed=F + T, kind=0, device="cuda:0")
    check(eng, eng.fb_to_numpy(synth), F, T, x=synth, msg="synth")
    check(eng, ties(shape, F * 100 + T), F, T, msg="ties")
    check(eng, np.full(shape, -0.0, np.float32, order="F"), F, T, msg="constant")
    sp = specials(shape, F, T, F + 7 * T)
    check(eng, sp, F, T, msg="specials")
    if F * T > 2:  # the NaN blocks: first offset, last offset, the earlier NaN of a later row
        idx = arg_ref(sp, F, T, "argmax")[0].ravel(order="F")
        assert {0, F * T - 1, F * (T - 1) + (F - 1) // 2} <= set(idx.tolist())


@pytest.mark.parametrize("F,T,shape", EXTRA)
def test_long_blocks_time_split_and_whole_time_axis(eng, F, T, shape):
    plan = eng.argext_plan(eng.fb_empty(*shape, device="cuda:0"), F, T, "argmin")
    assert plan["path"] == path_of(F, T), plan
    if (F, T) == (8, 1024):
        assert plan["time_slices"] == 64 and plan["lanes_per_block"] == 2 and plan["workgroups"] == 2
    check(eng, ties(shape, F + T), F, T, msg="ties")
    check(eng, specials(shape, F, T, F + T), F, T, msg="specials")
    a = ties(shape, 3)
    a[shape[0] - 1, 0, shape[2] - 1] = np.float32(2e30)  # the only maximum: the last element
    a[shape[0] - 2, 0, shape[2] - 1] = np.float32(-4.0)
    check(eng, a, F, T, msg="last element")


def test_every_path_is_planned_for_a_shape_that_runs(eng, pkg):
    seen = set()
    for F in SWEEP_F:
        for T in SWEEP_T:
            x = eng.fb_empty(5 * F, 2, 3 * T, device="cuda:0")
            seen.add(eng.argext_plan(x, F, T, "argmax")["path"])
    for F, T, shape in EXTRA:
        seen.add(eng.argext_plan(eng.fb_empty(*shape, device="cuda:0"), F, T, "argmax")["path"])
    assert seen == set(pkg._lib.ARGEXT_PATHS.values())


def test_blocks_of_one_element(eng):
    a = specials((24, 2, 6), 4, 3, 1)
    x = put(eng, a)
    for F, T in ((1, 1), (0, 1), (1, -3)):
        idx, val = eng.argext(x, F, T, "argmax", values=True)
        assert tuple(idx.shape) == (24, 2, 6) and not eng.fb_to_numpy(idx).any()
        assert np.array_equal(eng.fb_to_numpy(val).view(np.uint32), a.view(np.uint32))
    check(eng, a, 1, 3, x=x)
    check(eng, a, 4, 1, x=x)


# ---------------------------------------------------------------------------
# windows

WIN_SHAPE = (300, 3, 24)
WINDOWS = {
    "c0=3": [3, 128, 1, 0, 3, 1, 0, 24, 1],             # off the 16-byte boundary
    "channel step 2": [1, 128, 2, 0, 3, 1, 0, 24, 1],
    "reversed channels": [299, 128, -1, 0, 3, 1, 0, 24, 1],
    "IF subset": [0, 128, 1, 1, 2, 1, 0, 24, 1],
    "one IF of three": [4, 128, 1, 2, 1, 1, 0, 24, 1],
    "time offset 1 step 3": [0, 128, 1, 0, 3, 1, 1, 8, 3],
    "reversed time": [3, 128, 1, 0, 3, 1, 23, 24, -1],
}


@pytest.fixture(scope="module")
def win_data(eng):
    rng = np.random.default_rng(17)
    a = ties(WIN_SHAPE, 17)
    hit = rng.random(WIN_SHAPE) < 0.01
    a[hit] = rng.choice(np.float32([np.nan, -np.nan, np.inf, -np.inf]), int(hit.sum()))
    return a, put(eng, a)


@pytest.mark.parametrize("FT", [(4, 1), (64, 1), (8, 4), (128, 8), (32, 2)])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows(eng, win_data, name, FT):
    a, x = win_data
    w = WINDOWS[name]
    F, T = FT
    assert eng.argext_plan(x, F, T, "argmax", w)["vector_loads"] == (w[2] == 1), name
    check(eng, a, F, T, w, x=x, msg=name)


def test_window_errors(eng):
    x = put(eng, ties((64, 2, 8), 1))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        eng.argext(x, 5, 1, "argmax")
    with pytest.raises(ValueError, match="DimensionMismatch"):
        eng.argext(x, 4, 3, "argmax")
    with pytest.raises(IndexError):
        eng.argext(x, 4, 1, "argmax", [0, 68, 1, 0, 2, 1, 0, 8, 1])
    with pytest.raises(ValueError):
        eng.argext(x, 4, 1, "max")


# ---------------------------------------------------------------------------
# layers

def test_strided_outputs_leave_the_guards(eng):
    import torch

    a = ties((256, 2, 32), 5)
    x = put(eng, a)
    for F, T in ((64, 1), (8, 16), (4, 32)):
        nco, nto = 256 // F, 32 // T
        want_i, want_v = arg_ref(a, F, T, "argmin")
        big_i = eng.fb_empty(3 * nco, 2, nto, device="cuda:0", dtype=torch.int32)
        big_v = eng.fb_empty(3 * nco, 2, nto, device="cuda:0")
        big_i.fill_(-7)
        big_v.fill_(-7.0)
        si, sv = big_i[nco:2 * nco], big_v[nco:2 * nco]
        r = eng.argext(x, F, T, "argmin", values=True, out=(si, sv))
        assert r[0] is si and r[1] is sv
        torch.cuda.synchronize()
        hi, hv = eng.fb_to_numpy(big_i), eng.fb_to_numpy(big_v)
        assert np.array_equal(hi[nco:2 * nco], want_i) and same_bits(hv[nco:2 * nco], want_v)
        assert (hi[:nco] == -7).all() and (hi[2 * nco:] == -7).all()
        assert (hv[:nco] == -7).all() and (hv[2 * nco:] == -7).all()
        # idx alone into a slot
        big_i.fill_(-7)
        assert eng.argext(x, F, T, "argmin", out=si) is si
        hi = eng.fb_to_numpy(big_i)
        assert np.array_equal(hi[nco:2 * nco], want_i) and (hi[:nco] == -7).all()


def test_bad_out_raises_before_any_launch(eng, pkg):
    import torch

    x = put(eng, ties((64, 2, 32), 1))
    good = eng.fb_empty(16, 2, 2, device="cuda:0", dtype=torch.int32)
    good.fill_(-1)
    bad = [eng.fb_empty(16, 2, 2, device="cuda:0"),                      # Float32 idx
           eng.fb_empty(16, 2, 4, device="cuda:0", dtype=torch.int32),   # shape
           torch.empty((16, 2, 2), dtype=torch.int32, device="cuda:0"),  # row-major
           torch.empty((2, 2, 16), dtype=torch.int32, device="cpu").permute(2, 1, 0)]
    for out in bad:
        with pytest.raises((TypeError, ValueError)):
            eng.argext(x, 4, 16, "argmax", out=out)
    with pytest.raises(TypeError):
        eng.argext(x, 4, 16, "argmax", values=True, out=good)  # a pair is needed
    with pytest.raises((TypeError, ValueError)):
        eng.argext(x, 4, 16, "argmax", values=True,
                   out=(good, eng.fb_empty(32, 2, 2, device="cuda:0")[::2]))
    # the ABI refuses outputs inside the input
    L = pkg._lib.lib()
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    rc = L.bldp_argext_f32(ptr, nchan, nif, ntime, None, 4, 16, 0, ptr + 64, None, 16, 32,
                           pkg._lib.stream_ptr())
    assert rc == pkg._lib.BLDP_EINVAL and "overlap" in pkg._lib.last_error()
    torch.cuda.synchronize()
    assert (good == -1).all()


def test_band_is_the_concatenation(eng):
    banks = [specials((320, 2, 48), 64, 16, 20), ties((320, 2, 48), 21)]
    xs = [put(eng, b) for b in banks]
    for F, T, op in ((64, 16, "argmax"), (64, 1, "argmin"), (8, 48, "argmax"), (320, 2, "argmin")):
        bi, bv = eng.band_argext(xs, F, T, op, values=True)
        parts = [arg_ref(b, F, T, op) for b in banks]
        assert np.array_equal(eng.fb_to_numpy(bi), np.concatenate([p[0] for p in parts], axis=0))
        assert same_bits(eng.fb_to_numpy(bv), np.concatenate([p[1] for p in parts], axis=0))
        per = [eng.fb_to_numpy(eng.argext(x, F, T, op)) for x in xs]
        assert np.array_equal(eng.fb_to_numpy(eng.band_argext(xs, F, T, op)),
                              np.concatenate(per, axis=0))


def test_host_entry_point(eng):
    a = specials((200, 2, 96), 8, 16, 8)
    for F, T, op in ((8, 16, "argmax"), (200, 1, "argmin"), (4, 96, "argmax")):
        idx, val = eng.argext_host(a, F, T, op, values=True)
        want_i, want_v = arg_ref(a, F, T, op)
        assert idx.dtype == np.int32 and np.array_equal(idx, want_i) and same_bits(val, want_v)
        assert np.array_equal(eng.argext_host(a, F, T, op), want_i)
    win = [197, 96, -2, 1, 1, 1, 95, 48, -2]  # reversed channels and time: staged in window order
    idx, val = eng.argext_host(a, 8, 16, "argmin", win, values=True)
    want_i, want_v = arg_ref(a, 8, 16, "argmin", win)
    assert np.array_equal(idx, want_i) and same_bits(val, want_v)


def test_fqav_getdata_findmax_on_arrays(eng, pkg):
    import torch

    W = pkg.worker
    a = specials((256, 2, 24), 8, 4, 3)
    x = put(eng, a)
    r = W.fqav(x, 8, "argmax")
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.int32
    assert np.array_equal(eng.fb_to_numpy(r), arg_ref(a, 8, 1, "argmax")[0])
    assert np.array_equal(W.fqav(a, 8, "argmin"), arg_ref(a, 8, 1, "argmin")[0])
    assert W.fqav(x, 1, "argmax") is x
    idxs = (pkg.JRange(5, 132), pkg.COLON, pkg.JRange(24, -1, 1))
    win = [4, 128, 1, 0, 2, 1, 23, 24, -1]
    r = W.getdata(x, idxs, fqavby=8, fqavfunc="argmin", tavby=4)
    assert r.is_cuda and np.array_equal(eng.fb_to_numpy(r), arg_ref(a, 8, 4, "argmin", win)[0])
    h = W.getdata(a, idxs, fqavby=8, fqavfunc="argmin", tavby=4)
    assert h.dtype == np.int32 and np.array_equal(h, arg_ref(a, 8, 4, "argmin", win)[0])
    # findmax / findmin: the values are the input at the returned offsets
    for fn, op in ((W.findmax, "argmax"), (W.findmin, "argmin")):
        vals, idx = fn(a, fqavby=8, tavby=4)
        assert np.array_equal(idx, arg_ref(a, 8, 4, op)[0])
        for (co, i, to), off in np.ndenumerate(idx):
            assert a[co * 8 + off % 8, i, to * 4 + off // 8].tobytes() == vals[co, i, to].tobytes()
        dv, di = fn(x, fqavby=8, tavby=4)
        assert dv.is_cuda and np.array_equal(eng.fb_to_numpy(di), idx)
        assert same_bits(eng.fb_to_numpy(dv), vals)
    with pytest.raises(TypeError, match="tavfunc"):
        W.getdata(x, fqavby=8, fqavfunc="argmax", tavby=4, tavfunc="sum")


def test_getdata_files_and_getband(eng, pkg, orc, tmp_path):
    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = specials((64, 2, 40), 8, 8, 4)
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
        got = W.getdata(src, fqavby=8, fqavfunc="argmax", tavby=8)
        assert got.dtype == np.int32 and np.array_equal(got, arg_ref(data, 8, 8, "argmax")[0]), src
        assert np.array_equal(W.getdata(src, idxs, fqavby=4, fqavfunc="argmin", tavby=16),
                              arg_ref(data, 4, 16, "argmin", win)[0]), src
        vals, idx = W.findmax(src, idxs, fqavby=4, tavby=1)
        want_i, want_v = arg_ref(data, 4, 1, "argmax", win)
        assert np.array_equal(idx, want_i) and same_bits(vals, want_v), src
    want = arg_ref(data, 8, 8, "argmin")[0]
    band = pkg.GBT.getband([0, 0], [fil, bs], fqavby=8, fqavfunc="argmin", tavby=8)
    assert band.dtype == np.int32 and np.array_equal(band, np.concatenate([want, want], axis=0))
    parts = pkg.GBT.getdata([0, 0], [fil, raw], fqavby=8, fqavfunc="argmin", tavby=8)
    assert all(np.array_equal(p, want) for p in parts)
    with pytest.raises(TypeError, match="despike"):
        pkg.GBT.getband([0, 0], [fil, bs], fqavby=8, fqavfunc="argmin", despike_nfpc=4)
