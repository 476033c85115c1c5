"""GPU: the hits list (csrc/hits.hip) against the NumPy restatement of its rule
(hits_ref.py).  Every comparison is equality: ``total``, ``idx``, and ``val`` by
bits.  The data is random bit patterns (NaNs with payloads, infinities, -0.0 and
denormals occur under flags as they come) with the named specials planted too.
The raw calls write into lists with sentinel slabs before, after and in the
unwritten tail, and the sentinels are asserted untouched."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from hits_ref import hits_ref, snr_ref
from mad_ref import window

pytestmark = pytest.mark.gpu

G = 8                      # sentinel entries before and after a list
SI, SV = -7, 0xdeadbeef    # sentinels: idx, val bits
SPECIAL = np.array([0x7fc01234, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001,
                    0x807fffff], dtype=np.uint32)  # NaN payloads, +-Inf, -0.0, denormals


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def bits_data(shape, seed):
    """Float32 array of random bit patterns, the specials at the front and the back."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 1 << 32, int(np.prod(shape)), dtype=np.uint64).astype(np.uint32)
    n = min(u.size, SPECIAL.size)
    u[:n] = SPECIAL[:n]
    u[u.size - n:] = SPECIAL[:n]
    return u.view(np.float32).reshape(shape, order="F")


def put(eng, a):
    return eng.fb_from_numpy(np.asfortranarray(a), device="cuda:0")


def dmask(m, odd=False):
    """A host mask on the device with channel-fastest strides; ``odd``: as a view
    one byte into a larger byte tensor (test_gpu_masked.py's helper)."""
    import torch

    m = np.asarray(m)
    if m.dtype == np.bool_ or not odd:
        return torch.from_numpy(np.asfortranarray(m).transpose(2, 1, 0).copy()).to("cuda:0") \
            .permute(2, 1, 0)
    nc, ni, nt = m.shape
    buf = torch.zeros(m.size + 1, dtype=torch.uint8, device="cuda:0")
    buf[1:] = torch.from_numpy(m.ravel(order="F").copy()).to("cuda:0")
    v = torch.as_strided(buf, (nc, ni, nt), (1, nc, nc * ni), storage_offset=1)
    assert v.data_ptr() % 2 == 1
    return v


def raw(pkg, xs, md, wshape, cap, win=None, idx=True, val=True):
    """One bldp_hits_f32 (xs a tensor) or bldp_band_hits_f32 (a list) call into
    sentinel-framed lists: (total, idx, val bits) with the sentinels asserted."""
    import torch

    eng, lib = pkg.engine, pkg._lib
    band = isinstance(xs, (list, tuple))
    x0 = xs[0] if band else xs
    mptr, ld = eng._mask_arg(md, wshape, x0.device, "test")
    di = torch.full((cap + 2 * G,), SI, dtype=torch.int64, device="cuda:0")
    dv = torch.full((cap + 2 * G,), SV - (1 << 32), dtype=torch.int32, device="cuda:0")
    dt = torch.full((3,), SI, dtype=torch.int64, device="cuda:0")
    ip = di.data_ptr() + 8 * G if idx else None
    vp = dv.data_ptr() + 4 * G if val else None
    keep, wp = lib.win_arg(eng._full_win(win, tuple(x0.shape)))
    ptr, nchan, nif, ntime = eng._abi_dims(x0)
    if band:
        ptrs = (ctypes.c_void_p * len(xs))(*[b.data_ptr() for b in xs])
        rc = lib.lib().bldp_band_hits_f32(len(xs), ctypes.cast(ptrs, ctypes.c_void_p), nchan, nif,
                                          ntime, wp, mptr, ld, cap, ip, vp, dt.data_ptr() + 8, None)
    else:
        rc = lib.lib().bldp_hits_f32(ptr, nchan, nif, ntime, wp, mptr, ld, cap, ip, vp,
                                     dt.data_ptr() + 8, None)
    lib.check(rc, "hits")
    torch.cuda.synchronize()
    t = dt.cpu().numpy()
    assert t[0] == SI and t[2] == SI
    total = int(t[1])
    n = min(total, cap)
    hi, hv = di.cpu().numpy(), dv.cpu().numpy().view(np.uint32)
    assert (hi[:G] == SI).all() and (hi[G + (n if idx else 0):] == SI).all()
    assert (hv[:G] == SV).all() and (hv[G + (n if val else 0):] == SV).all()
    return total, hi[G:G + n] if idx else None, hv[G:G + n] if val else None


def check(pkg, x, md, a_win, m, cap=None, win=None, what=""):
    """The raw call against the restatement on the host window ``a_win`` and mask ``m``."""
    total, idx, val = hits_ref(a_win, m)
    c = total + 3 if cap is None else cap
    got = raw(pkg, x, md, a_win.shape, c, win)
    assert got[0] == total, what
    assert np.array_equal(got[1], idx[:c]), what
    assert np.array_equal(got[2], val[:c].view(np.uint32)), what
    return total


def densities(N, tile, seed, W=1):
    """name -> flat (column-major) uint8 flags of N elements.  ``W``: the plan's
    flags per lane per load, so that lanes 63 and 64 of a wave step are elements
    64*W - 1 and 64*W."""
    rng = np.random.default_rng(seed)
    vals = np.array([1, 2, 255], dtype=np.uint8)
    z = lambda: np.zeros(N, dtype=np.uint8)  # noqa: E731
    d = {"empty": z(), "all": vals[np.arange(N) % 3]}
    d["first"], d["last"] = z(), z()
    d["first"][0], d["last"][N - 1] = 1, 255
    d["lanes_63_64"] = z()
    d["lanes_63_64"][np.array([k for k in (64 * W - 1, 64 * W) if k < N], dtype=np.int64)] = 2
    d["tile_edge"] = z()
    d["tile_edge"][np.array([k for k in (tile - 1, tile) if k < N], dtype=np.int64)] = 1
    for name, p in (("sparse", 1e-3), ("dense", 0.3)):
        d[name] = np.where(rng.random(N) < p, vals[rng.integers(0, 3, N)], 0).astype(np.uint8)
    return d


# ---- window sizes, against the planned tile -----------------------------------------------
@pytest.mark.parametrize("nc", [1, 6, 65, 4, 16, 64])
def test_sizes_around_the_tile(eng, pkg, nc):
    p = eng.hits_plan(eng.fb_empty(nc, 1, 1, device="cuda:0"),
                      dmask(np.zeros((nc, 1, 1), np.uint8)))
    tile = p["tile_elems"]
    # (a mask with one channel has a channel stride of 0: the row form, of any N)
    assert p["mask_loads"] == ("wide" if nc % 4 == 0 else "row" if nc == 1 else "byte")
    assert p["flags_per_load"] == (16 if nc % 16 == 0 else 4 if nc % 4 == 0 else 1)
    nts = set()
    for target in (1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 1):
        nts |= {max(1, target // nc), -(-target // nc)}
    for nt in sorted(nts):
        shape = (nc, 1, nt)
        N = nc * nt
        a = bits_data(shape, nt)
        x = put(eng, a)
        q = eng.hits_plan(x, dmask(np.zeros(shape, np.uint8)))
        assert q["tile_elems"] == tile and q["tiles"] == -(-N // tile)
        assert q["flags_per_load"] == p["flags_per_load"]
        for name, f in densities(N, tile, 7 * nt, q["flags_per_load"]).items():
            m = f.reshape(shape, order="F")
            check(pkg, x, dmask(m), a, m, what=(shape, name))


def test_exact_small_sizes(eng, pkg):
    """Windows of exactly 1, 63, 64, 65, 255, 256 and 257 elements, and around the
    byte form's tile, as a column (aligned: the widest load N allows; one byte
    into a buffer: the byte form at any N) and as a row of spectra."""
    for N in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3073):
        for shape, odd in (((N, 1, 1), False), ((N, 1, 1), True), ((1, 1, N), False)):
            a = bits_data(shape, N)
            x = put(eng, a)
            p = eng.hits_plan(x, dmask(np.zeros(shape, np.uint8), odd))
            if odd:
                assert p["mask_loads"] == ("byte" if N > 1 else "row") and p["tile_elems"] == 1024
            for name, f in densities(N, p["tile_elems"], N, p["flags_per_load"]).items():
                m = f.reshape(shape, order="F")
                check(pkg, x, dmask(m, odd), a, m, what=(shape, odd, name))


# ---- mask forms -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 2, 9), (6, 2, 9), (12, 3, 5), (65, 2, 3)])
def test_mask_forms(eng, pkg, shape):
    nc, ni, nt = shape
    a = bits_data(shape, 11)
    x = put(eng, a)
    rng = np.random.default_rng(12)
    vals = np.array([1, 2, 255], dtype=np.uint8)

    def rand(shp):
        return np.where(rng.random(shp) < 0.3, vals[rng.integers(0, 3, shp)], 0).astype(np.uint8)

    dense = rand(shape)
    forms = {"dense": (dense, False), "odd": (dense, True), "bool": (dense != 0, False),
             "chan": (rand((nc, 1, 1)), False), "time": (rand((1, 1, nt)), False),
             "if": (np.array([0, 1, 0][:ni], np.uint8).reshape(1, ni, 1), False),
             "chan_if": (rand((nc, ni, 1)), False), "if_time": (rand((1, ni, nt)), False)}
    want = {"dense": "wide" if nc % 4 == 0 else "byte", "odd": "byte", "time": "row", "if": "row",
            "if_time": "row"}
    for name, (m, odd) in forms.items():
        md = dmask(m, odd)
        if name in want:
            assert eng.hits_plan(x, md)["mask_loads"] == want[name], name
        check(pkg, x, md, a, m, what=(shape, name))
        # through engine.hits: all of them, and cut
        total, idx, val = hits_ref(a, m)
        for mh in (None, 5, total + 2):
            h = eng.hits(x, md, maxhits=mh)
            n = total if mh is None else min(mh, total)
            assert h["total"] == total and isinstance(h["total"], int)
            assert np.array_equal(h["index"].cpu().numpy(), idx[:n])
            assert np.array_equal(h["value"].cpu().numpy().view(np.uint32),
                                  val[:n].view(np.uint32))


# ---- windows ----------------------------------------------------------------------------
WINDOWS = {"full": None, "offset": [3, 32, 1, 0, 3, 1, 0, 10, 1], "cstep": [1, 16, 2, 0, 3, 1, 0, 10, 1],
           "reversed": [35, 32, -1, 0, 3, 1, 0, 10, 1], "steps": [0, 40, 1, 2, 2, -2, 1, 5, 2],
           "ni2": [3, 6, 1, 1, 2, 1, 9, 10, -1], "one": [39, 1, 1, 2, 1, 1, 9, 1, 1]}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows(eng, pkg, name):
    win = WINDOWS[name]
    a = bits_data((40, 3, 10), 21)
    x = put(eng, a)
    w = np.asfortranarray(window(a, win))
    rng = np.random.default_rng(22)
    for p in (0.3, 1.0):
        m = (rng.random(w.shape) < p).astype(np.uint8)
        check(pkg, x, dmask(m), w, m, win=win, what=(name, p))
    chan = (rng.random((w.shape[0], 1, 1)) < 0.5).astype(np.uint8)
    check(pkg, x, dmask(chan), w, chan, win=win, what=(name, "chan"))


# ---- cap --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 1, 700), (64, 1, 520), (4, 2, 1100)])
def test_cap(eng, pkg, shape):
    a = bits_data(shape, 31)
    x = put(eng, a)
    N = a.size
    rng = np.random.default_rng(32)
    m = (rng.random(shape) < 0.3).astype(np.uint8) * 255
    md = dmask(m)
    tile = eng.hits_plan(x, md)["tile_elems"]
    assert N > 2 * tile
    total, idx, val = hits_ref(a, m)
    at_tile1 = int((idx < tile).sum())       # the list offset of tile 1
    at_tile2 = int((idx < 2 * tile).sum())
    mid_wave = int((idx < tile + 30).sum())  # inside the first wave's first step of tile 1
    for cap in (0, 1, 2, mid_wave, at_tile1 - 1, at_tile1, at_tile1 + 1, at_tile2, total - 1, total,
                total + 5):
        check(pkg, x, md, a, m, cap=cap, what=(shape, cap))
    # idx alone, val alone, neither (count-only with a cap)
    t, gi, gv = raw(pkg, x, md, shape, total, idx=True, val=False)
    assert t == total and gv is None and np.array_equal(gi, idx)
    t, gi, gv = raw(pkg, x, md, shape, 17, idx=False, val=True)
    assert t == total and gi is None and np.array_equal(gv, val[:17].view(np.uint32))
    assert raw(pkg, x, md, shape, 17, idx=False, val=False)[0] == total
    assert eng.hits_plan(x, md, maxhits=0)["launches"] == 2
    h = eng.hits(x, md, maxhits=0)
    assert h["total"] == total and h["index"].numel() == 0 and h["value"].numel() == 0


# ---- the scan's chunks, the doubled tile, determinism -------------------------------------
def test_scan_loops_over_chunks(eng, pkg):
    shape = (6, 1, 400000)   # 2344 tiles of 1024: two passes of the scan workgroup
    a = bits_data(shape, 41)
    x = put(eng, a)
    rng = np.random.default_rng(42)
    m = (rng.random(shape) < 0.01).astype(np.uint8)
    m[5, 0, -1] = m[0, 0, 0] = 1
    md = dmask(m)
    p = eng.hits_plan(x, md)
    assert p["scan_chunks"] == 2 and p["tiles"] > 2048 and p["tile_elems"] == 1024
    total = check(pkg, x, md, a, m)
    # determinism: the same call twice gives byte-identical lists
    r1, r2 = raw(pkg, x, md, shape, total), raw(pkg, x, md, shape, total)
    assert r1[0] == r2[0] and r1[1].tobytes() == r2[1].tobytes()
    assert r1[2].tobytes() == r2[2].tobytes()
    # a cut in the second chunk's tiles
    check(pkg, x, md, a, m, cap=total - 3)
    every = np.ones((1, 1, 1), np.uint8)   # every sample, through the row form
    assert eng.hits_plan(x, dmask(every))["mask_loads"] == "row"
    check(pkg, x, dmask(every), a, every, cap=5000)


def test_doubled_tile(eng, pkg):
    shape = (3, 1, 2800000)  # 8.4M elements: more than 8192 tiles of 1024, so tiles of 2048
    a = bits_data(shape, 43)
    x = put(eng, a)
    rng = np.random.default_rng(44)
    m = (rng.random(shape) < 1e-3).astype(np.uint8)
    m[2, 0, -1] = 1
    md = dmask(m)
    p = eng.hits_plan(x, md)
    assert p["tile_elems"] == 2048 and 4096 < p["tiles"] <= 8192 and p["scan_chunks"] == 3
    check(pkg, x, md, a, m)
    spec = np.zeros((1, 1, shape[2]), np.uint8)   # bad spectra: rows counted by their one byte
    spec[0, 0, rng.integers(0, shape[2], 50)] = 1
    check(pkg, x, dmask(spec), a, spec)


# ---- a stream of the caller's ---------------------------------------------------------------
def test_non_current_stream(eng, pkg):
    """hits and band_hits on a torch stream that is not the current one: the
    launches go there, and total is read only after that stream has drained."""
    import torch

    shape = (64, 2, 300)   # three tiles of the 16-flag form
    banks = [bits_data(shape, 80 + b) for b in range(2)]
    xs = [put(eng, b) for b in banks]
    cat = np.asfortranarray(np.concatenate(banks, axis=0))
    rng = np.random.default_rng(83)
    m = (rng.random(cat.shape) < 0.1).astype(np.uint8)
    md, md0 = dmask(m), dmask(m[:64])
    torch.cuda.synchronize()   # the inputs were made on the current stream
    s = torch.cuda.Stream()
    assert s != torch.cuda.current_stream()
    for mh in (None, 0, 50, 10 ** 6):
        for got, (total, idx, val) in ((eng.hits(xs[0], md0, maxhits=mh, stream=s),
                                        hits_ref(banks[0], m[:64])),
                                       (eng.band_hits(xs, md, maxhits=mh, stream=s),
                                        hits_ref(cat, m)),
                                       (eng.hits(xs[1], dmask(m[64:]), maxhits=mh,
                                                 stream=int(s.cuda_stream)),
                                        hits_ref(banks[1], m[64:]))):
            n = total if mh is None else min(mh, total)
            assert got["total"] == total and total > 50
            assert np.array_equal(got["index"].cpu().numpy(), idx[:n])
            assert np.array_equal(got["value"].cpu().numpy().view(np.uint32),
                                  val[:n].view(np.uint32))
    assert torch.cuda.current_stream() != s   # (the caller's current stream is left as it was)


def test_host_masks_arrive_channel_fastest(eng, pkg):
    """worker.getflagged's host masks reach the device in the window's layout, in
    whatever order the host array lies: a dense mask keeps the wide loads."""
    shape = (64, 2, 9)
    x = put(eng, bits_data(shape, 90))
    m = (np.random.default_rng(91).random(shape) < 0.3)
    for host in (np.ascontiguousarray(m), np.asfortranarray(m), m.astype(np.uint8),
                 np.asfortranarray(m.astype(np.uint8))[:, ::-1][:, ::-1]):
        t = pkg.worker._mask_to_device(host, "cuda:0")
        assert tuple(t.shape) == shape and t.stride() == (1, 64, 128)
        assert np.array_equal(t.cpu().numpy() != 0, m)
        p = eng.hits_plan(x, t)
        assert (p["mask_loads"], p["flags_per_load"]) == ("wide", 16)
    t = pkg.worker._mask_to_device(np.zeros((64, 1, 1), bool), "cuda:0")
    assert tuple(t.shape) == (64, 1, 1) and eng.hits_plan(x, t)["flags_per_load"] == 16


# ---- bands ------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [6, 16])
def test_band_is_the_vcat(eng, pkg, nc):
    shape = (nc, 2, 70)
    banks = [bits_data(shape, 50 + b) for b in range(3)]
    xs = [put(eng, b) for b in banks]
    cat = np.asfortranarray(np.concatenate(banks, axis=0))
    rng = np.random.default_rng(53)
    m = (rng.random(cat.shape) < 0.2).astype(np.uint8)
    m[:, 1, 3] = 0
    m[[1, nc + 2, 2 * nc + 3], 1, 3] = 1   # hits in every bank of one row, in bank order
    for mm, odd in ((m, False), (m, True), (m[:, :1, :1].copy(), False)):
        md = dmask(mm, odd)
        total, idx, val = hits_ref(cat, mm)
        got = raw(pkg, xs, md, cat.shape, total + 2)
        assert got[0] == total and np.array_equal(got[1], idx)
        assert np.array_equal(got[2], val.view(np.uint32))
        h = eng.band_hits(xs, md, maxhits=7)
        assert h["total"] == total and np.array_equal(h["index"].cpu().numpy(), idx[:7])
        assert np.array_equal(h["value"].cpu().numpy().view(np.uint32), val[:7].view(np.uint32))
    row = [k for k in hits_ref(cat, m)[1] if (k // (3 * nc)) == 1 + 2 * 3]
    assert [k % (3 * nc) for k in row] == [1, nc + 2, 2 * nc + 3]
    # a window of the banks
    win = [1, nc - 2, 1, 0, 2, 1, 69, 35, -2]
    wcat = np.asfortranarray(np.concatenate([window(b, win) for b in banks], axis=0))
    mw = (rng.random(wcat.shape) < 0.3).astype(np.uint8)
    total, idx, val = hits_ref(wcat, mw)
    got = raw(pkg, xs, dmask(mw), wcat.shape, total, win=win)
    assert got[0] == total and np.array_equal(got[1], idx)
    assert np.array_equal(got[2], val.view(np.uint32))


# ---- through the layers --------------------------------------------------------------------
def test_host_entry_point(eng):
    a = bits_data((40, 2, 12), 60)
    win = [3, 32, 1, 0, 2, 1, 11, 12, -1]
    w = np.asfortranarray(window(a, win))
    rng = np.random.default_rng(61)
    for m in ((rng.random(w.shape) < 0.3).astype(np.uint8) * 2, rng.random(w.shape) < 0.5,
              (rng.random((32, 1, 1)) < 0.5).astype(np.uint8), np.zeros(w.shape, np.uint8),
              (rng.random((1, 1, 12)) < 0.5).astype(np.uint8)):
        total, idx, val = hits_ref(w, m)
        for mh in (None, 0, 3, total + 4):
            r = eng.hits_host(np.asfortranarray(a), m, maxhits=mh, win=win)
            n = total if mh is None else min(mh, total)
            assert r["total"] == total and r["index"].dtype == np.int64
            assert np.array_equal(r["index"], idx[:n])
            assert np.array_equal(r["value"].view(np.uint32), val[:n].view(np.uint32))


def spiky(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(100, 110, shape).astype(np.float32)
    a[rng.random(shape) < 0.02] = 255.0
    a[rng.random(shape) < 0.01] = 3.0
    return a


def hits_want(W, data, idxs, win, n, axis, nsigma, maxhits):
    """gethits' dict from getoutliers' mask and planes and the restatement."""
    o = W.getoutliers(data, idxs, n=n, axis=axis, nsigma=nsigma, mask=True)
    w = np.asfortranarray(window(data, win))
    total, idx, val = hits_ref(w, o["mask"], maxhits)
    assert np.array_equal(hits_ref(w, o["mask"])[1], np.flatnonzero(o["mask"].ravel(order="F")))
    c, i, t = np.unravel_index(idx, w.shape, order="F")
    nb = n or w.shape[2]
    blk = (c // nb, i, t) if axis == 0 else (c, i, t // nb)
    return {"total": total, "channel": c, "if": i, "time": t, "value": val,
            "snr": snr_ref(val, o["median"][blk], o["mad"][blk]), "median": o["median"],
            "mad": o["mad"], "count": o["count"]}


def same_dict(got, want, host):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        g = got[k] if isinstance(got[k], int) else host(got[k])
        if isinstance(v, int):
            assert g == v, k
        else:
            assert g.shape == v.shape and g.tobytes() == v.astype(g.dtype).tobytes(), k


def test_getflagged_and_gethits(eng, pkg, tmp_path):
    import torch

    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = spiky((64, 2, 40), 70)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    h5 = str(tmp_path / "raw.rawspec.0000.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(h5, dict(foff=-1.0, nfpc=64), data)
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    w = np.asfortranarray(window(data, win))
    rng = np.random.default_rng(71)
    m = (rng.random(w.shape) < 0.2).astype(np.uint8)
    bad = (rng.random((32, 1, 1)) < 0.2).astype(np.uint8)
    x = put(eng, data)
    for src in (data, x, fil, h5):
        dev = isinstance(src, torch.Tensor)
        host = (lambda t: t.cpu().numpy() if t.dim() == 1 else eng.fb_to_numpy(t)) if dev \
            else (lambda t: t)
        for mk in (m, bad, m != 0, dmask(m)):
            mh = mk.cpu().numpy() if isinstance(mk, torch.Tensor) else mk
            for cap in (None, 9):
                got = W.getflagged(src, idxs, mask=mk, maxhits=cap)
                assert all(isinstance(v, (torch.Tensor if dev else np.ndarray, int))
                           for v in got.values())
                total, idx, val = hits_ref(w, mh, cap)
                c, i, t = np.unravel_index(idx, w.shape, order="F")
                same_dict(got, {"total": total, "index": idx, "channel": c, "if": i, "time": t,
                                "value": val}, host)
        for axis, n, ns, cap in ((2, 16, 3.0, None), (0, 8, 3.0, 11), (2, None, 3.0, None)):
            got = W.gethits(src, idxs, n=n, axis=axis, nsigma=ns, maxhits=cap)
            want = hits_want(W, data, idxs, win, n, axis, ns, cap)
            assert want["total"] > 0 and got["snr"].dtype in (np.float64, torch.float64)
            same_dict(got, want, host)
        got = W.gethits(src)  # the defaults: the whole time range, 5 mads, every hit
        same_dict(got, hits_want(W, data, (C, C, C), None, None, 2, 5.0, None), host)
    parts = pkg.GBT.gethits([0, 0], [fil, h5], idxs, n=16, nsigma=3.0, maxhits=20)
    assert len(parts) == 2
    for p in parts:
        same_dict(p, hits_want(W, data, idxs, win, 16, 2, 3.0, 20), lambda t: t)
    parts = pkg.GBT.getflagged([0, 0], [fil, h5], idxs, mask=m)
    total, idx, val = hits_ref(w, m)
    for p in parts:
        assert p["total"] == total and np.array_equal(p["index"], idx)
        assert p["value"].tobytes() == val.tobytes()
