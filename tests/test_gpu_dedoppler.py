"""GPU: the dedoppler against the NumPy restatement (tests/dedoppler_ref.py), bit
for bit: best bits, drift and sums bits on signed, gamma-like non-integer data and
on the special values; every case of tests/dedoppler_cases.py with the plan it must
take; the outputs' strides and null forms; the band; the host and worker forms from
SIGPROC and FBH5 files; getdrifthits on planted drifting lines."""
from __future__ import annotations

import numpy as np
import pytest

import dedoppler_cases as dc
from dedoppler_ref import bits, dedoppler_ref, off, offsets, scan_order
from mad_ref import window
from outliers_ref import outliers_ref
from test_gpu_histogram import signed
from test_gpu_masked import put

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def bit_equal(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def host(eng, r):
    return {k: eng.fb_to_numpy(t) if t.dim() == 3 else eng.planes_to_numpy(t) for k, t in r.items()}


def check(eng, a, D, T, seg=0, win=None, x=None, tag=""):
    """One window on the GPU against the restatement, with and without the sums,
    twice; returns the restatement."""
    import torch

    x = put(eng, a) if x is None else x
    s, best, drift = dedoppler_ref(window(a, win), D, T, seg)
    r = eng.dedoppler(x, D, T, seg, win=win, sums=True)
    assert r["best"].dtype == torch.float32 and r["drift"].dtype == torch.int32
    g = host(eng, r)
    assert bit_equal(g["sums"], s), tag
    assert bit_equal(g["best"], best), tag
    assert g["drift"].shape == drift.shape and np.array_equal(g["drift"], drift), tag
    r2 = eng.dedoppler(x, D, T, seg, win=win)
    assert set(r2) == {"best", "drift"}
    g2 = host(eng, r2)
    assert bit_equal(g2["best"], best) and np.array_equal(g2["drift"], drift), tag
    g3 = host(eng, eng.dedoppler(x, D, T, seg, win=win, sums=True))
    assert all(g3[k].tobytes() == g[k].tobytes() for k in g), tag
    return s, best, drift


@pytest.mark.parametrize("c", dc.CASES, ids=dc.case_id)
def test_case_against_the_restatement(eng, pkg, c):
    a = signed(dc.array_shape(c), 100 + dc.CASES.index(c))
    x, win = put(eng, a), dc.window(c)
    p = eng.dedoppler_plan(x, c.D, c.T, c.seg, win=win)
    assert (p["path"], p["vector_loads"], p["tile_channels"]) == c.plan, p
    assert p["drifts_per_group"] == dc.GROUP and p["workspace_bytes"] == 0
    assert set(p) == set(eng.DEDOPPLER_PLAN_KEYS)
    check(eng, a, c.D, c.T, c.seg, win, x=x, tag=dc.case_id(c))


def test_zero_drift_is_the_sequential_float32_sum(eng):
    a = signed((300, 2, 34), 7)
    _, best, drift = check(eng, a, 0, 17)
    acc = np.zeros((300, 2, 2), np.float32)
    for b in range(2):
        for t in range(17):
            acc[:, :, b] = acc[:, :, b] + a[:, :, b * 17 + t]
    assert bit_equal(best, acc) and (drift == 0).all()


def test_special_values(eng):
    T, D = 16, 6
    # a NaN with a payload at one (c, t): exactly the sums whose path passes it are
    # NaN, best carries the payload, drift is the first such in scan order
    a = signed((300, 1, T), 11)
    nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    a[140, 0, 9] = nan
    x = put(eng, a)
    g = host(eng, eng.dedoppler(x, D, T, sums=True))
    s, best, drift = check(eng, a, D, T, x=x)
    tab = offsets(D, T)
    for c in range(300):
        for k in range(2 * D + 1):
            assert np.isnan(g["sums"][c, 0, 0, k]) == (c + tab[k, 9] == 140)
    hit = np.isnan(g["best"][:, 0, 0])
    assert hit.sum() == len({int(tab[k, 9]) for k in range(2 * D + 1)})
    assert (bits(g["best"][hit]) == 0x7FC12345).all()
    for c in np.flatnonzero(hit):
        first = next(d for d in scan_order(D) if c + off(d, 9, T) == 140)
        assert g["drift"][c, 0, 0] == first
    # +Inf and -Inf on one path give NaN (its sign is the adder's own: compared as NaN)
    b = signed((300, 1, T), 12)
    b[100, 0, 0], b[100, 0, 1] = INF, -INF
    g = host(eng, eng.dedoppler(put(eng, b), D, T, sums=True))
    s, best, drift = dedoppler_ref(b, D, T)
    made = np.isnan(s)
    assert made[100, 0, 0, D] and np.array_equal(np.isnan(g["sums"]), made)
    assert np.array_equal(bits(g["sums"])[~made], bits(s)[~made])
    nb = np.isnan(best)
    assert nb[100, 0, 0] and np.array_equal(np.isnan(g["best"]), nb)
    assert np.array_equal(bits(g["best"])[~nb], bits(best)[~nb])
    assert np.array_equal(g["drift"], drift)
    # an all -0.0 window gives +0.0; ties on a flat window give drift 0
    z = host(eng, eng.dedoppler(put(eng, np.full((300, 2, T), -0.0, np.float32)), D, T, sums=True))
    assert (bits(z["best"]) == 0).all() and (bits(z["sums"]) == 0).all() and (z["drift"] == 0).all()
    f = host(eng, eng.dedoppler(put(eng, np.full((300, 2, 2 * T), 2.5, np.float32)), D, T, seg=50))
    assert (f["drift"] == 0).all() and (f["best"] == 2.5 * T).all()
    # infinities and the largest finite values elsewhere: IEEE results stand
    e = signed((300, 1, T), 13)
    e[7, 0, 3], e[200, 0, 5], e[250, 0, 0], e[251, 0, 1] = INF, -INF, 3.0e38, 3.0e38
    check(eng, e, D, T, seg=150)


@pytest.mark.parametrize("c0,d", [(96, -8), (96, 0), (96, 8), (64, 8), (127, -8), (299, -8)])
def test_planted_line(eng, c0, d):
    """A line at d = -D, 0, +D away from and at a segment edge."""
    T, D, seg = 16, 8, 64
    a = signed((300, 1, T), 21) * np.float32(0.01)
    for t in range(T):
        a[c0 + off(d, t, T), 0, t] += np.float32(1000.25)
    _, best, drift = check(eng, a, D, T, seg)
    lo = c0 // seg * seg
    assert lo + int(np.argmax(best[lo:lo + seg, 0, 0])) == c0 and drift[c0, 0, 0] == d


def test_outputs_strided_and_single(eng, pkg):
    import torch

    nc, ni, nt, T, D, seg = 300, 2, 32, 16, 5, 100
    K, nb = 2 * D + 1, nt // T
    a = signed((nc, ni, nt), 31)
    x = put(eng, a)
    s, best, drift = dedoppler_ref(a, D, T, seg)
    L = pkg._lib.lib()
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    ld_i, ld_t = nc + 8, (nc + 8) * ni + 12
    ld_q = ld_t * nb + 20
    fb = torch.full((ld_t * nb + 64,), -7.0, device="cuda:0")
    fd = torch.full((ld_t * nb + 64,), -7, dtype=torch.int32, device="cuda:0")
    fs = torch.full((ld_q * K + 64,), -7.0, device="cuda:0")

    def rows(buf, planes=None):
        h = buf.cpu().numpy()
        body = np.full(h.shape, True)
        out = []
        for q in range(planes or 1):
            o = np.empty((nc, ni, nb), h.dtype)
            for b in range(nb):
                for i in range(ni):
                    st = q * ld_q * (planes is not None) + b * ld_t + i * ld_i
                    o[:, i, b] = h[st:st + nc]
                    body[st:st + nc] = False
            out.append(o)
        assert (h[body] == -7).all()   # the sentinels between the rows
        return out[0] if planes is None else np.stack(out, axis=-1)

    def call(b, d, sm):
        pkg._lib.check(L.bldp_dedoppler_f32(ptr, nchan, nif, ntime, None, T, D, seg, b, d, sm, ld_i,
                                            ld_t, ld_q, None), "bldp_dedoppler_f32")
        torch.cuda.synchronize()

    # best / drift alone: the sums buffer keeps every sentinel
    call(fb.data_ptr(), fd.data_ptr(), None)
    assert bit_equal(rows(fb), best) and np.array_equal(rows(fd), drift)
    assert (fs == -7).all()
    # sums alone: best and drift keep theirs
    fb.fill_(-7.0)
    fd.fill_(-7)
    call(None, None, fs.data_ptr())
    assert bit_equal(rows(fs, K), s) and (fb == -7).all() and (fd == -7).all()
    # all three
    fs.fill_(-7.0)
    call(fb.data_ptr(), fd.data_ptr(), fs.data_ptr())
    assert bit_equal(rows(fb), best) and np.array_equal(rows(fd), drift) and bit_equal(rows(fs, K), s)


def test_band_is_the_vcat_of_its_banks(eng):
    nc, ni, nt, T, D, seg = 300, 2, 32, 16, 9, 64
    banks = [signed((nc, ni, nt), 40 + k) for k in range(3)]
    xs = [put(eng, b) for b in banks]
    for win in (None, [2, 260, 1, 0, 2, 1, 0, 32, 1]):
        got = host(eng, eng.band_dedoppler(xs, D, T, seg, win=win, sums=True))
        parts = [host(eng, eng.dedoppler(x, D, T, seg, win=win, sums=True)) for x in xs]
        refs = [dedoppler_ref(window(b, win), D, T, seg) for b in banks]
        for k, j in (("sums", 0), ("best", 1), ("drift", 2)):
            cat = np.concatenate([p[k] for p in parts], axis=0)
            want = np.concatenate([r[j] for r in refs], axis=0)
            if k == "drift":
                assert np.array_equal(got[k], cat) and np.array_equal(got[k], want)
            else:
                assert bit_equal(got[k], cat) and bit_equal(got[k], want), k
        two = host(eng, eng.band_dedoppler(xs, D, T, seg, win=win))
        assert set(two) == {"best", "drift"} and np.array_equal(two["drift"], got["drift"])


def test_host_worker_and_files(eng, pkg, tmp_path):
    import torch

    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = signed((64, 2, 40), 50)
    data[8::16] += np.float32(500.0)   # a DC spike in the middle of every coarse channel
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=16), data)
    # the host form against the device form and the restatement
    win = [3, 48, 1, 0, 2, 1, 39, 32, -1]
    r = eng.dedoppler_host(np.asfortranarray(data), 4, 8, 16, win=win, sums=True)
    s, best, drift = dedoppler_ref(window(data, win), 4, 8, 16)
    assert r["best"].flags.f_contiguous and r["drift"].dtype == np.int32
    assert bit_equal(r["sums"], s) and bit_equal(r["best"], best) and np.array_equal(r["drift"], drift)
    assert set(eng.dedoppler_host(np.asfortranarray(data), 4, 8, 16, win=win)) == {"best", "drift"}
    # the FBH5 header names nfpc = 16; the whole file, the whole time range
    got = W.getdedoppler(raw, maxdrift=3)
    s, best, drift = dedoppler_ref(data, 3, 40, 16)
    assert bit_equal(got["best"], best) and np.array_equal(got["drift"], drift)
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    x = put(eng, data)
    for src in (data, x, fil, raw):
        dev = isinstance(src, torch.Tensor)
        got = W.getdedoppler(src, idxs, maxdrift=5, tavby=16, nfpc=8, sums=True)
        assert all(isinstance(v, torch.Tensor if dev else np.ndarray) for v in got.values())
        got = host(eng, got) if dev else got
        s, best, drift = dedoppler_ref(window(data, win), 5, 16, 8)
        assert bit_equal(got["sums"], s) and bit_equal(got["best"], best)
        assert np.array_equal(got["drift"], drift)
        # nfpc = 0: the whole window one segment; despike: the DC bins patched first
        got = W.getdedoppler(src, idxs, maxdrift=5, tavby=16, nfpc=0)
        got = host(eng, got) if dev else got
        assert bit_equal(got["best"], dedoppler_ref(window(data, win), 5, 16)[1])
        w = window(data, [0, 64, 1, 0, 2, 1, 0, 32, 1]).copy()
        w[8::16] = w[7::16]
        got = W.getdedoppler(src, (C, C, J(1, 32)), maxdrift=5, tavby=16, nfpc=16, despike=True)
        got = host(eng, got) if dev else got
        assert bit_equal(got["best"], dedoppler_ref(w, 5, 16, 16)[1])
    assert bit_equal(eng.fb_to_numpy(x), data)   # despike worked on a copy
    parts = pkg.GBT.getdedoppler([0, 0], [fil, raw], idxs, maxdrift=5, tavby=16, nfpc=8)
    assert len(parts) == 2
    for p in parts:
        assert bit_equal(p["best"], dedoppler_ref(window(data, win), 5, 16, 8)[1])


def test_getdrifthits_lists_the_planted_lines(eng, pkg, tmp_path):
    import torch

    W = pkg.worker
    nc, T, D, nfpc, nsigma = 512, 16, 8, 128, 160.0
    planted = [(70, -8), (300, 0), (450, 5)]
    a = signed((nc, 1, T), 60) * np.float32(0.01)
    for c0, d in planted:
        for t in range(T):
            a[c0 + off(d, t, T), 0, t] += np.float32(30.5)
    # the condition: the restatement's best plane, flagged along its nc channels at nsigma
    # (a neighbour of a line holds up to 10 of its 16 samples: 0.62 of its excess), holds
    # the three planted channels and nothing else
    _, best, drift = dedoppler_ref(a, D, T, nfpc)
    med, mad, count, mask = outliers_ref(best, nc, nsigma, axis=0)
    assert sorted(np.flatnonzero(mask[:, 0, 0]).tolist()) == [c for c, _ in planted]
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=nc, nifs=1, nbits=32)
    fil = str(tmp_path / "guppi_59000_00002_VOYAGER1_0001.rawspec.0000.fil")
    pkg.readers.write_fil(fil, hdr, a)
    rates = eng.drift_rates(D, T, hdr["foff"], hdr["tsamp"])
    for src in (put(eng, a), a, fil):
        h = W.getdrifthits(src, maxdrift=D, tavby=T, nfpc=nfpc, n=nc, nsigma=nsigma)
        if isinstance(src, torch.Tensor):
            h = {k: v if isinstance(v, int) else v.cpu().numpy() for k, v in h.items()}
        assert h["total"] == 3
        assert list(zip(h["channel"].tolist(), h["drift"].tolist())) == planted
        assert h["if"].tolist() == [0, 0, 0] and h["time"].tolist() == [0, 0, 0]
        assert np.array_equal(bits(h["value"]), bits(best[[c for c, _ in planted], 0, 0]))
        assert (h["snr"] > nsigma).all()
        if isinstance(src, str):
            assert np.array_equal(h["drift_rate"], rates[np.array([d for _, d in planted]) + D])
        else:
            assert "drift_rate" not in h
    got = pkg.GBT.getdrifthits([0], [fil], maxdrift=D, tavby=T, nfpc=nfpc, n=nc, nsigma=nsigma,
                               maxhits=2)
    assert got[0]["total"] == 3 and got[0]["channel"].tolist() == [70, 300]
