"""GPU: fqavfunc / tavfunc quantiles(ps) of Float32 windows (csrc/stats.hip,
csrc/tstats.hip with the rank set of a QSet): every plane bit for bit against
the rule restated in NumPy (quantile_ref.py) for its p, and against the
single-p engine.quantile on the same tensor.  Every step of the rule is exactly
specified, so no tolerance applies; NaN results compare as NaN
(conftest.same_bits).

The data are test_gpu_quantile.py's: every block size on at least 11 blocks,
whole blocks planted with a NaN, a minority, half and a majority of +Inf, -Inf,
+-floatmax alternating, odd subnormals, +-0.0, one repeated value, and the
integers 0..3.  Block sizes are the smallest that reach each kernel form and
its edges."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from conftest import same_bits
from quantile_ref import quantile_ref, rank_weight
from test_gpu_quantile import (BELOW_ONE, chan_array, chan_shape, chan_windows, exact_p, put,
                               time_array, time_shape)

pytestmark = pytest.mark.gpu

QUARTILES = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def overlap_pair(n):
    """Two p's whose rank pairs overlap by one key: j = 1 and j = 2."""
    ps = (0.5 / (n - 1), 1.5 / (n - 1))
    assert [rank_weight(n, p)[0] for p in ps] == [1, 2]
    return ps


def same_ranks(n):
    """Two p's with the same ranks and different weights."""
    ps = (0.75 / (n - 1), 0.25 / (n - 1))
    (ja, ga), (jb, gb) = (rank_weight(n, p) for p in ps)
    assert ja == jb == 1 and ga > gb > 0.0
    return ps


def p_sets(n):
    e = exact_p(n)
    sets = [(0.3,), QUARTILES, (0.9, 0.1), (0.5, 0.5), (0.0, 1.0), (1e-300, BELOW_ONE),
            same_ranks(n),
            (max(float(np.nextafter(e, 0.0)), 0.0), e, min(float(np.nextafter(e, 1.0)), 1.0)),
            tuple(np.linspace(0.05, 0.95, 8)),   # 8 distinct: one full launch
            tuple(np.linspace(0.0, 1.0, 9))]     # 9: two launches into the one output
    if n >= 3:
        sets.append(overlap_pair(n))
    return sets


def check_planes(eng, x, a, n, ps, axis, win=None):
    got = eng.quantiles(x, n, ps, axis, win)
    h = eng.planes_to_numpy(got)
    assert h.dtype == np.float32 and h.ndim == 4 and h.shape[3] == len(ps)
    for k, p in enumerate(ps):
        want = quantile_ref(a, n, p, win, axis)
        assert h[..., k].shape == want.shape
        assert same_bits(h[..., k], want), (n, axis, ps, k, win)
        # ... and the single-p call's plane, itself a tensor as fb_empty makes it
        one = eng.quantile(x, n, p, axis, win)
        assert got[..., k].stride() == one.stride()
        assert same_bits(eng.fb_to_numpy(got[..., k]), eng.fb_to_numpy(one)), (n, axis, ps, k)
    return h


# ---------------------------------------------------------------------------
# the channel axis: sort (<= 64), register select (<= 4096; 100: no float4), stream

CHAN_F = [2, 3, 4, 5, 63, 64, 65, 100, 4096, 4099, 4100]
CHAN_PATH = {**{F: "median_sort" for F in CHAN_F[:6]}, 65: "median_select", 100: "median_select",
             4096: "median_select", 4099: "median_stream", 4100: "median_stream"}


@pytest.mark.parametrize("F", CHAN_F)
def test_fqav_quantiles_bits(eng, pkg, F):
    _, nco, ni, nt = chan_shape(F)
    a = chan_array(F, nco, ni, nt, F)
    x = put(eng, a)
    med = eng.plan(x, F, 1, "median")
    for ps in p_sets(F):
        if len(ps) <= 8:
            plan = eng.quantiles_plan(x, F, ps)
            assert plan["path"] == CHAN_PATH[F] == med["path"]
            assert {k: v for k, v in plan.items() if k not in ("ranks", "reads")} == med
            lows = {rank_weight(F, p)[0] - 1 for p in ps}
            assert plan["ranks"] == len(lows | {q + 1 for q in lows})
            assert plan["reads"] == (4 if F > 4096 else 1)  # never 4 K
            assert plan == eng.plan(x, F, 1, pkg.quantiles(ps))
        check_planes(eng, x, a, F, ps, 0)
    assert same_bits(eng.planes_to_numpy(eng.reduce(x, F, 1, pkg.quantiles(QUARTILES))),
                     eng.planes_to_numpy(eng.quantiles(x, F, QUARTILES)))


@pytest.mark.parametrize("F", [64, 4096, 4100])
def test_fqav_quantiles_windows(eng, F):
    """The big size of each form: a channel step of 2 (one dword per element),
    reversed channels, channel offset 3 (off a 16-byte boundary), nif = 2, and
    a time step of 2."""
    _, nco, ni, nt = chan_shape(F)
    a = chan_array(F, nco, ni, nt, F + 1)
    x = put(eng, a)
    nch = F * nco
    wins = chan_windows(F, nco)[1:] + [[3, F * (nco - 2), 1, 1, 1, 1, 0, 2, 2],
                                       [nch - 2, F * (nco // 2), -2, 0, 2, 1, 2, 2, -2]]
    for w in wins:
        check_planes(eng, x, a, F, (0.75, 0.1, 0.5), 0, w)


# ---------------------------------------------------------------------------
# the time axis: registers (<= 32), split

TIME_T = [2, 3, 5, 31, 32, 33, 272, 1024]


@pytest.mark.parametrize("T", TIME_T)
def test_tav_quantiles_bits(eng, pkg, T):
    path = "regs_median" if T <= 32 else "split_median"
    for nc in (8, 6):  # float4 columns, and one dword per lane
        _, _, ni, nb = time_shape(T, nc)
        a = time_array(T, nc, ni, nb, 100 * T + nc)
        x = put(eng, a)
        for ps in p_sets(T):
            if len(ps) <= 8:
                plan = eng.quantiles_plan(x, T, ps, 2)
                nlow = len({rank_weight(T, p)[0] for p in ps})
                assert plan["path"] == path and plan["channels_per_lane"] == (4 if nc == 8 else 1)
                assert plan["reads"] == plan["passes"] == (1 if T <= 32 else 1 + 4 * -(-nlow // 3))
                assert plan == eng.tstat_plan(x, T, pkg.quantiles(ps))
            check_planes(eng, x, a, T, ps, 2)
        assert same_bits(eng.planes_to_numpy(eng.tstat(x, T, pkg.quantiles(QUARTILES))),
                         eng.planes_to_numpy(eng.quantiles(x, T, QUARTILES, 2)))


@pytest.mark.parametrize("T", [32, 1024])
def test_tav_quantiles_windows(eng, T):
    """The big size of each form: reversed and stepped channels, channel offset
    3, nif = 2 and one IF of them, a time step of 2 and a reversed time range."""
    nc, ni, nb = 16, 2, 8
    a = time_array(T, nc, ni, nb, T + 5)
    x = put(eng, a)
    nt = T * nb
    wins = [[nc - 1, nc, -1, 0, ni, 1, T, T * (nb // 2), 1],
            [3, 8, 1, 1, 1, 1, 0, T * (nb // 2), 2],
            [nc - 2, nc // 2, -2, 0, ni, 1, nt - 1, T * (nb // 2), -2],
            [3, 12, 1, 0, ni, 1, 0, nt, 1]]
    for w in wins:
        check_planes(eng, x, a, T, (0.75, 0.1, 0.5, 0.1), 2, w)


# ---------------------------------------------------------------------------
# n <= 1, out=, the layers

def test_copy_out_and_errors(eng, pkg):
    import torch

    a = chan_array(8, 6, 2, 3, 3)  # (48, 2, 3)
    x = put(eng, a)
    for axis in (0, 2):
        for n in (1, 0):
            r = eng.quantiles(x, n, QUARTILES, axis)
            assert tuple(r.shape) == (48, 2, 3, 3)
            for k, p in enumerate(QUARTILES):  # what the scalar form copies, bit for bit
                assert same_bits(eng.fb_to_numpy(r[..., k]),
                                 eng.fb_to_numpy(eng.quantile(x, n, p, axis)))
        plan = eng.quantiles_plan(x, 1, QUARTILES, axis)
        assert plan["ranks"] == 0 and plan["reads"] == 1
    r = pkg.fqav(x, 1, pkg.quantiles((0.1, 0.9)))
    assert isinstance(r, torch.Tensor) and tuple(r.shape) == (48, 2, 3, 2)
    assert same_bits(eng.fb_to_numpy(r[..., 1]), a) and r[..., 0].stride() == x.stride()
    # out=: a 4-D tensor, here the middle planes of a larger one
    big = eng.planes_empty(6, 2, 3, 5, device="cuda:0")
    big.fill_(-7.0)
    r = eng.quantiles(x, 8, (0.9, 0.1, 0.5), 0, out=big[..., 1:4])
    torch.cuda.synchronize()
    h = eng.planes_to_numpy(big)
    assert r.data_ptr() == big[..., 1:4].data_ptr()
    assert (h[..., 0] == -7.0).all() and (h[..., 4] == -7.0).all()
    for k, p in enumerate((0.9, 0.1, 0.5)):
        assert same_bits(h[..., 1 + k], quantile_ref(a, 8, p))
    # nine planes into a caller's tensor: two launches
    ps = tuple(np.linspace(0, 1, 9))
    out = eng.planes_empty(48, 2, 1, 9, device="cuda:0")
    eng.quantiles(x, 3, ps, 2, out=out)
    assert same_bits(eng.planes_to_numpy(out)[..., 8], quantile_ref(a, 3, 1.0, axis=2))
    w = pkg.worker.getdata_device(x, fqavby=8, fqavfunc=pkg.quantiles(QUARTILES), out=big[..., :3])
    assert w.data_ptr() == big.data_ptr()
    assert same_bits(eng.planes_to_numpy(big)[..., 2], quantile_ref(a, 8, 0.75))
    for bad in (eng.planes_empty(6, 2, 3, 2, device="cuda:0"),
                eng.planes_empty(6, 2, 2, 3, device="cuda:0"), eng.fb_empty(6, 2, 3, device="cuda:0")):
        with pytest.raises(ValueError, match="out is"):
            eng.quantiles(x, 8, QUARTILES, 0, out=bad)
    with pytest.raises(TypeError, match="tavby"):
        eng.reduce(x, 2, 2, pkg.quantiles(QUARTILES))
    with pytest.raises(TypeError, match="Float32"):
        eng.reduce(x.to(torch.int16), 4, 1, pkg.quantiles(QUARTILES))
    with pytest.raises(TypeError, match="quantile"):
        eng.PreparedReduce(x, 2, 1, pkg.quantiles(QUARTILES))
    with pytest.raises(TypeError):
        eng.band_reduce_multi([x, x], 2, 1, pkg.quantiles(QUARTILES))
    with pytest.raises(pkg.DimensionMismatch):
        eng.quantiles(x, 5, QUARTILES)
    with pytest.raises(ValueError, match="quantile"):
        eng.quantiles(x, 2, (0.5, 1.5))


def test_band_and_host(eng, pkg):
    ps = (0.9, 0.25, 0.5)
    banks = [chan_array(64, 16, 2, 3, 30 + k) for k in range(3)]
    xs = [put(eng, b) for b in banks]
    for F in (64, 256):
        band = eng.planes_to_numpy(eng.band_quantiles(xs, F, ps))
        for k, p in enumerate(ps):
            want = np.concatenate([quantile_ref(b, F, p) for b in banks], axis=0)
            assert same_bits(band[..., k], want), (F, k)
            assert same_bits(band[..., k], eng.fb_to_numpy(eng.band_quantile(xs, F, p)))
        assert same_bits(eng.planes_to_numpy(eng.band_reduce(xs, F, 1, pkg.quantiles(ps))), band)
        host = eng.quantiles_host(banks[0], F, ps)
        assert host.flags.f_contiguous and same_bits(host, band[:band.shape[0] // 3])
        assert same_bits(eng.reduce_host(banks[0], F, 1, pkg.quantiles(ps)), host)
        assert same_bits(pkg.fqav(banks[0], F, pkg.quantiles(ps)), host)
    nine = tuple(np.linspace(0, 1, 9))
    band = eng.planes_to_numpy(eng.band_quantiles(xs, 64, nine))
    assert same_bits(band[..., 8], np.concatenate([quantile_ref(b, 64, 1.0) for b in banks], axis=0))
    assert same_bits(eng.quantiles_host(banks[1], 64, nine)[..., 7], quantile_ref(banks[1], 64, 0.875))
    win = [5, 512, 1, 1, 1, 1, 0, 2, 2]
    host = eng.quantiles_host(banks[0], 64, ps, 0, win)
    assert same_bits(host[..., 1], quantile_ref(banks[0], 64, 0.25, win))
    tb = [time_array(48, 12, 2, 4, 40 + k) for k in range(3)]
    ts = [put(eng, b) for b in tb]
    for T in (16, 48):
        band = eng.planes_to_numpy(eng.band_quantiles(ts, T, ps, 2))
        for k, p in enumerate(ps):
            want = np.concatenate([quantile_ref(b, T, p, axis=2) for b in tb], axis=0)
            assert same_bits(band[..., k], want), (T, k)
        assert same_bits(eng.planes_to_numpy(eng.band_tstat(ts, T, pkg.quantiles(ps))), band)
        host = eng.quantiles_host(tb[2], T, ps, 2)
        assert same_bits(host, band[24:])
        assert same_bits(eng.tstat_host(tb[2], T, pkg.quantiles(ps)), host)
    win = [1, 8, 1, 1, 1, 1, 191, 96, -2]  # a reversed time range
    host = eng.quantiles_host(tb[0], 16, ps, 2, win)
    assert same_bits(host[..., 0], quantile_ref(tb[0], 16, 0.9, win, axis=2))


def test_getdata_every_source(eng, pkg, orc, tmp_path):
    import torch

    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    ps = (0.75, 0.25, 0.5)
    q = pkg.quantiles(ps)
    data = chan_array(8, 8, 2, 40, 4)  # (64, 2, 40)
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    bs = str(tmp_path / "bs.rawspec.0002.h5")
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=64), data)
    pkg.fbh5.write_bslz4(bs, dict(foff=-1.0, nfpc=64), data, (8, 1, 64),
                         lambda blk: orc.np_bslz4_encode(blk, 512, lz4=orc.lz4_compress))
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    s1 = eng.fb_to_numpy(eng.reduce(put(eng, data), 2, 1, "sum"))

    def planes(r):
        if isinstance(r, torch.Tensor):
            assert r.is_cuda
            return eng.planes_to_numpy(r)
        assert r.dtype == np.float32 and r.flags.f_contiguous
        return r

    for src in (put(eng, data), data, raw, bs):
        got = planes(W.getdata(src, fqavby=8, fqavfunc=q))
        win8 = planes(W.getdata(src, idxs, 16, q))
        tav = planes(W.getdata(src, fqavby=2, fqavfunc="sum", tavby=8, tavfunc=q))
        tw = planes(W.getdata(src, idxs, tavby=16, tavfunc=q))
        for k, p in enumerate(ps):
            assert same_bits(got[..., k], quantile_ref(data, 8, p)), (type(src), k)
            assert same_bits(win8[..., k], quantile_ref(data, 16, p, win)), (type(src), k)
            assert same_bits(tav[..., k], quantile_ref(s1, 8, p, axis=2)), (type(src), k)
            assert same_bits(tw[..., k], quantile_ref(data, 16, p, win, axis=2)), (type(src), k)
        with pytest.raises(TypeError, match="tavby"):
            W.getdata(src, fqavby=8, fqavfunc=q, tavby=2)
        with pytest.raises(TypeError, match="tavfunc"):
            W.getdata(src, fqavby=8, fqavfunc=q, tavby=2, tavfunc="sum")
    parts = pkg.GBT.getdata([0, 0], [raw, bs], fqavby=8, fqavfunc=q)
    assert all(same_bits(p[..., 1], quantile_ref(data, 8, 0.25)) for p in parts)
    with pytest.raises(TypeError, match="engine.band_quantiles"):
        pkg.GBT.getband([0, 0], [raw, bs], fqavby=8, fqavfunc=q)


def test_plan_on_the_gpu_is_the_cpu_plan(eng, pkg):
    """quantiles_plan of a resident tensor against bldp_quantiles_plan_f32 with
    null pointers (the plan the CPU tests pin), on each path's shapes."""
    L = pkg._lib.lib()
    keys0 = ["path", "lanes_per_group", "time_split_waves", "float4_per_lane", "time_chunks",
             "workgroups", "workspace_bytes", "vec_out", "ranks", "reads"]
    keys2 = ["path", "channels_per_lane", "time_split_lanes", "passes", "workgroups",
             "workspace_bytes", "blocks", "channel_lanes", "ranks", "reads"]
    info = (ctypes.c_int64 * 10)()
    for axis, n, dims in ((0, 64, (128, 2, 3)), (0, 100, (200, 2, 3)), (0, 4100, (8200, 1, 2)),
                          (2, 16, (264, 2, 32)), (2, 272, (264, 2, 544)), (2, 272, (6, 1, 544))):
        x = eng.fb_empty(*dims, device="cuda:0")
        for ps in (QUARTILES, (0.3,), tuple(np.linspace(0.05, 0.95, 8))):
            arr = (ctypes.c_double * len(ps))(*ps)
            assert L.bldp_quantiles_plan_f32(None, *dims, None, axis, n, len(ps), arr, None,
                                             info) == 0
            cpu = dict(zip(keys0 if axis == 0 else keys2, [int(v) for v in info]))
            cpu["path"] = (pkg._lib.PATHS if axis == 0 else pkg._lib.TSTAT_PATHS)[cpu["path"]]
            assert eng.quantiles_plan(x, n, ps, axis) == cpu, (axis, n, ps)
