"""Every reachable instantiation of stats.hip and tstats.hip on planted blocks.

For each row of tests/stat_cases.py (a small call that
tools/stat_launch_record.cpp says starts one entry point of the two files;
tests/test_stat_reach_host.py holds the table to the dispatcher), on the blocks
of tests/stat_planted.py (built by key structure: the pass at which two ranks
part, tie runs under a finite, an infinite and a NaN key, one / two / many
digits, every top byte, rank sets in one, five and sixteen slots, paired and
zero deviations, Inf and NaN blocks, middle subnormals with inexact halves): the plan the library reports on this
device is the recorded one (which ties the recorder's restatement of api.hip to
the library); the call of the row's op through the engine (the band entries for
more than one bank) into a slab of sentinels writes every element of the result
and nothing else; and the result is

  median, mad     the bits of mad_ref.median_ref / mad_ref;
  quantile        the bits of quantile_ref at the row's p and at both clamp ends;
  quantiles       per plane the bits of quantile_ref and of the single-p call;
  outliers        the bits of outliers_ref's median and mad, its count and its
                  mask, at nsigma 5, at 0 and at 1e300 (a threshold of Inf), the
                  first through the ABI into guarded slabs, the others through
                  engine.outliers (which allocates its own results);
  var, std        the Float64 two-pass value within RTOL = 1e-5, the Float32
                  bound test_gpu_stats.py and test_gpu_tstat.py state, on their
                  kind of data (finite, of moderate size); a constant block is
                  exactly 0.0.  A var row also runs std and the other way round
                  (the op is a run-time argument of one entry point).

The module reads nothing outside the repository and needs no compiler.
"""
from __future__ import annotations

import numpy as np
import pytest

import stat_cases as sc
import stat_planted as sp
from conftest import same_bits
from mad_ref import blocks, mad_ref, median_ref, window
from outliers_ref import outliers_ref
from quantile_ref import quantile_ref

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # test_gpu_stats.py / test_gpu_tstat.py
GUARD = 64   # elements before and after every result
SENTINEL = -7777.25
NSIGMAS = (5.0, 0.0, 1e300)


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()  # loud failure if libbldp_hip.so is missing
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == sc.NUM_CUS, "the plans of tests/stat_cases.py were recorded for %d CUs, this " \
        "device reports %d: the moments' tiles and chunks differ, so would the plan assertions" % (
            sc.NUM_CUS, cus)
    return pkg.engine


class Slab:
    """A Julia-order result of `dims` (and K planes) between two guards."""

    def __init__(self, dims, planes=None, dtype="float32"):
        import torch

        self.n = int(np.prod(dims)) * (planes or 1)
        self.sent = SENTINEL if dtype == "float32" else 0x5a
        self.t = torch.full((2 * GUARD + self.n,), self.sent, dtype=getattr(torch, dtype),
                            device="cuda:0")
        body = self.t[GUARD:GUARD + self.n]
        nc, ni, nt = dims
        self.out = body.view(nt, ni, nc).permute(2, 1, 0) if planes is None else \
            body.view(planes, nt, ni, nc).permute(3, 2, 1, 0)

    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def numpy(self, eng, msg, written=True):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all(), \
            (msg, "wrote outside its result")
        if written:
            assert (h[GUARD:GUARD + self.n] != self.sent).all(), \
                (msg, "left elements of its result unwritten")
        return eng.fb_to_numpy(self.out)


def out_dims(case):
    w = sc.window(case)
    n = max(case.n, 1)
    nc, ni, nt = (w[1] // n, w[4], w[7]) if case.axis == 0 else (w[1], w[4], w[7] // n)
    return (case.nbank * nc, ni, nt)


def cat(parts):
    """The vcat of the banks' results."""
    return np.asfortranarray(np.concatenate(parts, axis=0))


def device_plan(eng, case, x):
    """The ten plan words of one bank on this device, paths as their codes."""
    win = None if case.window is None else list(case.window)
    op = sc.kind(case)
    if op == "quantile":
        d = eng.quantile_plan(x, case.n, sc.probs(case)[0], case.axis, win)
    elif op == "quantiles":
        d = eng.quantiles_plan(x, case.n, sc.probs(case), case.axis, win)
    elif op == "outliers":
        d = eng.outliers_plan(x, case.n, case.axis, win, sc.mask(case))
    elif case.axis == 0:
        d = eng.plan(x, case.n, 1, op, win)
    else:
        d = eng.tstat_plan(x, case.n, op, win)
    paths = sc.PATHS0 if case.axis == 0 else sc.PATHS2
    words = [{v: k for k, v in paths.items()}[d["path"]]] + list(d.values())[1:]
    return tuple(words + [0] * (10 - len(words)))


def run_plain(eng, case, xs, op, win, msg):
    s = Slab(out_dims(case))
    if case.axis == 0:
        eng.reduce(xs[0], case.n, 1, op, win, out=s.out) if case.nbank == 1 else \
            eng.band_reduce(xs, case.n, 1, op, win, out=s.out)
    else:
        eng.tstat(xs[0], case.n, op, win, out=s.out) if case.nbank == 1 else \
            eng.band_tstat(xs, case.n, op, win, out=s.out)
    return s.numpy(eng, (msg, op))


def moments_ref(a, n, win, axis, std):
    """The Float64 two-pass value (test_gpu_stats.var_ref / test_gpu_tstat.var_ref)."""
    R = blocks(a, n, win, axis).astype(np.float64)
    m = R.sum(axis=0) / n
    v = ((R - m) ** 2).sum(axis=0) / (n - 1)
    return np.asfortranarray(np.moveaxis(np.sqrt(v) if std else v, 0, axis))


def check_moments(eng, case, banks, carried, xs, win, msg):
    const = {np.float32(3.0000001), np.float32(1e9)}
    for op in ("var", "std"):
        got = run_plain(eng, case, xs, op, win, msg)
        if case.n < 2:  # fqav of n <= 1: the window itself
            assert same_bits(got, cat([window(a, win) for a in banks])), (msg, op)
            continue
        want = cat([moments_ref(a, case.n, win, case.axis, op == "std") for a in banks])
        err = np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)
        print("%s %s: max rel err %.3g" % (sc.case_id(case), op, err[want > 0].max(initial=0.0)))
        assert got.dtype == np.float32 and got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=str((msg, op)))
        if {"const", "const_big"} <= set(carried):  # a constant block: exactly 0.0
            R = [blocks(a, case.n, win, case.axis) for a in banks]
            mn = cat([np.moveaxis(r.min(axis=0), 0, case.axis) for r in R])
            mx = cat([np.moveaxis(r.max(axis=0), 0, case.axis) for r in R])
            flat = (mn == mx) & np.isin(mn, list(const))
            assert flat.sum() >= 2 and (got[flat] == 0.0).all() and \
                not np.signbit(got[flat]).any(), (msg, op, "constant blocks")


def check_quantile(eng, case, banks, xs, win, msg):
    for p in sp.quantile_probs(case):
        s = Slab(out_dims(case))
        if case.nbank == 1:
            eng.quantile(xs[0], case.n, p, case.axis, win, out=s.out)
        else:
            eng.band_quantile(xs, case.n, p, case.axis, win, out=s.out)
        got = s.numpy(eng, (msg, p))
        want = cat([quantile_ref(a, case.n, p, win, case.axis) for a in banks])
        assert same_bits(got, want), (msg, p, mismatch(got, want))


def check_quantiles(eng, case, banks, xs, win, msg):
    ps = sc.probs(case)
    s = Slab(out_dims(case), planes=len(ps))
    if case.nbank == 1:
        eng.quantiles(xs[0], case.n, ps, case.axis, win, out=s.out)
    else:
        eng.band_quantiles(xs, case.n, ps, case.axis, win, out=s.out)
    got = s.numpy(eng, msg)
    assert got.shape == out_dims(case) + (len(ps),)
    for k, p in enumerate(ps):
        want = cat([quantile_ref(a, case.n, p, win, case.axis) for a in banks])
        assert same_bits(got[..., k], want), (msg, "plane", k, p, mismatch(got[..., k], want))
        one = eng.quantile(xs[0], case.n, p, case.axis, win) if case.nbank == 1 else \
            eng.band_quantile(xs, case.n, p, case.axis, win)
        assert same_bits(got[..., k], eng.fb_to_numpy(one)), (msg, "the single-p call", k, p)


def check_outliers(pkg, eng, case, banks, xs, win, msg):
    import torch

    w = sc.window(case)
    mdims = (case.nbank * w[1], w[4], w[7])
    dims = out_dims(case)
    for ns in NSIGMAS:
        refs = [outliers_ref(a, case.n, ns, win, case.axis) for a in banks]
        want = [cat([r[k] for r in refs]) for k in range(4)]
        if ns == NSIGMAS[0]:  # the ABI, into guarded slabs
            L = pkg._lib.lib()
            slabs = [Slab(dims), Slab(dims), Slab(dims, dtype="int32"),
                     Slab(mdims, dtype="uint8") if sc.mask(case) else None]
            ptrs = [s.ptr() if s else None for s in slabs]
            sp_ = pkg._lib.stream_ptr()
            if case.nbank == 1:
                wa, keep = eng._win_args(xs[0], win)
                rc = L.bldp_outliers_f32(*wa, case.axis, case.n, ns, *ptrs, dims[0],
                                         dims[0] * dims[1], sp_)
            else:
                _, nb, bp, geo = eng._banks(xs)
                keep, wp = eng._win_ptr(win, tuple(xs[0].shape))
                rc = L.bldp_band_outliers_f32(nb, bp, *geo, wp, case.axis, case.n, ns, *ptrs, sp_)
            pkg._lib.check(rc, "bldp_outliers_f32")
            torch.cuda.synchronize()
            got = [s.numpy(eng, (msg, "outliers", k), written=k < 2) if s else None
                   for k, s in enumerate(slabs)]
        else:
            r = eng.outliers(xs[0], case.n, case.axis, ns, win, sc.mask(case)) \
                if case.nbank == 1 else eng.band_outliers(xs, case.n, case.axis, ns, win,
                                                          sc.mask(case))
            got = [eng.fb_to_numpy(r[k]) if k in r else None
                   for k in ("median", "mad", "count", "mask")]
        assert same_bits(got[0], want[0]), (msg, ns, "median", mismatch(got[0], want[0]))
        assert same_bits(got[1], want[1]), (msg, ns, "mad", mismatch(got[1], want[1]))
        assert (got[2].astype(np.int64) == want[2].astype(np.int64)).all(), (msg, ns, "count")
        if sc.mask(case):
            assert got[3].dtype == np.uint8 and got[3].shape == want[3].shape
            assert (got[3] == want[3]).all(), (msg, ns, "mask", int((got[3] != want[3]).sum()))


def mismatch(got, want):
    """Where two arrays differ in bits, for the message."""
    g = np.ascontiguousarray(got).view(np.uint32)
    w = np.ascontiguousarray(want).view(np.uint32)
    at = np.argwhere(g != w)
    return "%d differ, first at %s: got %r want %r" % (
        len(at), at[0].tolist() if len(at) else None,
        got[tuple(at[0])] if len(at) else None, want[tuple(at[0])] if len(at) else None)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_case(pkg, eng, case):
    banks, carried = sp.build(case)
    assert carried, sc.case_id(case)
    xs = [eng.fb_from_numpy(a, device="cuda:0") for a in banks]
    win = None if case.window is None else list(case.window)
    msg = sc.case_id(case)
    assert device_plan(eng, case, xs[0]) == case.plan, msg
    op = sc.kind(case)
    if op in ("var", "std"):
        check_moments(eng, case, banks, carried, xs, win, msg)
    elif op in ("median", "mad"):
        ref = median_ref if op == "median" else mad_ref
        got = run_plain(eng, case, xs, op, win, msg)
        want = cat([ref(a, case.n, win, case.axis) for a in banks])
        assert got.dtype == np.float32 and same_bits(got, want), (msg, mismatch(got, want))
        if "inf_half" in carried:  # (the NaN and Inf blocks are there)
            assert np.isnan(want).any() and (op == "mad" or np.isinf(want).any())
    elif op == "quantile":
        check_quantile(eng, case, banks, xs, win, msg)
    elif op == "quantiles":
        check_quantiles(eng, case, banks, xs, win, msg)
    else:
        check_outliers(pkg, eng, case, banks, xs, win, msg)
