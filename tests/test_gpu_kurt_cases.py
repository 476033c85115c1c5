"""Every reachable instantiation of kurtosis.hip on planted rows.

For each case of tests/kurt_cases.py (a small call, with its plan options, that
tools/kurt_launch_record.cpp says starts one entry point of kurtosis.hip;
tests/test_kurt_reach_host.py holds the table to the dispatcher), on the rows
of tests/kurt_planted.py: the plan the library reports on this device is the
recorded one (which ties the recorder's restatement of kurt_setup and mom_plan
to the library); the call of the case's order and tblock, through the ABI into
a slab of sentinels (dense as the engine's entries lay it out, the band entries
for more than one bank; or strided), writes every element of the result and
nothing else; the result holds the statement in the class of the path the plan
reports (conftest.assert_kurtosis, skewness_ref.assert_skewness,
moments_ref.assert_moments, unchanged: "regs" the same bits), NaN and +-Inf
where the statement has them; a dense case gives the same bits through
engine.kurtosis / skewness / moments or their band forms.  On "regs" a negated
row's skewness is minus its source's, bit for bit, and its kurtosis the same
bits.  A moments case gives in its skewness and kurtosis planes the bits of
the order-3 and order-4 calls on the same tensors (the latter with
kurt_leaf_tile = 0, as moments plans), and with two planes null the bits of
the other two.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

import kurt_cases as kc
import kurt_planted as kp
from conftest import assert_kurtosis, same_bits
from moments_ref import assert_moments
from skewness_ref import assert_positions, assert_skewness

pytestmark = pytest.mark.gpu

GUARD = 64  # doubles before and after every result
SENTINEL = -7777.25
ENTRY = {4: "kurtosis_blocks", 3: "skewness", 0: "moments"}


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()  # loud failure if libbldp_hip.so is missing
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == kc.NUM_CUS, "the plans of tests/kurt_cases.py were recorded for %d CUs, this " \
        "device reports %d: narrow and chunked plans differ, so would every plan assertion" % (
            kc.NUM_CUS, cus)
    return pkg.engine


def layout(case):
    """(nc, ni, nb, out_bank, ld_i, ld_b, span) of the case's result: element
    (c, i, b) of bank k at k out_bank + c + i ld_i + b ld_b."""
    w = kc.window(case)
    nc, ni, nt = w[1], w[4], w[7]
    nb = nt // case.tblock if case.tblock else 1
    if case.dense:
        return nc, ni, nb, nc * ni * nb, nc, nc * ni, case.nbank * nb * ni * nc
    ld_i = nc + 3
    ld_b = ni * ld_i + 5
    return nc, ni, nb, 0, ld_i, ld_b, (nb - 1) * ld_b + (ni - 1) * ld_i + nc


def call(pkg, eng, case, xs, order, names):
    """The ABI call of `order` on the case's tensors into guarded slabs: per
    bank {plane: (nc, ni, nb) array} of the planes in `names`."""
    import torch

    L = pkg._lib.lib()
    nc, ni, nb, out_bank, ld_i, ld_b, span = layout(case)
    M, nbank = case.tblock, case.nbank
    planes = kp.planes_of(order)
    slabs = {n: torch.full((2 * GUARD + span,), SENTINEL, dtype=torch.float64, device="cuda:0")
             for n in planes}
    outs = [slabs[n].data_ptr() + 8 * GUARD if n in names else None for n in planes]
    ptr, nchan, nif, ntime = eng._abi_dims(xs[0])
    ptrs = (ctypes.c_void_p * nbank)(*[x.data_ptr() for x in xs])
    band = ctypes.cast(ptrs, ctypes.c_void_p)
    keep, wp = pkg._lib.win_arg(case.window)
    s = pkg._lib.stream_ptr()
    if order == 4 and M == 0:
        assert case.dense or nbank == 1
        if nbank == 1:
            fn, rc = "bldp_kurtosis_f32", L.bldp_kurtosis_f32(ptr, nchan, nif, ntime, wp, outs[0],
                                                              None, s)
        else:
            fn, rc = "bldp_band_kurtosis_f32", L.bldp_band_kurtosis_f32(nbank, band, nchan, nif,
                                                                       ntime, wp, outs[0], s)
    elif nbank > 1:
        fn = "bldp_band_%s_f32" % ENTRY[order]
        rc = getattr(L, fn)(nbank, band, nchan, nif, ntime, wp, M, *outs, s)
    else:
        fn = "bldp_%s_f32" % ENTRY[order]
        rc = getattr(L, fn)(ptr, nchan, nif, ntime, wp, M, *outs, ld_i, ld_b, s)
    pkg._lib.check(rc, fn)
    torch.cuda.synchronize()
    # where the result's elements lie in a slab
    c, i, b, k = np.meshgrid(np.arange(nc), np.arange(ni), np.arange(nb), np.arange(nbank),
                             indexing="ij")
    at = GUARD + k * out_bank + c + i * ld_i + b * ld_b
    used = np.zeros(2 * GUARD + span, bool)
    used[at.ravel()] = True
    assert used.sum() == at.size
    res = [{} for _ in range(nbank)]
    for n in planes:
        h = slabs[n].cpu().numpy()
        where = (fn, n, kc.case_id(case))
        if n not in names:
            assert (h == SENTINEL).all(), (where, "a plane not asked for was written")
            continue
        assert (h[~used] == SENTINEL).all(), (where, "wrote outside its result")
        assert (h[used] != SENTINEL).all(), (where, "left elements of its result unwritten")
        v = h[at]
        for kb in range(nbank):
            res[kb][n] = v[..., kb]
    return res


def through_engine(eng, case, xs):
    """The dense result through the engine's own entries, shaped as call()'s."""
    win, M = (None if case.window is None else list(case.window)), case.tblock or None
    if case.order == 4:
        r = [eng.kurtosis(xs[0], win, tblock=M)] if case.nbank == 1 else \
            eng.band_kurtosis(xs, win, tblock=M)
        r = [{"kurtosis": t} for t in r]
    elif case.order == 3:
        r = [eng.skewness(xs[0], win, tblock=M)] if case.nbank == 1 else \
            eng.band_skewness(xs, win, tblock=M)
        r = [{"skewness": t} for t in r]
    else:
        r = [eng.moments(xs[0], win, tblock=M)] if case.nbank == 1 else \
            eng.band_moments(xs, win, tblock=M)
        r = [m._asdict() for m in r]
    out = []
    for d in r:
        d = {n: eng.fb_to_numpy(t) for n, t in d.items()}
        out.append({n: v if M else v[:, :, None] for n, v in d.items()})
    return out


def report(pkg, eng, case, x):
    """The four public plan words of one bank on this device."""
    win = None if case.window is None else list(case.window)
    if case.order == 4 and case.tblock == 0:
        p = eng.kurtosis_plan(x, win)
        return (p["path"], p["K"], p["leaf_slots"], p["workspace_bytes"])
    fn = {4: lambda: eng.kurtosis_blocks_plan(x, case.tblock, win),
          3: lambda: eng.skewness_plan(x, win, case.tblock or None),
          0: lambda: eng.moments_plan(x, win, case.tblock or None)}[case.order]
    p = fn()
    return (p["path"], p["fused"], p["blocks"], p["workspace_bytes"])


def compare(case, got, want, msg):
    path = kc.path(case)
    n = case.tblock if case.tblock else kc.window(case)[7]
    if case.order == 4:
        assert_positions(got["kurtosis"], want["kurtosis"], msg)
        assert_kurtosis(got["kurtosis"], want["kurtosis"], path, n, msg)
    elif case.order == 3:
        assert_skewness(got["skewness"], want["skewness"], want["A"], path, n, msg)
    else:
        assert_moments(got, want, path, n, msg)


def negated_rows_flip(case, got, kinds, bank, msg):
    """"regs": the recipe in its own order, so minus a row gives minus its mean
    and skewness and the bits of its variance and kurtosis."""
    for c, i in zip(*np.nonzero(kinds[:, :, bank] == kp.NEGATED)):
        if c < 2 or kinds[c - 2, i, bank] != kp.POWER:
            continue
        for n, v in got.items():
            sign = -1.0 if n in ("mean", "skewness") else 1.0
            assert same_bits(v[c, i], sign * v[c - 2, i]), (msg, "negated row", n, c, i)


@pytest.mark.parametrize("case", kc.CASES, ids=kc.case_id)
def test_case(pkg, eng, orc, case):
    banks, kinds, spikes = kp.build(case)
    want = kp.statements(orc, case, banks)
    xs = [eng.fb_from_numpy(a, device="cuda:0") for a in banks]
    names = kp.planes_of(case.order)
    with contextlib.ExitStack() as stack:
        for name, val in case.options:
            stack.enter_context(pkg._lib.plan_option(name, val))
        assert report(pkg, eng, case, xs[0]) == (kc.PATHS[case.plan[0]],) + tuple(case.plan[1:]), \
            kc.case_id(case)
        got = call(pkg, eng, case, xs, case.order, names)
        for k in range(case.nbank):
            msg = (kc.case_id(case), "bank %d" % k)
            w = {n: v if case.tblock else v[:, :, None] for n, v in want[k].items()}
            compare(case, got[k], w, msg)
            if kc.path(case) == "regs":
                negated_rows_flip(case, got[k], kinds, k, msg)
        if case.dense:
            eng_got = through_engine(eng, case, xs)
            for k in range(case.nbank):
                for n in names:
                    assert same_bits(eng_got[k][n], got[k][n]), (kc.case_id(case), "engine", n, k)
        if case.order == 0:
            # the separate calls on the same tensors (dense where the ABI has no strided form)
            three = call(pkg, eng, case, xs, 3, ("skewness",))
            four_case = case if case.tblock else case._replace(dense=1)
            with pkg._lib.plan_option("kurt_leaf_tile", 0):
                four = call(pkg, eng, four_case, xs, 4, ("kurtosis",))
            two = call(pkg, eng, case, xs, 0, ("var", "kurtosis"))
            for k in range(case.nbank):
                msg = (kc.case_id(case), "bank %d" % k)
                assert same_bits(got[k]["skewness"], three[k]["skewness"]), (msg, "order 3")
                assert same_bits(got[k]["kurtosis"], four[k]["kurtosis"]), (msg, "order 4")
                assert sorted(two[k]) == ["kurtosis", "var"]
                for n in two[k]:
                    assert same_bits(two[k][n], got[k][n]), (msg, "two planes", n)
