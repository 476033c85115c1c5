"""Every reachable Float32 reduce instantiation on planted signed data.

For each case of tests/reduce_cases.py (a small input, with its plan options,
that tools/reduce_launch_record.cpp says starts one instantiation of a
k_reduce_* kernel; tests/test_reduce_reach_host.py holds the table to the
dispatcher): the plan the library reports on this device is the recorded one,
and sum, mean, max and min of the all-negative, mixed, all-positive and special
sets of tests/reduce_signed_ref.py equal the plain reference bit for bit.  The
output lies inside a slab of sentinels, a single bank's rows 4 floats apart
from each other as well: nothing but the result's slots may change.
"""
from __future__ import annotations

import contextlib

import pytest

import reduce_cases as rc
import reduce_signed_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64  # floats before and after the output (256 bytes: the alignment the plan was recorded for)
PAD = 4  # floats between a single bank's output rows (keeps every pitch's residue mod 4)
SENTINEL = -7777.25


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()  # loud failure if libbldp_hip.so is missing
    return pkg.engine


def output(torch, nbank, nco, ni, nto):
    """(slab, out): a Julia-order (nbank nco, ni, nto) view inside a slab of sentinels."""
    pitch = nco + PAD if nbank == 1 else nbank * nco
    slab = torch.full((2 * GUARD + pitch * ni * nto,), SENTINEL, dtype=torch.float32, device="cuda:0")
    rows = slab[GUARD:GUARD + pitch * ni * nto].view(nto, ni, pitch)
    return slab, rows[:, :, :nbank * nco].permute(2, 1, 0)


def untouched(slab, nbank, nco, ni, nto):
    """Everything of the slab but the result's slots still holds the sentinel."""
    s = slab.cpu().numpy()
    pitch = nco + PAD if nbank == 1 else nbank * nco
    body = s[GUARD:GUARD + pitch * ni * nto].reshape(nto, ni, pitch)
    return (s[:GUARD] == SENTINEL).all() and (s[-GUARD:] == SENTINEL).all() and \
        (body[:, :, nbank * nco:] == SENTINEL).all()


def run_case(pkg, eng, case):
    import torch

    shape, window, F, T, nb = (case.nchan, case.nif, case.ntime), case.window, case.F, case.T, \
        case.nbank
    win = None if window is None else list(window)
    nc, ni, nt = ref.window_shape(shape, window)
    nco, nto = nc // F, nt // T
    u = ref.planted(shape, window, F, T, nb, seed=rc.seed_of(case))
    sets = ref.offsets(u, F, T)
    sets["special"] = ref.special(u, shape, window, F, T)
    with contextlib.ExitStack() as stack:
        for name, val in case.options:
            stack.enter_context(pkg._lib.plan_option(name, val))
        for name in ref.SETS:
            xs = [eng.fb_from_numpy(a, device="cuda:0") for a in sets[name]]
            if name == ref.SETS[0]:  # the plan first: what one bank reduced alone would run
                for op in ref.OPS:
                    p = eng.plan(xs[0], F, T, op, win)
                    got = (p["path"], p["lanes_per_group"], p["time_split_waves"],
                           p["float4_per_lane"], p["time_chunks"], p["workgroups"], p["vec_out"])
                    assert got == (pkg._lib.PATHS[case.query[0]],) + tuple(case.query[1:]), \
                        (rc.case_id(case), op, p)
            want = ref.references(u if name == "special" else sets[name], window, F, T,
                                  fix=sets[name] if name == "special" else None)
            for op in ref.OPS:
                slab, out = output(torch, nb, nco, ni, nto)
                if nb == 1:
                    eng.reduce(xs[0], F, T, op, win, out=out)
                else:
                    eng.band_reduce(xs, F, T, op, win, out=out)
                torch.cuda.synchronize()
                got = eng.fb_to_numpy(out)
                bad = ref.mismatch(got, want[op], op, F * T)
                where = "k_reduce_%s op=%s set=%s case=%s" % (case.sym, op, name, rc.case_id(case))
                assert bad is None, where + ": " + bad
                assert untouched(slab, nb, nco, ni, nto), where + ": wrote outside its slots"


@pytest.mark.parametrize("group", rc.GROUPS)
def test_signed_planted(pkg, eng, group):
    cases = [c for c in rc.CASES if rc.group(c) == group]
    assert 1 <= len(cases) <= 64
    for case in cases:
        run_case(pkg, eng, case)
