"""Which instantiations of stats.hip and tstats.hip the case table of
tests/stat_cases.py runs.

tools/stat_launch_record.cpp (the host halves of the two files on stand-ins for
the HIP runtime: no GPU, hipcc only to compile) answers three questions here:
`--list`, the registered entry points C; `--reach`, the set S its sweep of
block lengths, windows, channels, IFs, banks and ops starts; `--cases`, what
each row of the table starts: G.  Asserted: every row plans what the table
recorded and starts the entry point it names; the recorder's restatement of
api.hip (windows, `words`, quantile_set, the plan words) answers what the
library's own plan entry points answer for every row; G holds all of S but
TOO_BIG, each entry of which names the smallest swept input that reaches it,
above MAX_ELEMS; C \\ S is the committed list of profiles/stat_reach/reach.json,
so an instantiation becoming reachable or unreachable is noticed; no kernel
lies wholly in C \\ S or in TOO_BIG; and the entry points the earlier GPU
modules' sweeps leave out are in G.
"""
from __future__ import annotations

import ctypes
import json
import os
import re
import subprocess

import pytest

from conftest import REPO
from test_reduce_dispatch_host import CSRC, _tool

import stat_cases as sc
from quantile_ref import rank_weight

REACH_JSON = os.path.join(REPO, "profiles", "stat_reach", "reach.json")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    hipcc = _tool(["hipcc", "/opt/rocm/bin/hipcc"])
    if not hipcc:
        pytest.skip("hipcc is not installed")
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm",
                        "bin")
    cxx = _tool([os.path.join(llvm, "clang++"), "clang++", "c++"])
    readelf = _tool([os.path.join(llvm, "llvm-readelf"), "readelf"])
    out = str(tmp_path_factory.mktemp("stat_reach"))
    host = [hipcc, "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(REPO, "include"),
            "-I" + CSRC, "-DBLDP_BUILD"]
    objs = [os.path.join(out, n) for n in ("stats.o", "tstats.o", "record.o")]
    jobs = [subprocess.Popen(host + ["-c", os.path.join(CSRC, "stats.hip"), "-o", objs[0]]),
            subprocess.Popen(host + ["-c", os.path.join(CSRC, "tstats.hip"), "-o", objs[1]]),
            subprocess.Popen(host + ["-x", "hip", "-c",
                                     os.path.join(REPO, "tools", "stat_launch_record.cpp"),
                                     "-o", objs[2]])]
    assert [j.wait() for j in jobs] == [0, 0, 0]
    syms = subprocess.run([readelf, "--syms"] + objs, check=True, capture_output=True,
                          text=True).stdout
    defs = ["-Wl,--defsym=%s=0" % s for s in sorted(set(re.findall(r"__hip_fatbin_\w+", syms)))]
    exe = os.path.join(out, "stat_launch_record")
    subprocess.run([cxx] + objs + defs + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def listed(tool):
    """C: every registered entry point of stats.hip and tstats.hip."""
    r = subprocess.run([tool, "--list"], check=True, capture_output=True, text=True)
    return set(r.stdout.split())


@pytest.fixture(scope="module")
def swept(tool):
    """S: {entry point: (elements, the case) of the smallest swept input that starts it}"""
    r = subprocess.run([tool, "--reach"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"total cases=\d+ errors=0", lines[-1]), lines[-1]
    out = {}
    for l in lines[:-1]:
        m = re.fullmatch(r"reach sym=(\S+) elems=(\d+) case=(.*)", l)
        assert m, l
        out[m.group(1)] = (int(m.group(2)), m.group(3))
    return out


@pytest.fixture(scope="module")
def table(tool):
    """[(case, plan, symbols started in order, their (grid, block))] of the table's rows."""
    lines = [sc.case_line(c) for c in sc.CASES]
    r = subprocess.run([tool, "--cases"], input="\n".join(lines) + "\n", capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert out[-1] == "total cases=%d errors=0" % len(lines)
    rows = []
    for k, l in enumerate(out[:-1]):
        parts = l.split(" | ")
        assert parts[0] == "case " + lines[k].strip() and parts[1].startswith("rc=0 "), l
        plan = tuple(int(x) for x in parts[1].split("plan=")[1].split(","))
        launches = [dict(kv.split("=", 1) for kv in p.split()[1:]) for p in parts[2:]]
        rows.append((sc.CASES[k], plan, [d["sym"] for d in launches], launches))
    return rows


def test_every_case_plans_what_the_table_recorded(table):
    for case, plan, syms, launches in table:
        assert plan == case.plan, (sc.case_id(case), plan)
        assert syms[0] == case.first and case.sym in syms, (sc.case_id(case), syms)
        for d in launches:  # a grid within the launch limit, a row per bank, whole waves
            assert 1 <= int(d["gx"]) <= 2 ** 31 - 1 and d["gz"] == "1", d
            assert int(d["gy"]) == case.nbank, d
            assert d["bx"] == "256" and d["by"] == d["bz"] == "1", d


def library_plan(L, case):
    """The ten plan words of one bank from the library's own plan entry points
    (no GPU: they plan for 256 CUs, and take null data)."""
    info = (ctypes.c_int64 * 10)()
    w = None if case.window is None else (ctypes.c_int64 * 9)(*case.window)
    wp = ctypes.cast(w, ctypes.c_void_p) if w else None
    dims = (case.nchan, case.nif, case.ntime)
    op = sc.kind(case)
    codes = {"var": 4, "std": 5, "median": 6, "mad": 8}
    if op in codes and case.axis == 0:
        rc = L.bldp_reduce_plan_f32(None, *dims, wp, case.n, 1, codes[op], None, info)
    elif op in codes:
        rc = L.bldp_tstat_plan_f32(None, *dims, wp, case.n, codes[op], None, info)
    elif op == "quantile":
        rc = L.bldp_quantile_plan_f32(None, *dims, wp, case.axis, case.n,
                                      ctypes.c_double(sc.probs(case)[0]), None, info)
    elif op == "quantiles":
        ps = sc.probs(case)
        rc = L.bldp_quantiles_plan_f32(None, *dims, wp, case.axis, case.n, len(ps),
                                       (ctypes.c_double * len(ps))(*ps), None, info)
    else:
        rc = L.bldp_outliers_plan_f32(None, *dims, wp, case.axis, case.n, int(sc.mask(case)), info)
    assert rc == 0, sc.case_id(case)
    return tuple(info)


def test_the_restatement_answers_what_the_library_plans(pkg):
    L = pkg._lib.lib()
    for case in sc.CASES:
        assert library_plan(L, case) == case.plan, sc.case_id(case)
        paths = sc.PATHS0 if case.axis == 0 else sc.PATHS2
        assert case.plan[0] in paths and paths[case.plan[0]] == \
            (pkg._lib.PATHS if case.axis == 0 else pkg._lib.TSTAT_PATHS)[case.plan[0]]
    # quantile_set: the counts of distinct ranks the quantiles rows recorded
    for case in sc.CASES:
        if sc.kind(case) == "quantiles":
            low = {rank_weight(case.n, p)[0] - 1 for p in sc.probs(case)}
            assert case.plan[8] == len(low | {q + 1 for q in low}), sc.case_id(case)


def test_cases_are_small_and_varied():
    seen = set()
    for c in sc.CASES:
        assert c.nchan * c.nif * c.ntime <= sc.MAX_ELEMS, sc.case_id(c)
        assert c.axis in (0, 2) and c.nbank in (1, 2) and c.note in ("reach", "ranks", "tail")
        assert sc.window(c)[4] * c.nbank >= 2, sc.case_id(c)  # two (bank, IF) rows at least
        assert sc.case_id(c) not in seen
        seen.add(sc.case_id(c))
    # the window forms of the earlier modules, on both axes
    for axis in (0, 2):
        assert {sc.window_form(c) for c in sc.CASES if c.axis == axis} == \
            {"whole", "off3", "step2", "rev", "tstep"}
    assert {sc.kind(c) for c in sc.CASES} == {"var", "std", "median", "mad", "quantile",
                                              "quantiles", "outliers"}
    assert {sc.mask(c) for c in sc.CASES if sc.kind(c) == "outliers"} == {False, True}
    # tails: the last item of a lane partial, on the register and the stream selects
    tails = {(c.axis, c.n) for c in sc.CASES if c.note == "tail"}
    assert tails == {(0, n) for n in (4095, 4096, 4097, 4100, 257, 260, 1025, 1028)} | \
        {(2, n) for n in (257, 1025, 4095, 4097)}
    # sixteen ranks in one launch, on every quantiles kernel
    full = {sc.kernel(c.sym) for c in sc.CASES if sc.kind(c) == "quantiles" and c.plan[8] == 16}
    assert full >= {"k_median_sort", "k_quantiles_select", "k_tstat_regs", "k_tquantiles_split"}


def test_table_reaches_what_the_sweep_reaches(listed, swept, table):
    C, S = listed, set(swept)
    G = {s for row in table for s in row[2]}
    assert S <= C and G <= C
    too_big = set(sc.TOO_BIG)
    assert too_big <= S, sorted(too_big - S)
    assert not too_big & G, sorted(too_big & G)  # (an entry the table reaches is not too big)
    missing = S - G - too_big
    assert not missing, sorted(missing)
    assert len(G) == len(S) - len(too_big)
    named = {c.sym for c in sc.CASES if c.note == "reach"}  # every one by a row of its own
    assert named == S - too_big, sorted((S - too_big) ^ named)
    for s, why in sc.TOO_BIG.items():  # each names the smallest swept input, beyond the limit
        elems = swept[s][0]
        assert elems > sc.MAX_ELEMS and ("%d elements" % elems) in why, (s, elems, why)

    def kernels(syms):
        return {sc.kernel(s) for s in syms}

    assert kernels(C - S) <= kernels(S), sorted(kernels(C - S) - kernels(S))
    assert kernels(too_big) <= kernels(G), sorted(kernels(too_big) - kernels(G))

    with open(REACH_JSON) as f:
        reach = json.load(f)
    unswept = sorted(C - S)
    committed = sorted(s for group in reach["unswept"].values() for s in group["entries"])
    assert unswept == committed, (sorted(set(unswept) - set(committed)),
                                  sorted(set(committed) - set(unswept)))
    for name, group in reach["unswept"].items():
        assert group["entries"] and all(sc.kernel(s) == name for s in group["entries"])
        assert group["excluded_by"]
    assert reach["counts"] == {"C": len(C), "S": len(S), "G": len(G), "TOO_BIG": len(too_big)}
    print("stats/tstats reach: |C| = %d, |S| = %d, |G| = %d, |TOO_BIG| = %d" %
          (len(C), len(S), len(G), len(too_big)))


def test_what_the_earlier_sweeps_leave_out_is_run(table):
    """The entry points no parametrisation of test_gpu_outliers.py and
    test_gpu_quantiles.py names: outliers and quantiles of 16 and 32 sorted keys,
    outliers of 8 spectra in registers, and a last sweep of one lower rank in
    k_tquantiles_split<., 3> (4 or 7 lower ranks)."""
    G = {s for row in table for s in row[2]}
    want = {"k_median_sort<%d,%s,%d>" % (L, v, sel) for L in (16, 32) for v in ("true", "false")
            for sel in (3, 4)}
    want |= {"k_tstat_regs<8,%d,5>" % cpl for cpl in (1, 4)}
    want |= {"k_tquantiles_split<%d,3>" % cpl for cpl in (1, 4)}
    assert want <= G, sorted(want - G)
    for cpl in (1, 4):
        nlow = set()
        for case, plan, syms, _ in table:
            if "k_tquantiles_split<%d,3>" % cpl in syms:
                nlow.add(len({rank_weight(case.n, p)[0] for p in sc.probs(case)}))
        assert nlow >= {4, 7} and nlow & {3, 6}, (cpl, nlow)  # a last sweep of one rank, and full ones
