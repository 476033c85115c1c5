"""Which k_reduce_* instantiations the case table of tests/reduce_cases.py runs.

tools/reduce_launch_record.cpp (the host half of kernels.hip on stand-ins for
the HIP runtime: no GPU, hipcc only to compile) answers three questions here:
`--list`, the registered entry points C; `--reach 1 1`, the set S the full
sweep of shapes, alignments and plan options starts; `--cases`, what each case
of the table starts, with all four ops: G.  Asserted: every case plans what
the table recorded; G holds all of S but TOO_BIG, each entry of which names
the smallest swept input that reaches it, above 2^24 elements per bank; C \\ S
is the committed list of profiles/reduce_reach/reach.json, so an instantiation
becoming reachable or unreachable is noticed; and no kernel lies wholly in
C \\ S or in TOO_BIG.
"""
from __future__ import annotations

import json
import os
import re
import subprocess

import pytest

from conftest import REPO
from test_reduce_dispatch_host import CSRC, _tool

import reduce_cases as rc

REACH_JSON = os.path.join(REPO, "profiles", "reduce_reach", "reach.json")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    hipcc = _tool(["hipcc", "/opt/rocm/bin/hipcc"])
    if not hipcc:
        pytest.skip("hipcc is not installed")
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm",
                        "bin")
    cxx = _tool([os.path.join(llvm, "clang++"), "clang++", "c++"])
    readelf = _tool([os.path.join(llvm, "llvm-readelf"), "readelf"])
    out = str(tmp_path_factory.mktemp("reduce_reach"))
    host = [hipcc, "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(REPO, "include"),
            "-I" + CSRC, "-DBLDP_BUILD"]
    objs = [os.path.join(out, "kernels.o"), os.path.join(out, "record.o")]
    jobs = [subprocess.Popen(host + ["-c", os.path.join(CSRC, "kernels.hip"), "-o", objs[0]]),
            subprocess.Popen(host + ["-x", "hip", "-c",
                                     os.path.join(REPO, "tools", "reduce_launch_record.cpp"),
                                     "-o", objs[1]])]
    assert [j.wait() for j in jobs] == [0, 0]
    syms = subprocess.run([readelf, "--syms"] + objs, check=True, capture_output=True,
                          text=True).stdout
    defs = ["-Wl,--defsym=%s=0" % s for s in sorted(set(re.findall(r"__hip_fatbin_\w+", syms)))]
    exe = os.path.join(out, "reduce_launch_record")
    subprocess.run([cxx] + objs + defs + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def listed(tool):
    """C: every registered k_reduce_* entry point."""
    r = subprocess.run([tool, "--list"], check=True, capture_output=True, text=True)
    return set(r.stdout.split())


@pytest.fixture(scope="module")
def swept(tool):
    """S: {entry point: (elements per bank, the input) of the smallest swept input that starts it}"""
    r = subprocess.run([tool, "--reach", "1", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"total cases=\d+ errors=0", lines[-1]), lines[-1]
    out = {}
    for l in lines[:-1]:
        m = re.fullmatch(r"reach sym=(\S+) elems=(\d+) (.*)", l)
        assert m, l
        out[m.group(1)] = (int(m.group(2)), m.group(3))
    return out


@pytest.fixture(scope="module")
def table(tool):
    """[(case, op, plan, query, symbols)] of the table's cases at all four ops."""
    lines = [rc.case_line(c, op) for c in rc.CASES for op in range(4)]
    r = subprocess.run([tool, "--cases"], input="\n".join(lines) + "\n", capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert out[-1] == "total cases=%d errors=0" % len(lines)
    rows = []
    for k, l in enumerate(out[:-1]):
        parts = l.split(" | ")
        assert parts[0] == "case " + lines[k].strip() and parts[1].startswith("rc=0 "), l
        f = dict(kv.split("=", 1) for kv in parts[1].split())
        rows.append((rc.CASES[k // 4], k % 4, tuple(map(int, f["plan"].split(","))),
                     tuple(map(int, f["query"].split(","))),
                     [p.split("sym=")[1] for p in parts[2:]]))
    return rows


def test_every_case_plans_what_the_table_recorded(table):
    for case, op, plan, query, syms in table:
        assert plan == case.plan and query == case.query, (rc.case_id(case), plan, query)
        assert rc.strip_op(syms[0]) == "k_reduce_" + case.sym, (rc.case_id(case), syms)
        assert re.match(r"k_reduce_\w+<%d[,>]" % op, syms[0]), syms
        if case.nbank == 1:  # one bank alone: the launch is the one the library's query describes
            assert plan == query, rc.case_id(case)


def test_cases_are_small_and_hold_enough_blocks():
    seen = set()
    for c in rc.CASES:
        assert c.nchan * c.nif * c.ntime <= 2 ** 24, rc.case_id(c)
        assert c.stitched == (c.nbank > 1)  # (what engine.reduce / band_reduce can ask for)
        assert rc.case_id(c) not in seen
        seen.add(rc.case_id(c))
        if rc.nblocks(c) < min(c.F * c.T, 1024):
            assert rc.few_blocks(c), rc.case_id(c)  # the case says why
    for g in rc.GROUPS:
        assert 1 <= sum(rc.group(c) == g for c in rc.CASES) <= 64, g


def test_table_reaches_what_the_sweep_reaches(listed, swept, table):
    C, S = listed, set(swept)
    G = {s for row in table for s in row[4]}
    assert S <= C and G <= C
    too_big = {rc.with_op(s, op) for s in rc.TOO_BIG for op in range(4)}
    assert too_big <= S, sorted(too_big - S)
    assert not too_big & G, sorted(too_big & G)  # (an entry the table reaches is not too big)
    missing = S - G - too_big
    assert not missing, sorted(missing)
    for s, why in rc.TOO_BIG.items():  # each names the smallest swept input, beyond the limit
        elems = min(swept[f][0] for f in too_big if rc.strip_op(f) == s)
        assert elems > 2 ** 24 and ("%d elements" % elems) in why, (s, elems, why)

    def kernels(syms):
        return {s.split("<")[0] for s in syms}

    assert kernels(C - S) <= kernels(S), sorted(kernels(C - S) - kernels(S))
    assert kernels(too_big) <= kernels(G), sorted(kernels(too_big) - kernels(G))

    with open(REACH_JSON) as f:
        reach = json.load(f)
    unswept = sorted(C - S)
    committed = sorted(s for group in reach["unswept"].values() for s in group["entries"])
    assert unswept == committed, (sorted(set(unswept) - set(committed)),
                                  sorted(set(committed) - set(unswept)))
    for name, group in reach["unswept"].items():
        assert group["entries"] and all(s.startswith(name + "<") for s in group["entries"])
        assert group["excluded_by"]
    assert reach["counts"] == {"C": len(C), "S": len(S), "G": len(G), "TOO_BIG": len(too_big)}
