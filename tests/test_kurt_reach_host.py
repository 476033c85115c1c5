"""Which instantiations of kurtosis.hip the case table of tests/kurt_cases.py runs.

tools/kurt_launch_record.cpp (the host half of kurtosis.hip on stand-ins for
the HIP runtime: no GPU, hipcc only to compile) answers three questions here:
`--list`, the registered entry points C; `--reach`, the set S its sweep of
spectrum counts, channels, IFs, banks, tblock, orders and plan options starts;
`--cases`, what each case of the table starts: G.  Asserted: every case plans
what the table recorded and starts the entry point it names; G holds all of S
but TOO_BIG, each entry of which names the smallest swept input that reaches
it, above 2^25 elements per bank; C \\ S is the committed list of
profiles/kurt_reach/reach.json, so an instantiation becoming reachable or
unreachable is noticed; and no kernel lies wholly in C \\ S or in TOO_BIG.
"""
from __future__ import annotations

import json
import os
import re
import subprocess

import pytest

from conftest import REPO
from test_reduce_dispatch_host import CSRC, _tool

import kurt_cases as kc

REACH_JSON = os.path.join(REPO, "profiles", "kurt_reach", "reach.json")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    hipcc = _tool(["hipcc", "/opt/rocm/bin/hipcc"])
    if not hipcc:
        pytest.skip("hipcc is not installed")
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm",
                        "bin")
    cxx = _tool([os.path.join(llvm, "clang++"), "clang++", "c++"])
    readelf = _tool([os.path.join(llvm, "llvm-readelf"), "readelf"])
    out = str(tmp_path_factory.mktemp("kurt_reach"))
    host = [hipcc, "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(REPO, "include"),
            "-I" + CSRC, "-DBLDP_BUILD"]
    objs = [os.path.join(out, n) for n in ("kurtosis.o", "kernels.o", "record.o")]
    jobs = [subprocess.Popen(host + ["-c", os.path.join(CSRC, "kurtosis.hip"), "-o", objs[0]]),
            subprocess.Popen(host + ["-c", os.path.join(CSRC, "kernels.hip"), "-o", objs[1]]),
            subprocess.Popen(host + ["-x", "hip", "-c",
                                     os.path.join(REPO, "tools", "kurt_launch_record.cpp"),
                                     "-o", objs[2]])]
    assert [j.wait() for j in jobs] == [0, 0, 0]
    syms = subprocess.run([readelf, "--syms"] + objs, check=True, capture_output=True,
                          text=True).stdout
    defs = ["-Wl,--defsym=%s=0" % s for s in sorted(set(re.findall(r"__hip_fatbin_\w+", syms)))]
    exe = os.path.join(out, "kurt_launch_record")
    subprocess.run([cxx] + objs + defs + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def listed(tool):
    """C: every registered entry point of kurtosis.hip."""
    r = subprocess.run([tool, "--list"], check=True, capture_output=True, text=True)
    return set(r.stdout.split())


@pytest.fixture(scope="module")
def swept(tool):
    """S: {entry point: (elements per bank, the case) of the smallest swept input that starts it}"""
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
    """[(case, plan, symbols started in order, their (grid, block))] of the table's cases."""
    lines = [kc.case_line(c) for c in kc.CASES]
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
        rows.append((kc.CASES[k], plan, [d["sym"] for d in launches], launches))
    return rows


def test_every_case_plans_what_the_table_recorded(table):
    for case, plan, syms, launches in table:
        assert plan == case.plan, (kc.case_id(case), plan)
        assert syms[0] == case.first and case.sym in syms, (kc.case_id(case), syms)
        for d in launches:  # a 1-D grid within the launch limit, whole waves
            assert 1 <= int(d["gx"]) <= 2 ** 31 - 1 and d["gy"] == d["gz"] == "1", d
            assert int(d["bx"]) in (256, 512, 1024) and d["by"] == d["bz"] == "1", d


def test_cases_are_small_and_varied():
    seen = set()
    for c in kc.CASES:
        assert c.nchan * c.nif * c.ntime <= kc.MAX_ELEMS, kc.case_id(c)
        assert c.order in (4, 3, 0) and c.tblock >= 0
        assert c.dense or (c.nbank == 1 and not (c.order == 4 and c.tblock == 0)), kc.case_id(c)
        assert kc.case_id(c) not in seen
        seen.add(kc.case_id(c))
    # both result layouts, bands, two IFs, every order with and without tblock
    assert {c.dense for c in kc.CASES} == {0, 1}
    assert {(c.order, c.tblock > 0) for c in kc.CASES} == {(o, t) for o in (4, 3, 0)
                                                           for t in (False, True)}
    assert any(c.nbank > 1 for c in kc.CASES) and any(kc.window(c)[4] > 1 for c in kc.CASES)


def test_table_reaches_what_the_sweep_reaches(listed, swept, table):
    C, S = listed, set(swept)
    G = {s for row in table for s in row[2]}
    assert S <= C and G <= C
    too_big = set(kc.TOO_BIG)
    assert too_big <= S, sorted(too_big - S)
    assert not too_big & G, sorted(too_big & G)  # (an entry the table reaches is not too big)
    missing = S - G - too_big
    assert not missing, sorted(missing)
    assert len(G) == len(S) - len(too_big)
    for s, why in kc.TOO_BIG.items():  # each names the smallest swept input, beyond the limit
        elems = swept[s][0]
        assert elems > kc.MAX_ELEMS and ("%d elements" % elems) in why, (s, elems, why)

    def kernels(syms):
        return {kc.kernel(s) for s in syms}

    assert kernels(C - S) <= kernels(S), sorted(kernels(C - S) - kernels(S))
    assert kernels(too_big) <= kernels(G), sorted(kernels(too_big) - kernels(G))

    with open(REACH_JSON) as f:
        reach = json.load(f)
    unswept = sorted(C - S)
    committed = sorted(s for group in reach["unswept"].values() for s in group["entries"])
    assert unswept == committed, (sorted(set(unswept) - set(committed)),
                                  sorted(set(committed) - set(unswept)))
    for name, group in reach["unswept"].items():
        assert group["entries"] and all(kc.kernel(s) == name for s in group["entries"])
        assert group["excluded_by"]
    assert reach["counts"] == {"C": len(C), "S": len(S), "G": len(G), "TOO_BIG": len(too_big)}
    print("kurtosis.hip reach: |C| = %d, |S| = %d, |G| = %d, |TOO_BIG| = %d" %
          (len(C), len(S), len(G), len(too_big)))
