"""The Float32 reduce's planner and dispatcher agree, checked on the host.

tools/reduce_launch_record.cpp links the host half of kernels.hip against
stand-ins for the HIP runtime and prints, for a sweep of shapes, alignments and
plan options, the plan and every launch launch_reduce makes of it.  No GPU and
no HIP runtime library: the test needs hipcc only to compile the host half.

What must hold whatever the tuning: no case is an error, the grid is the
plan's tile count (a 1-D grid capped at INT32_MAX, its kernels looping over
the tiles beyond; a 3-D grid exactly, x <= INT32_MAX and y, z <= 65535, so
its product may exceed INT32_MAX: 2^26-channel rows at 100000 time blocks
give k_reduce_narrowt 819200000 x 1 x 8 workgroups), every dimension fits,
the kernel started is the one the plan names (and of the case's op), a
time-chunked plan is followed by exactly one finalize launch, and the sweep
reaches every kernel and every plan option value.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "bldistributeddataproducts.jl_amd", "csrc")
KERNELS = ("vec", "wavet", "il", "row", "rows", "rowt", "narrow", "narrowt", "narrow_mis", "lane",
           "lanet", "lanes", "col3", "tile", "scalar")
# the reduce plan options of tests/test_gpu_parity.py's PLAN_OPTION_VALUES
OPTION_VALUES = {
    "row_split": (1, 2, 4), "ts_fill": (0, 1), "narrow_mis": (0, 1), "t38": (0, 1),
    "wide_split": (0, 1), "narrow_tpb": (0, 1, 2), "lane": (0, 1), "lane3": (0, 1),
    "lanet": (0, 1), "lanet_pack": (0, 1), "vec_il": (0, 1), "vec_row": (0, 1), "row_tpb": (0, 1),
    "rowt_pack": (0, 1), "rowt_small": (0, 64, 100000), "wavet": (0, 1),
    "unaligned_vec": (0, 1, 2), "row_bpack": (0, 1), "lane_bpack": (0, 1), "wave_bpack": (0, 1),
    "col3": (0, 1), "rowt_narrow8": (0, 1), "st_plain": (0, 1, 2),
}
# every 11th shape at the default plan, every 67th under each option value
# (strides prime to the sweep's loop lengths); `1 1` is the full cross product
STRIDES = ("11", "67")
INT32_MAX = 2 ** 31 - 1


def _tool(names):
    for n in names:
        p = n if os.path.isabs(n) else shutil.which(n)
        if p and os.path.exists(p):
            return p
    return None


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    hipcc = _tool(["hipcc", "/opt/rocm/bin/hipcc"])
    if not hipcc:
        pytest.skip("hipcc is not installed")
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm",
                        "bin")
    cxx = _tool([os.path.join(llvm, "clang++"), "clang++", "c++"])
    readelf = _tool([os.path.join(llvm, "llvm-readelf"), "readelf"])
    out = str(tmp_path_factory.mktemp("reduce_launch_record"))
    host = [hipcc, "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(REPO, "include"),
            "-I" + CSRC, "-DBLDP_BUILD"]
    objs = [os.path.join(out, "kernels.o"), os.path.join(out, "record.o")]
    jobs = [subprocess.Popen(host + ["-c", os.path.join(CSRC, "kernels.hip"), "-o", objs[0]]),
            subprocess.Popen(host + ["-x", "hip", "-c",
                                     os.path.join(REPO, "tools", "reduce_launch_record.cpp"),
                                     "-o", objs[1]])]
    assert [j.wait() for j in jobs] == [0, 0]
    # the device code the host half would register: absent here, its symbol defined as 0
    syms = subprocess.run([readelf, "--syms"] + objs, check=True, capture_output=True,
                          text=True).stdout
    defs = ["-Wl,--defsym=%s=0" % s for s in sorted(set(re.findall(r"__hip_fatbin_\w+", syms)))]
    exe = os.path.join(out, "reduce_launch_record")
    subprocess.run([cxx] + objs + defs + ["-o", exe], check=True)
    r = subprocess.run([exe, *STRIDES], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _fields(part):
    return dict(kv.split("=", 1) for kv in part.split()[1:])


def test_planner_and_dispatcher_agree(record):
    assert re.fullmatch(r"total cases=\d+ errors=0", record[-1]), record[-1]
    cases = record[:-1]
    assert len(cases) == int(record[-1].split()[1].split("=")[1]) > 100000
    kernels, options = set(), set()
    for line in cases:
        parts = line.split(" | ")
        c, p = _fields(parts[0]), _fields("plan " + parts[1])
        launches = [_fields(x) for x in parts[2:]]
        assert p["rc"] == "0" and int(p["nlaunch"]) == len(launches) >= 1, line
        first = launches[0]
        gx, gy, gz = int(first["gx"]), int(first["gy"]), int(first["gz"])
        ntiles = int(first["ntiles"])
        assert 1 <= gx <= INT32_MAX and 1 <= gy <= 65535 and 1 <= gz <= 65535, line
        if gy == gz == 1:  # also the grid-stride kernels: tiles beyond the grid are looped over
            assert gx == min(ntiles, INT32_MAX) == int(p["grid"]), line
        else:  # a workgroup per tile: nothing to cap, the product may pass INT32_MAX
            assert gx * gy * gz == ntiles == int(p["grid"]), line
        assert first["sym"].startswith("k_reduce_%s<%s" % (p["kernel"], c["op"])), line
        for l in launches:
            assert 1 <= int(l["bx"]) * int(l["by"]) * int(l["bz"]) <= 1024, line
            assert int(l["shm"]) <= 160 * 1024, line
        if int(first["nchunk"]) > 1:  # partials, then one finalize
            assert len(launches) == 2 and int(p["ws_bytes"]) > 0, line
            assert re.match(r"k_reduce_finalize(_w)?<%s>$" % c["op"], launches[1]["sym"]), line
        else:
            assert len(launches) == 1 and int(p["ws_bytes"]) == 0, line
        kernels.add(p["kernel"])
        options.add(c["opt"])
    assert kernels == set(KERNELS)
    assert options == {"default:-1"} | {"%s:%d" % (k, v) for k, vs in OPTION_VALUES.items()
                                        for v in vs}
