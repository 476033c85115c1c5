#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): outliers (csrc/stats.hip, csrc/tstats.hip
with SEL_OUTLIERS) beside "mad" on the same tensors in the same process, in the
method of tools/mad_probe.py.  Per shape, in this order:

  mad (first)     bldp_band_reduce_f32 / bldp_band_tstat_f32 with BLDP_OP_MAD
  outliers        bldp_band_outliers_f32, the three planes, no mask
  outliers+mask   the same with the mask
  mad (again)     the spread of the two mad runs is what a ratio is read against
  host route      what a user did before: the "median" call, the "mad" call, both
                  products copied back, and the NumPy threshold over the window
                  (already on the host); wall clock, beside the wall clock of
                  outliers+mask with its four results copied back

Every kernel row is the median of ``--launches`` launches after 3 untimed ones,
each between two events on the stream (the ~10 us launch latency included, the
same for every row: all go through the plain ABI calls with outputs allocated
beforehand), going round copies of the input totalling >= 1 GiB.

--ops mad --lib PATH times another build of the library (the parent commit's) on
the same shapes; --parent FILE then sets those rows beside this build's mad.

    python tools/outliers_probe.py [--lib PATH --ops mad] [--parent FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MAD = 8
NSIGMA = 5.0
# name: (banks, nchan, nif, ntime, axis, n)
SHAPES = {
    "band0002_F64": (8, 65536, 1, 272, 0, 64),         # the 8-bank 0002 band
    "bank0000_F1024": (1, 1 << 26, 1, 16, 0, 1024),    # one bank of the 0000 band
    "bank0002_F65536": (1, 65536, 1, 272, 0, 65536),   # one 0002 bank, a block per spectrum
    "band0002_T16": (8, 65536, 1, 272, 2, 16),
    "band0002_T272": (8, 65536, 1, 272, 2, 272),
    "bank0001_T1024": (1, 512, 1, 879616, 2, 1024),    # one 0001 bank
}


def summary(ms):
    return {"ms": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5)}


def time_calls(fns, launches):
    """`launches` timed calls going round fns (one per copy of the input)."""
    import torch

    for i in range(3):
        fns[i % len(fns)]()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(launches)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        fns[(i + 3) % len(fns)]()
        e1.record()
    torch.cuda.synchronize()
    return summary([e0.elapsed_time(e1) for e0, e1 in ev])


def wall(fn, repeats):
    import torch

    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3),
            "ms_max": round(max(ts), 3), "repeats": repeats}


def shape_rows(pkg, name, ops, launches):
    import torch

    eng, L = pkg.engine, pkg._lib.lib()
    nb, nchan, nif, nt, axis, n = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=max(min(n if axis == 0 else nchan, 1024), 4),
                      seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    dims = (nchan // n, nif, nt) if axis == 0 else (nchan, nif, nt // n)
    f32 = [eng.fb_empty(nb * dims[0], dims[1], dims[2], device="cuda:0") for _ in range(2)]
    cnt = eng.fb_empty(nb * dims[0], dims[1], dims[2], device="cuda:0", dtype=torch.int32)
    ptrs = [(ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks]) for banks in sets]
    cast = [ctypes.cast(p, ctypes.c_void_p) for p in ptrs]
    torch.cuda.synchronize()

    def mad_fn(k):
        if axis == 0:
            return lambda: L.bldp_band_reduce_f32(nb, cast[k], nchan, nif, nt, None, n, 1, MAD,
                                                  f32[1].data_ptr(), None)
        return lambda: L.bldp_band_tstat_f32(nb, cast[k], nchan, nif, nt, None, n, MAD,
                                             f32[1].data_ptr(), None)

    def out_fn(k, mask):
        return lambda: L.bldp_band_outliers_f32(nb, cast[k], nchan, nif, nt, None, axis, n, NSIGMA,
                                                f32[0].data_ptr(), f32[1].data_ptr(),
                                                cnt.data_ptr(),
                                                mask.data_ptr() if mask is not None else None, None)

    assert mad_fn(0)() == 0, pkg._lib.last_error()
    rows, runs = [], []
    common = {"shape": name, "axis": axis, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt,
              "n": n, "copies": copies, "input_bytes": nbytes}

    def emit(row):
        rows.append({**common, **row})
        print(json.dumps(rows[-1]), flush=True)

    runs.append(("mad", "first", time_calls([mad_fn(k) for k in range(copies)], launches)))
    if "outliers" in ops:
        plan = eng.outliers_plan(sets[0][0], n, axis=axis)
        common.update(path=plan["path"], reads=plan["reads"],
                      reads_mask=eng.outliers_plan(sets[0][0], n, axis=axis, mask=True)["reads"])
        assert out_fn(0, None)() == 0, pkg._lib.last_error()
        runs.append(("outliers", "planes",
                     time_calls([out_fn(k, None) for k in range(copies)], launches)))
        mask = eng.fb_empty(nb * nchan, nif, nt, device="cuda:0", dtype=torch.uint8)
        runs.append(("outliers", "planes+mask",
                     time_calls([out_fn(k, mask) for k in range(copies)], launches)))
        runs.append(("mad", "again", time_calls([mad_fn(k) for k in range(copies)], launches)))
    mads = [t["ms"] for op, run, t in runs if op == "mad"]
    base = statistics.mean(mads)
    spread = round(abs(mads[-1] - mads[0]) / min(mads), 4) if len(mads) == 2 else None
    for op, run, t in runs:
        row = {"op": op, "run": run, **t}
        if op == "outliers":
            row.update(over_mad=round(t["ms"] / base, 3), mad_spread=spread)
        emit(row)
    if "outliers" in ops and "host" in ops:
        # the two routes to the flags on the host, wall clock; the window is there already
        repeats = 2 if nbytes >= (1 << 30) else 3
        banks = sets[0]
        a = np.concatenate([eng.fb_to_numpy(b) for b in banks], axis=0)
        stat = (lambda op: eng.band_reduce(banks, n, 1, op)) if axis == 0 else \
               (lambda op: eng.band_tstat(banks, n, op))

        def old_route():
            c = eng.fb_to_numpy(stat("median"))
            s = eng.fb_to_numpy(stat("mad"))
            thr = (NSIGMA * s.astype(np.float64)).astype(np.float32)
            c, thr = np.repeat(c, n, axis=axis), np.repeat(thr, n, axis=axis)
            return np.abs(a - c) > thr

        def new_route():
            out_fn(0, mask)()
            return [eng.fb_to_numpy(t) for t in (f32[0], f32[1], cnt, mask)]

        flags = old_route()
        got = new_route()
        agree = bool(np.array_equal(flags.astype(np.uint8), got[3]))
        del flags, got
        t_old, t_new = wall(old_route, repeats), wall(new_route, repeats)
        emit({"op": "host route", "run": "median + mad + copies + NumPy threshold", **t_old})
        emit({"op": "outliers", "run": "planes+mask, results copied back", **t_new,
              "host_route_over_this": round(t_old["ms"] / t_new["ms"], 2),
              "same_flags": agree})
    del sets, f32, cnt
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--ops", nargs="*", default=["mad", "outliers", "host"],
                    choices=["mad", "outliers", "host"])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--lib", default=None, help="another build of libbldp_hip.so to time")
    ap.add_argument("--parent", default=None, help="the JSON of a --lib --ops mad run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("outliers_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.lib:
        pkg._lib.LIB_PATH = os.path.abspath(a.lib)  # (before the first call loads it)
        if "outliers" not in a.ops:  # (a build from before outliers lacks its symbols)
            for name in [n for n in pkg._lib.SIGNATURES if "outliers" in n]:
                del pkg._lib.SIGNATURES[name]
    rows = []
    for name in a.shapes:
        rows += shape_rows(pkg, name, a.ops, a.launches)
    doc = {"tool": "tools/outliers_probe.py", "device": torch.cuda.get_device_name(0),
           "library": "the tree's" if not a.lib else os.path.basename(a.lib),
           "launches": a.launches, "nsigma": NSIGMA, "rows": rows}
    if a.parent:
        with open(a.parent) as fh:
            parent = json.load(fh)
        doc["parent_mad_rows"] = parent["rows"]
        agree = []
        for name in a.shapes:
            mine = [r["ms"] for r in rows if r["shape"] == name and r["op"] == "mad"]
            theirs = [r["ms"] for r in parent["rows"] if r["shape"] == name and r["op"] == "mad"]
            if mine and theirs:
                agree.append({"shape": name, "mad_ms": mine, "parent_mad_ms": theirs,
                              "this_over_parent": round(statistics.mean(mine) /
                                                        statistics.mean(theirs), 4),
                              "mad_spread": round(abs(mine[-1] - mine[0]) / min(mine), 4)})
        doc["mad_against_parent"] = agree
        print(json.dumps(agree), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
