#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): fqavfunc / tavfunc "mad" (csrc/stats.hip,
csrc/tstats.hip with MAD set) beside "median" on the same tensors in the same
process.  median is timed twice, before and after mad; the spread of its two
runs is what a ratio has to be read against.

Channel axis (prepared handles, every launch timed by events carried on its own
dispatch, bldp_reduce_launch_timed): one 0002 file and the 8-bank 0002 band at
fqavby = 64, one bank of the 0000 band at fqavby = 1024.  "cold" rotates over
copies totalling >= 1 GiB, as tools/stat_probe.py does.
Time axis (no prepared handle: two events around each call on the stream, the
~10 us launch latency included): the 0002 band at tavby = 16 and 272, one 0001
bank at tavby = 1024; both are beyond the 256 MB Infinity Cache.
A row is the median of ``--launches`` launches after 3 untimed ones.

--ops median --lib PATH times another build of the library (the parent
commit's) on the same shapes: its median rows are the yardstick for "the
median instantiations are unchanged".

--e2e also times what a user calls: getdata on a page-cached SIGPROC file with
fqavfunc="mad" (native read, GPU kernel, result on the host) against the same
call with a NumPy MAD callable, which runs on the host.

    python tools/mad_probe.py [--e2e] [--ops median mad] [--lib PATH] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name: (banks, nchan, nif, ntime, fqavby)
CHAN_SHAPES = {
    "file": (1, 65536, 1, 272, 64),         # one 0002 file
    "band": (8, 65536, 1, 272, 64),         # the 8-bank 0002 band
    "bank0000": (1, 1 << 26, 1, 16, 1024),  # one bank of the 0000 band
}
# name: (banks, nchan, nif, ntime, tavby values)
TIME_SHAPES = {
    "band0002": (8, 65536, 1, 272, (16, 272)),
    "bank0001": (1, 512, 1, 879616, (1024,)),
}


def summary(ms):
    return {"ms": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5)}


def time_prepared(pkg, sets, F, op, launches):
    """`launches` timed launches going round the prepared copies."""
    import torch

    eng = pkg.engine
    preps = [eng.PreparedBandReduce(banks, F, 1, op) if len(banks) > 1
             else eng.PreparedReduce(banks[0], F, 1, op) for banks in sets]
    ev = [(pkg._lib.HipEvent(timing=True, fence=False), pkg._lib.HipEvent(timing=True, fence=False))
          for _ in range(launches)]
    for i in range(3):
        preps[i % len(preps)].launch()
    for i, (e0, e1) in enumerate(ev):
        preps[(i + 3) % len(preps)].launch_timed(None, e0, e1)
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    for p in preps:
        p.close()
    return summary(ms)


def time_call(fn, launches):
    import torch

    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return summary([e0.elapsed_time(e1) for e0, e1 in ev])


def finish(rows, runs, common, nbytes, obytes):
    """The rows of one shape from its runs [(label, op, timing)], with mad / median
    and the spread of the two median runs."""
    med = [t["ms"] for label, op, t in runs if op == "median"]
    base = statistics.mean(med) if med else None
    spread = round(abs(med[1] - med[0]) / min(med), 4) if len(med) == 2 else None
    for label, op, t in runs:
        row = {**common, "op": op, "run": label, **t,
               "GBps": round((nbytes + obytes) / (t["ms"] * 1e-3) / 1e9, 1)}
        if op == "mad" and base:
            row["mad_over_median"] = round(t["ms"] / base, 3)
            row["median_spread"] = spread
        rows.append(row)
        print(json.dumps(row), flush=True)


def order(ops):
    """median, mad, median again."""
    runs = [("first", "median")] if "median" in ops else []
    if "mad" in ops:
        runs.append(("only", "mad"))
        if "median" in ops:
            runs.append(("again", "median"))
    return runs


def chan_rows(pkg, name, ops, launches):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, F = CHAN_SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=max(F, 4), seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    torch.cuda.synchronize()
    rows = []
    runs = [(label, op, time_prepared(pkg, sets, F, op, launches)) for label, op in order(ops)]
    common = {"axis": "channel", "shape": name, "banks": nb, "nchan": nchan, "nif": nif,
              "ntime": nt, "fqavby": F, "cache": "cold", "copies": copies,
              "path": eng.plan(sets[0][0], F, 1, "median")["path"]}
    finish(rows, runs, common, nbytes, nbytes // F)
    del sets
    torch.cuda.empty_cache()
    return rows


def time_rows(pkg, name, ops, launches):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, tavbys = TIME_SHAPES[name]
    banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
    for b, v in enumerate(banks):
        eng.synth(nchan, nif, nt, nfpc=max(min(nchan, 1024), 4), seed=b, kind=0, out=v)
    torch.cuda.synchronize()
    nbytes = 4 * nb * nchan * nif * nt
    rows = []
    for T in tavbys:
        out = eng.fb_empty(nb * nchan, nif, nt // T, device="cuda:0")

        def fn(op):
            return (lambda: eng.band_tstat(banks, T, op, out=out)) if nb > 1 else \
                   (lambda: eng.tstat(banks[0], T, op, out=out))

        runs = [(label, op, time_call(fn(op), launches)) for label, op in order(ops)]
        plan = eng.tstat_plan(banks[0], T, "median")
        common = {"axis": "time", "shape": name, "banks": nb, "nchan": nchan, "nif": nif,
                  "ntime": nt, "tavby": T, "path": plan["path"], "median_passes": plan["passes"]}
        finish(rows, runs, common, nbytes, nbytes // T)
        del out
    del banks
    torch.cuda.empty_cache()
    return rows


def numpy_mad(R, axis):
    """What a user without the kernel passes as fqavfunc: the host route."""
    c = np.median(R, axis=axis, keepdims=True)
    return np.median(np.abs(R - c), axis=axis) * np.float32(1.4826022185056018)


def e2e_rows(pkg, repeats=3):
    rd, W = pkg.readers, pkg.worker
    nb, nchan, nif, nt, F = CHAN_SHAPES["file"]
    rng = np.random.default_rng(1)
    data = np.asfortranarray(rng.gamma(2.0, 5e8, (nchan, nif, nt)).astype(np.float32))
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="PROBE", tstart=59000.5,
               tsamp=18.253611, fch1=8438.96484375, foff=-187.5 / nchan, nchans=nchan, nifs=nif,
               nbits=32)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "guppi_59000_00001_PROBE_0001.rawspec.0002.fil")
        rd.write_fil(f, hdr, data)
        W.getdata(f, fqavby=F, fqavfunc="sum")  # page cache, code objects, staging buffers
        t = {}
        for route, fn in (("gpu", "mad"), ("host", numpy_mad)):
            ts = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                r = W.getdata(f, fqavby=F, fqavfunc=fn)
                ts.append((time.perf_counter() - t0) * 1e3)
            t[route] = statistics.median(ts)
            t[route + "_shape"] = list(r.shape)
        rows.append({"shape": "file", "e2e": "getdata, page-cached SIGPROC file", "op": "mad",
                     "fqavby": F, "gpu_ms": round(t["gpu"], 2), "host_ms": round(t["host"], 2),
                     "speedup": round(t["host"] / t["gpu"], 1)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chan", nargs="*", default=sorted(CHAN_SHAPES), choices=sorted(CHAN_SHAPES))
    ap.add_argument("--time", nargs="*", default=sorted(TIME_SHAPES), choices=sorted(TIME_SHAPES))
    ap.add_argument("--ops", nargs="*", default=["median", "mad"], choices=["median", "mad"])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libbldp_hip.so to time")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("mad_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.lib:
        pkg._lib.LIB_PATH = os.path.abspath(a.lib)  # (before the first call loads it)
    rows = []
    for name in a.chan:
        rows += chan_rows(pkg, name, a.ops, a.launches)
    for name in a.time:
        rows += time_rows(pkg, name, a.ops, a.launches)
    if a.e2e:
        rows += e2e_rows(pkg)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/mad_probe.py", "device": torch.cuda.get_device_name(0),
                       "library": "the tree's" if not a.lib else os.path.basename(a.lib),
                       "launches": a.launches, "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
