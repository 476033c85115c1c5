#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): fqavfunc "var" / "std" / "median"
(csrc/stats.hip) beside "sum" on the same buffers, and beside what a kernel
that only reads reaches for the same bytes (tools/hbm_probe.py).

Every launch is timed by events carried on its own dispatch
(bldp_reduce_launch_timed); a row is the median of ``--launches`` launches
after 3 untimed ones.  "warm" re-reads one copy of the window (a 0002 file,
71 MB, stays in the 256 MB Infinity Cache between launches); "cold" rotates
over copies totalling >= 1 GiB, as bench.py --cache cold does.  GB/s counts
the window's bytes once plus the output.

--e2e also times what a user calls: getdata on a page-cached SIGPROC file with
the string op (native read, GPU kernel, result on the host) against the same
call with the NumPy callable, which runs on the host as every fqavfunc
outside sum/mean/max/min did before these kernels.

    python tools/stat_probe.py [--shapes file band bank0000] [--e2e] [--out profiles/x.json]
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
sys.path.insert(0, os.path.join(REPO, "tools"))

# name: (banks, nchan, nif, ntime, fqavby)
SHAPES = {
    "file": (1, 65536, 1, 272, 64),        # one 0002 file
    "band": (8, 65536, 1, 272, 64),        # the 8-bank 0002 band
    "bank0000": (1, 1 << 26, 1, 16, 1024),  # one bank of the 0000 band
}
OPS = ("sum", "var", "std", "median")


def time_op(pkg, sets, F, op, launches):
    """Median ms of `launches` timed launches going round the prepared copies."""
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
    return statistics.median(ms), min(ms), max(ms)


def kernel_rows(pkg, name, launches):
    import torch

    import hbm_probe

    eng = pkg.engine
    nb, nchan, nif, nt, F = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    obytes = nbytes // F
    rows = []
    for cache in ("warm", "cold"):
        copies = 1 if cache == "warm" else max(2, -(-(1 << 30) // nbytes))
        if cache == "cold" and nbytes >= (1 << 30):
            copies = 1  # (already beyond the cache)
        sets = []
        for c in range(copies):
            banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
            for b, v in enumerate(banks):
                eng.synth(nchan, nif, nt, nfpc=max(F, 4), seed=100 * c + b, kind=0, out=v)
            sets.append(banks)
        torch.cuda.synchronize()
        probe = hbm_probe.read_probe(nbytes, launches=launches, pkg=pkg, copies=copies)
        base = None
        for op in OPS:
            med, lo, hi = time_op(pkg, sets, F, op, launches)
            if op == "sum":
                base = med
            rows.append({
                "shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt, "fqavby": F,
                "op": op, "cache": cache, "copies": copies,
                "path": eng.plan(sets[0][0], F, 1, op)["path"],
                "ms": round(med, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5),
                "GBps": round((nbytes + obytes) / (med * 1e-3) / 1e9, 1),
                "time_over_sum": round(med / base, 3),
                "probe_read_GBps": probe["GBps"],
                "share_of_probe": round((nbytes + obytes) / (med * 1e-3) / 1e9 / probe["GBps"], 3),
            })
            print(json.dumps(rows[-1]), flush=True)
        del sets
        torch.cuda.empty_cache()
    return rows


def e2e_rows(pkg, repeats=3):
    """getdata on one page-cached 0002-shaped SIGPROC file: string op (GPU)
    against the NumPy callable with Julia's rules (host)."""
    rd, W = pkg.readers, pkg.worker
    nb, nchan, nif, nt, F = SHAPES["file"]
    rng = np.random.default_rng(1)
    data = np.asfortranarray(rng.gamma(2.0, 5e8, (nchan, nif, nt)).astype(np.float32))
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="PROBE", tstart=59000.5,
               tsamp=18.253611, fch1=8438.96484375, foff=-187.5 / nchan, nchans=nchan, nifs=nif,
               nbits=32)
    host_f = {"median": np.median,
              "var": lambda R, axis: np.var(R, axis=axis, ddof=1),
              "std": lambda R, axis: np.std(R, axis=axis, ddof=1)}
    rows = []
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "guppi_59000_00001_PROBE_0001.rawspec.0002.fil")
        rd.write_fil(f, hdr, data)
        W.getdata(f, fqavby=F, fqavfunc="sum")  # page cache, code objects, staging buffers
        for op in ("median", "var", "std"):
            t = {}
            for route, fn in (("gpu", op), ("host", host_f[op])):
                ts = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    r = W.getdata(f, fqavby=F, fqavfunc=fn)
                    ts.append((time.perf_counter() - t0) * 1e3)
                t[route] = statistics.median(ts)
                t[route + "_shape"] = list(r.shape)
            rows.append({"shape": "file", "e2e": "getdata, page-cached SIGPROC file", "op": op,
                         "fqavby": F, "gpu_ms": round(t["gpu"], 2), "host_ms": round(t["host"], 2),
                         "speedup": round(t["host"] / t["gpu"], 1)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["file", "band"], choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("stat_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = []
    for name in a.shapes:
        rows += kernel_rows(pkg, name, a.launches)
    if a.e2e:
        rows += e2e_rows(pkg)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/stat_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
