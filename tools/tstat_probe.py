#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): tavfunc "var" / "std" / "median"
(csrc/tstats.hip) beside (a) the existing "sum" reduce with fqavby = 1 and the
same tavby on the same buffers, the pure-read yardstick, and (b) NumPy on the
host with the same rules.

Shapes: the 8-bank 0002 band (8 x 65536 x 272) at T = 16 and T = 272, and one
0001 bank (512 x 879616) at T = 1024 and T = nt.  Both are beyond the 256 MB
Infinity Cache (570 MB and 1.8 GB), so every launch reads HBM.

There is no prepared handle for tstat, so every call (the yardstick's too) is
timed by two events recorded around it on the stream: a row is the median of
``--launches`` calls after 2 untimed ones and includes the call's launch
latency (~10 us).  GB/s counts the window's bytes once plus the output.

The host rows time NumPy on a sub-window that fits a quick run (one 0002 bank;
the first 131072 spectra of the 0001 bank, T = nt meaning that sub-window's
nt) and are compared per byte.

    python tools/tstat_probe.py [--shapes band0002 bank0001] [--no-host] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name: (banks, nchan, nif, ntime, tavby values (0 = ntime), host sub-window spectra)
SHAPES = {
    "band0002": (8, 65536, 1, 272, (16, 0), 272),
    "bank0001": (1, 512, 1, 879616, (1024, 0), 131072),
}
OPS = ("sum", "var", "std", "median")


def time_call(fn, launches):
    import torch

    for _ in range(2):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return statistics.median(ms), min(ms), max(ms)


def host_stat(a, T, op):
    """Julia's rules in NumPy along time on a Fortran-ordered (nc, ni, nt) array."""
    nc, ni, nt = a.shape
    R = a.reshape((nc, ni, T, nt // T), order="F")
    if op == "var":
        return np.var(R, axis=2, ddof=1)
    if op == "std":
        return np.std(R, axis=2, ddof=1)
    return np.median(R, axis=2)


def rows_of(pkg, name, launches, host):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, tavbys, host_nt = SHAPES[name]
    banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
    for b, v in enumerate(banks):
        eng.synth(nchan, nif, nt, nfpc=max(min(nchan, 1024), 4), seed=b, kind=0, out=v)
    torch.cuda.synchronize()
    nbytes = 4 * nb * nchan * nif * nt
    rows = []
    for T in tavbys:
        T = T or nt
        out = eng.fb_empty(nb * nchan, nif, nt // T, device="cuda:0")
        base = None
        for op in OPS:
            if op == "sum":
                fn = (lambda: eng.band_reduce(banks, 1, T, "sum", out=out)) if nb > 1 else \
                     (lambda: eng.reduce(banks[0], 1, T, "sum", out=out))
                plan = eng.plan(banks[0], 1, T, "sum")
                plan = {"path": plan["path"]}
            else:
                fn = (lambda op=op: eng.band_tstat(banks, T, op, out=out)) if nb > 1 else \
                     (lambda op=op: eng.tstat(banks[0], T, op, out=out))
                plan = eng.tstat_plan(banks[0], T, op)
            med, lo, hi = time_call(fn, launches)
            if op == "sum":
                base = med
            obytes = nbytes // T
            row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt,
                   "tavby": T, "op": op, "plan": plan,
                   "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                   "GBps": round((nbytes + obytes) / (med * 1e-3) / 1e9, 1),
                   "time_over_sum": round(med / base, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del out
    if host:
        a = eng.fb_to_numpy(banks[0][:, :, :host_nt])
        hbytes = a.nbytes
        for T in tavbys:
            Th = T or host_nt
            for op in OPS[1:]:
                t0 = time.perf_counter()
                r = host_stat(a, Th, op)
                hms = (time.perf_counter() - t0) * 1e3
                gpu = next(x for x in rows if x["tavby"] == (T or nt) and x["op"] == op)
                gpu_ms_per_gb = gpu["ms"] / (nbytes / 1e9)
                row = {"shape": name, "host": "numpy, one run", "op": op, "tavby": Th,
                       "host_window": [nchan, nif, host_nt], "host_ms": round(hms, 1),
                       "host_ms_per_GB": round(hms / (hbytes / 1e9), 1),
                       "gpu_ms_per_GB": round(gpu_ms_per_gb, 4),
                       "gpu_over_host_per_byte": round(hms / (hbytes / 1e9) / gpu_ms_per_gb, 1),
                       "host_result_shape": list(r.shape)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    del banks
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tstats", "tstat_probe.json"))
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("tstat_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = []
    for name in a.shapes:
        rows += rows_of(pkg, name, a.launches, not a.no_host)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/tstat_probe.py", "device": torch.cuda.get_device_name(0),
                   "launches": a.launches,
                   "timing": "events around each call on the stream (launch latency included)",
                   "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
