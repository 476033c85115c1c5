#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): the histogram (csrc/hist.hip) on the
shapes of the three bands, beside three things on the same buffers in the same
process:

  (a) the plain "sum" reduce of the same fqavby and tavby, timed twice (before and
      after the rest: the spread of the two runs says what a ratio is worth);
  (b) the route a caller had before: ``torch.histc`` of the whole tensor for the
      whole-window cases (one histogram, float counts, no below / above / nan),
      and for the blocked cases a copy of a subset of the blocks to the host and
      ``numpy.histogram`` per block, scaled to all blocks (labelled as scaled);
  (c) for one 0001 bank at fqavby = 1 over all time, the exact "median" of the
      same blocks (tstat), the slow order statistic a histogram stands in for.

The data is ``engine.synth``'s; lo and hi are the median -+ 5 scaled mads of a
sample of it, so that the centre bins are as hot as on real data.

Every launch sits between two device events recorded on its stream; a row is the
median of ``--launches`` launches after 3 untimed ones.  Launches rotate over
copies of the buffers totalling >= 1 GiB ("cold"), so the 256 MB Infinity Cache
serves none of the reads.

    python tools/histogram_probe.py [--shapes file bank0001 bank0000 band] [--out profiles/histogram/histogram_probe.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from argext_probe import timed  # noqa: E402

# name -> (banks, nchan, nif, ntime, [(fqavby, tavby)]); None: the whole axis
SHAPES = {
    "file": (1, 65536, 1, 272, [(1, None), (64, 16), (None, None)]),        # one 0002 file
    "bank0001": (1, 512, 1, 879616, [(1, None), (None, None)]),             # one 0001 bank
    "bank0000": (1, 1 << 26, 1, 16, [(1024, 16), (None, None)]),            # one 0000 bank
    "band": (8, 65536, 1, 272, [(64, 16)]),                                 # the 8-bank 0002 band
}


def hist_launchers(pkg, sets, F, T, B, lo, hi):
    """One closure per copy: the band (or single-bank) histogram into a buffer made once."""
    eng, L = pkg.engine, pkg._lib.lib()
    out = []
    for banks in sets:
        nb = len(banks)
        nco, ni, nto = eng.out_shape(tuple(banks[0].shape), None, F, T)
        counts = eng.hist_empty(nb * nco, ni, nto, B + 3, device="cuda:0")
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        args = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, F, T, B, lo, hi,
                counts.data_ptr())

        def go(args=args, keep=(ptrs, counts)):
            pkg._lib.check(L.bldp_band_histogram_f32(*args, pkg._lib.stream_ptr()),
                           "bldp_band_histogram_f32")

        out.append(go)
    return out


def histc_launchers(sets, B, lo, hi):
    """torch.histc of each copy's whole storage (every bank: one call each)."""
    import torch

    def go(banks):
        return [torch.histc(x.permute(2, 1, 0).reshape(-1), bins=B, min=lo, max=hi) for x in banks]

    return [lambda banks=banks: go(banks) for banks in sets]


def numpy_route_ms(banks, F, T, B, lo, hi, nblocks=256):
    """Copy the first blocks of bank 0 to the host and numpy.histogram each; the
    wall time scaled to every block of every bank."""
    import numpy as np
    import torch

    x = banks[0]
    nc, ni, nt = x.shape
    total = (nc // F) * ni * (nt // T) * len(banks)
    cb = min(nc // F, nblocks)
    tb = max(1, min(nt // T, nblocks // cb))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = x[:cb * F, :, :tb * T].cpu().numpy()
    for c in range(cb):
        for i in range(ni):
            for t in range(tb):
                np.histogram(h[c * F:(c + 1) * F, i, t * T:(t + 1) * T], bins=B, range=(lo, hi))
    dt = (time.perf_counter() - t0) * 1e3
    done = cb * ni * tb
    return dt * total / done, done, total


def lo_hi(x):
    """median -+ 5 scaled mads of a sample of the bank."""
    import torch

    s = x.permute(2, 1, 0).reshape(-1)[: 1 << 22].float()
    med = s.median()
    mad = (s - med).abs().median() * 1.4826
    return float(med - 5 * mad), float(med + 5 * mad)


def rows_of(pkg, name, launches, out_lines):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, cases = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=1024, seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    torch.cuda.synchronize()
    lo, hi = lo_hi(sets[0][0])
    rows = []
    for F0, T0 in cases:
        F, T = F0 or nchan, T0 or nt
        whole = F0 is None and T0 is None

        def plain():
            preps = [eng.PreparedBandReduce(banks, F, T, "sum") if nb > 1
                     else eng.PreparedReduce(banks[0], F, T, "sum") for banks in sets]
            r = timed([p.launch for p in preps], launches, pkg)
            for p in preps:
                p.close()
            return r

        try:
            sum1 = plain()
        except Exception as e:  # (a shape the plain reduce refuses: no ratio for it)
            print(f"sum {name} F={F} T={T}: {e}", flush=True)
            sum1 = None
        res = {}
        for B in (64, 256) + ((4096,) if whole else ()):
            res[B] = timed(hist_launchers(pkg, sets, F, T, B, lo, hi), launches, pkg)
        old = {}
        for B in res:
            if whole:
                old[B] = ("torch.histc", timed(histc_launchers(sets, B, lo, hi),
                                               max(launches // 3, 5), pkg)[0], None)
            else:
                ms, done, total = numpy_route_ms(sets[0], F, T, B, lo, hi)
                old[B] = ("copy-back + numpy.histogram per block, scaled from a subset", ms,
                          f"{done} of {total} blocks")
        median_ms = None
        if name == "bank0001" and F == 1 and T == nt:
            median_ms = timed([lambda x=banks[0]: eng.tstat(x, T, "median") for banks in sets],
                              5, pkg)[0]
        sum2 = plain() if sum1 else None
        base = min(sum1[0], sum2[0]) if sum1 else None
        for B, h in res.items():
            p = eng.histogram_plan(sets[0][0], B, lo, hi, F, T)
            row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt,
                   "fqavby": F, "tavby": T, "nbins": B, "lo": round(lo, 3), "hi": round(hi, 3),
                   "cache": "cold", "copies": copies, "path": p["path"],
                   "workgroups_per_bank": p["workgroups"], "chunks_per_block": p["chunks_per_block"],
                   "blocks_per_workgroup": p["blocks_per_workgroup"], "lds_bytes": p["lds_bytes"],
                   "replicas": p["replicas"], "vector_loads": p["vector_loads"],
                   "ms": round(h[0], 5), "ms_min": round(h[1], 5), "ms_max": round(h[2], 5),
                   "sum_ms_run1": round(sum1[0], 5) if sum1 else None,
                   "sum_ms_run2": round(sum2[0], 5) if sum1 else None,
                   "sum_spread": round(abs(sum1[0] - sum2[0]) / base, 3) if sum1 else None,
                   "time_over_sum": round(h[0] / base, 3) if sum1 else None,
                   "read_GBps": round(nbytes / (h[0] * 1e-3) / 1e9, 1),
                   "old_route": old[B][0], "old_route_ms": round(old[B][1], 4),
                   "old_route_subset": old[B][2],
                   "old_route_over_histogram": round(old[B][1] / h[0], 1)}
            if median_ms is not None:
                row["median_ms"] = round(median_ms, 4)
                row["median_over_histogram"] = round(median_ms / h[0], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if out_lines:
                with open(out_lines, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
        torch.cuda.empty_cache()
    del sets
    torch.cuda.empty_cache()
    return rows


def pmc_run(pkg, name, calls):
    """Counter passes (rocprofv3 --pmc ... -- this tool --pmc): every case's
    histogram at 64 and 256 bins and its plain sum, `calls` launches each over
    the cold copies, nothing else; tools/sq_summary.py reads the CSV."""
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, cases = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=1024, seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    lo, hi = lo_hi(sets[0][0])
    for F0, T0 in cases:
        F, T = F0 or nchan, T0 or nt
        for B in (64, 256):
            go = hist_launchers(pkg, sets, F, T, B, lo, hi)
            for i in range(calls):
                go[i % len(go)]()
        for i in range(calls):
            banks = sets[i % len(sets)]
            eng.band_reduce(banks, F, T, "sum") if nb > 1 else eng.reduce(banks[0], F, T, "sum")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pmc", action="store_true", help="the launches of a counter pass only")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "histogram", "histogram_probe.json"))
    ap.add_argument("--lines", default="", help="also append every row to this file as it is measured")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("histogram_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.pmc:
        for name in a.shapes:
            pmc_run(pkg, name, 6)
        return
    rows = []
    for name in a.shapes:
        rows += rows_of(pkg, name, a.launches, a.lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/histogram_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "timing": "events recorded around each launch",
                       "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
