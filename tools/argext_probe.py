#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): fqavfunc "argmax" (csrc/argext.hip),
with and without the value output, beside the "max" reduce of the same F and T
on the same buffers, and beside what a kernel that only reads reaches for the
same bytes (tools/hbm_probe.py).

Every launch sits between two device events recorded on its stream (timing
events without a system fence); a row is the median of ``--launches`` launches
after 3 untimed ones.  The three ops are timed the same way in one process, so
their ratio is like for like; "max" is also timed by the events its own
dispatch carries (bldp_reduce_launch_timed), which shows what the recorded
events add.  Launches rotate over copies of the buffers totalling >= 1 GiB
("cold", as bench.py --cache cold), so the 256 MB Infinity Cache serves none of
the reads.  GB/s counts the window's bytes once plus the outputs.

    python tools/argext_probe.py [--shapes file band bank0000 bank0001] [--out profiles/argext/argext_probe.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

# name: (banks, nchan, nif, ntime, fqavby, tavby values)
SHAPES = {
    "file": (1, 65536, 1, 272, 64, (1, 16)),          # one 0002 file
    "band": (8, 65536, 1, 272, 64, (1, 16)),          # the 8-bank 0002 band
    "bank0000": (1, 1 << 26, 1, 16, 1024, (16,)),     # one bank of the 0000 band
    "bank0001": (1, 512, 1, 879616, 8, (1024,)),      # one bank of the 0001 band
}


def timed(launchers, launches, pkg):
    """Median / min / max ms of `launches` launches going round the launchers,
    each between two events recorded on the current stream."""
    import torch

    ev = [(pkg._lib.HipEvent(timing=True, fence=False), pkg._lib.HipEvent(timing=True, fence=False))
          for _ in range(launches)]
    for i in range(3):
        launchers[i % len(launchers)]()
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        launchers[(i + 3) % len(launchers)]()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return statistics.median(ms), min(ms), max(ms)


def dispatch_timed(preps, launches, pkg):
    import torch

    ev = [(pkg._lib.HipEvent(timing=True, fence=False), pkg._lib.HipEvent(timing=True, fence=False))
          for _ in range(launches)]
    for i in range(3):
        preps[i % len(preps)].launch()
    for i, (e0, e1) in enumerate(ev):
        preps[(i + 3) % len(preps)].launch_timed(None, e0, e1)
    torch.cuda.synchronize()
    return statistics.median([e0.elapsed_time(e1) for e0, e1 in ev])


def argext_launchers(pkg, sets, F, T, values):
    """One closure per copy: the band (or single-bank) argmax into buffers made once."""
    import torch

    eng, L = pkg.engine, pkg._lib.lib()
    out = []
    for banks in sets:
        nb = len(banks)
        nco, ni, nto = eng.out_shape(tuple(banks[0].shape), None, F, T)
        idx = eng.fb_empty(nb * nco, ni, nto, device="cuda:0", dtype=torch.int32)
        val = eng.fb_empty(nb * nco, ni, nto, device="cuda:0") if values else None
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        args = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, F, T, 0, idx.data_ptr(),
                val.data_ptr() if values else None)

        def go(args=args, keep=(ptrs, idx, val)):
            pkg._lib.check(L.bldp_band_argext_f32(*args, pkg._lib.stream_ptr()),
                           "bldp_band_argext_f32")

        out.append(go)
    return out


def rows_of(pkg, name, launches):
    import torch

    import hbm_probe

    eng = pkg.engine
    nb, nchan, nif, nt, F, Ts = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=max(F, 4), seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    torch.cuda.synchronize()
    probe = hbm_probe.read_probe(nbytes, launches=launches, pkg=pkg, copies=copies)
    rows = []
    for T in Ts:
        nout = nbytes // 4 // (F * T)
        preps = [eng.PreparedBandReduce(banks, F, T, "max") if nb > 1
                 else eng.PreparedReduce(banks[0], F, T, "max") for banks in sets]
        res = {"max": timed([p.launch for p in preps], launches, pkg)}
        max_dispatch = dispatch_timed(preps, launches, pkg)
        for p in preps:
            p.close()
        res["argmax"] = timed(argext_launchers(pkg, sets, F, T, False), launches, pkg)
        res["argmax+val"] = timed(argext_launchers(pkg, sets, F, T, True), launches, pkg)
        base = res["max"][0]
        for op, (med, lo, hi) in res.items():
            obytes = nout * {"max": 4, "argmax": 4, "argmax+val": 8}[op]
            gbps = (nbytes + obytes) / (med * 1e-3) / 1e9
            row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt,
                   "fqavby": F, "tavby": T, "op": op, "cache": "cold", "copies": copies,
                   "path": (eng.plan(sets[0][0], F, T, "max")["path"] if op == "max"
                            else eng.argext_plan(sets[0][0], F, T, "argmax")["path"]),
                   "ms": round(med, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5),
                   "GBps": round(gbps, 1), "time_over_max": round(med / base, 3),
                   "probe_read_GBps": probe["GBps"],
                   "share_of_probe": round(gbps / probe["GBps"], 3)}
            if op == "max":
                row["ms_dispatch_events"] = round(max_dispatch, 5)
            rows.append(row)
            print(json.dumps(row), flush=True)
    del sets
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "argext", "argext_probe.json"))
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("argext_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = []
    for name in a.shapes:
        rows += rows_of(pkg, name, a.launches)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/argext_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "timing": "events recorded around each launch",
                       "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
