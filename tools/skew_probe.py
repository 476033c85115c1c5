#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): getskewness (csrc/kurtosis.hip, the
order-3 instantiations) beside its yardstick, getkurtosis on the same tensor in
the same session: it reads the same bytes and does no less arithmetic, so the
skewness should cost what the kurtosis costs.

Per shape: kurtosis, skewness, kurtosis again (events around each call, median
of ``--launches`` calls after untimed ones; buffers under 1 GiB rotate over
copies totalling >= 1 GiB, past the Infinity Cache).  "ratio" is skewness over
the mean of the two kurtosis medians; "kurt_spread" is the relative distance of
the two kurtosis medians, the margin a ratio has to exceed to mean anything.
For the 0002 file also the host route the call replaces: the window copied to
the host plus the recipe in NumPy.

    python tools/skew_probe.py [--shapes ...] [--out profiles/skewness/skew_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from kurt_blocks_probe import time_passes  # noqa: E402

# name: (banks, nchan, nif, ntime, tblock or None, host route too)
SHAPES = {
    "band0002_whole": (8, 65536, 1, 272, None, True),     # the 8-bank 0002 band: mid (k_kurt_mid2)
    "bank0001_whole": (1, 512, 1, 879616, None, False),   # one 0001 bank: leaf
    "bank0001_tblock16": (1, 512, 1, 879616, 16, False),  # k_kurtb_regs
    "bank0001_tblock1024": (1, 512, 1, 879616, 1024, False),  # k_kurtb_stream
    "bank0000_nt16": (1, 1 << 26, 1, 16, None, False),    # one 0000 bank: regs
}


def numpy_statement(a):
    """The recipe on a host (nc, ni, nt <= 1024) Float32 array (one leaf of
    Julia's sum: sequential)."""
    nc, ni, nt = a.shape
    rows = a.reshape((nc * ni, nt), order="F")
    m = (np.add.accumulate(rows, axis=1, dtype=np.float32)[:, -1] / np.float32(nt))[:, None]
    z = rows - m
    z2 = z * z
    cm2 = np.add.accumulate(z2, axis=1, dtype=np.float64)[:, -1] / nt
    cm3 = np.add.accumulate(z2 * z, axis=1, dtype=np.float64)[:, -1] / nt
    return (cm3 / np.sqrt(cm2 * cm2 * cm2)).reshape((nc, ni), order="F")


def shape_row(pkg, name, launches):
    import torch

    eng = pkg.engine
    nbank, nchan, nif, nt, M, host_route = SHAPES[name]
    nbytes = 4 * nbank * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nbank, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=64, seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    torch.cuda.synchronize()
    band = nbank > 1

    def kurt(s):
        return (eng.band_kurtosis(sets[s], tblock=M) if band
                else eng.kurtosis(sets[s][0], tblock=M))

    def skew(s):
        return (eng.band_skewness(sets[s], tblock=M) if band
                else eng.skewness(sets[s][0], tblock=M))

    k1 = time_passes(pkg, kurt, copies, launches, 3)
    sk = time_passes(pkg, skew, copies, launches, 3)
    k2 = time_passes(pkg, kurt, copies, launches, 3)
    kmean = 0.5 * (k1[0] + k2[0])
    plan = eng.skewness_plan(sets[0][0], tblock=M)
    row = {"shape": name, "banks": nbank, "nchan": nchan, "nif": nif, "ntime": nt, "tblock": M,
           "copies": copies, "path": plan["path"], "fused": plan["fused"],
           "kurt_ms": round(k1[0], 5), "kurt_ms_min": round(k1[1], 5), "kurt_ms_max": round(k1[2], 5),
           "kurt_again_ms": round(k2[0], 5), "kurt_again_ms_min": round(k2[1], 5),
           "kurt_again_ms_max": round(k2[2], 5),
           "skew_ms": round(sk[0], 5), "skew_ms_min": round(sk[1], 5), "skew_ms_max": round(sk[2], 5),
           "skew_wall_ms": round(sk[3], 4),
           "ratio": round(sk[0] / kmean, 4),
           "kurt_spread": round(abs(k1[0] - k2[0]) / min(k1[0], k2[0]), 4),
           "skew_GBps": round(nbytes / (sk[0] * 1e-3) / 1e9, 1)}
    if host_route:  # one bank (one file): D2H of the window + the recipe in NumPy
        x = sets[0][0]
        t0 = time.perf_counter()
        a = eng.fb_to_numpy(x)
        t1 = time.perf_counter()
        ref = numpy_statement(a)
        t2 = time.perf_counter()
        got = eng.fb_to_numpy(eng.skewness(x))
        fin = np.isfinite(ref)
        row.update({"host_copy_ms": round((t1 - t0) * 1e3, 2),
                    "host_numpy_ms": round((t2 - t1) * 1e3, 2),
                    "host_route_ms": round((t2 - t0) * 1e3, 2),
                    "gpu_one_bank_ms": round(time_passes(pkg, lambda s: eng.skewness(sets[s][0]),
                                                         copies, launches, 3)[0], 5),
                    "max_abs_diff_vs_numpy": float(np.abs(got[fin] - ref[fin]).max())})
    print(json.dumps(row), flush=True)
    del sets
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("skew_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = [shape_row(pkg, name, a.launches) for name in a.shapes]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/skew_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
