#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): getmoments (csrc/kurtosis.hip, the
"all" instantiations) beside the two calls it fuses, getkurtosis and
getskewness on the same tensor in the same session.

Per shape: kurtosis, skewness, moments (all four planes), moments (skewness +
kurtosis only), kurtosis again (events around each call, median of
``--launches`` calls after untimed ones; buffers under 1 GiB rotate over copies
totalling >= 1 GiB, past the Infinity Cache).  "kurt_spread" is the relative
distance of the two kurtosis medians, the margin a ratio has to exceed to mean
anything.  "all_over_sum" is the four-plane call over kurtosis + skewness (the
claim: below 1 - kurt_spread), "two_over_kurt" the {skewness, kurtosis} call
over the mean of the two kurtosis medians (it should sit next to 1).
``--file`` adds the end-to-end figure for one 0002 file (a raw FBH5 file
written to a temporary directory): one getmoments call against getkurtosis
followed by getskewness, wall clock, median of 5 after one untimed round.

    python tools/moments_probe.py [--shapes ...] [--file] [--out profiles/moments/moments_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from kurt_blocks_probe import time_passes  # noqa: E402
from skew_probe import SHAPES  # noqa: E402


def shape_row(pkg, name, launches):
    import torch

    eng = pkg.engine
    nbank, nchan, nif, nt, M, _ = SHAPES[name]
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

    def moments(which):
        def run(s):
            return (eng.band_moments(sets[s], tblock=M, which=which) if band
                    else eng.moments(sets[s][0], tblock=M, which=which))
        return run

    k1 = time_passes(pkg, kurt, copies, launches, 3)
    sk = time_passes(pkg, skew, copies, launches, 3)
    m4 = time_passes(pkg, moments(eng.MOMENTS), copies, launches, 3)
    m2 = time_passes(pkg, moments(("skewness", "kurtosis")), copies, launches, 3)
    k2 = time_passes(pkg, kurt, copies, launches, 3)
    kmean = 0.5 * (k1[0] + k2[0])
    spread = abs(k1[0] - k2[0]) / min(k1[0], k2[0])
    plan = eng.moments_plan(sets[0][0], tblock=M)
    all_over_sum = m4[0] / (kmean + sk[0])
    row = {"shape": name, "banks": nbank, "nchan": nchan, "nif": nif, "ntime": nt, "tblock": M,
           "copies": copies, "path": plan["path"], "fused": plan["fused"],
           "kurt_ms": round(k1[0], 5), "kurt_again_ms": round(k2[0], 5),
           "skew_ms": round(sk[0], 5),
           "moments_all_ms": round(m4[0], 5), "moments_all_ms_min": round(m4[1], 5),
           "moments_all_ms_max": round(m4[2], 5),
           "moments_skew_kurt_ms": round(m2[0], 5), "moments_skew_kurt_ms_min": round(m2[1], 5),
           "moments_skew_kurt_ms_max": round(m2[2], 5),
           "kurt_spread": round(spread, 4),
           "all_over_sum": round(all_over_sum, 4),
           "all_beats_sum_by_more_than_spread": bool(all_over_sum < 1.0 - spread),
           "two_over_kurt": round(m2[0] / kmean, 4),
           "moments_all_GBps": round(nbytes / (m4[0] * 1e-3) / 1e9, 1)}
    print(json.dumps(row), flush=True)
    del sets
    torch.cuda.empty_cache()
    return row


def file_row(pkg, rounds=5):
    """One 0002 file (65536 x 1 x 272 Float32, raw FBH5): getmoments against
    getkurtosis followed by getskewness, wall clock."""
    W = pkg.WorkerFunctions
    nc, nt = 65536, 272
    a = np.asfortranarray(
        np.random.default_rng(2).gamma(4.0, 1e5, (nt, 1, nc)).astype(np.float32).transpose(2, 1, 0))
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "probe.rawspec.0002.h5")
        pkg.fbh5.write(f, dict(foff=-1.0, nfpc=64), a)

        def wall(fn):
            fn()  # untimed: page cache, pinned buffers, plans
            t = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(t))

        two = wall(lambda: (W.getkurtosis(f), W.getskewness(f)))
        one = wall(lambda: W.getmoments(f))
        pair = wall(lambda: W.getmoments(f, which=("skewness", "kurtosis")))
    row = {"file": "one 0002 file, raw FBH5", "nchan": nc, "nif": 1, "ntime": nt,
           "bytes": int(a.nbytes), "rounds": rounds,
           "getkurtosis_then_getskewness_ms": round(two, 3), "getmoments_ms": round(one, 3),
           "getmoments_skew_kurt_ms": round(pair, 3), "ratio": round(one / two, 4)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--file", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("moments_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = [shape_row(pkg, name, a.launches) for name in a.shapes]
    out = {"tool": "tools/moments_probe.py", "device": torch.cuda.get_device_name(0),
           "launches": a.launches, "rows": rows}
    if a.file:
        out["file"] = file_row(pkg)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
