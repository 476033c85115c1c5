#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): getkurtosis(...; tblock = M), the
kurtosis of every block of M spectra in one call (csrc/kurtosis.hip
k_kurtb_regs / k_kurtb_stream), beside

  (b) the route without it: one windowed engine.kurtosis (band_kurtosis) call
      per block over the same tensor, the baseline;
  (c) the whole-window kurtosis of the same tensor, and what a kernel that
      only reads reaches for the same bytes (tools/hbm_probe.py): what one
      pass over those bytes costs.

Every figure is the time between two events recorded on the stream around the
call(s) of one pass (a pass of (b) is nb calls, so its figure includes the gaps
between its launches: that is its cost), median of ``--launches`` passes after
untimed ones; "wall" is the host time of a pass with a synchronize at its end.
Passes of (b) with more than 4096 calls are timed ``--loop-launches`` times.
Buffers under 1 GiB rotate over copies totalling >= 1 GiB (cold), as
tools/stat_probe.py does.  The results of (a) are compared with those of (b).

    python tools/kurt_blocks_probe.py [--shapes bank0001 band0002] [--out profiles/x.json]
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
sys.path.insert(0, os.path.join(REPO, "tools"))

# name: (banks, nchan, nif, ntime, block lengths)
SHAPES = {
    "bank0001": (1, 512, 1, 879616, (16, 64, 256, 1024)),  # one bank of the 0001 product
    "band0002": (8, 65536, 1, 272, (16, 68)),              # the 8-bank 0002 band
}


def time_passes(pkg, fn, nsets, passes, warm):
    """Median / min / max ms (stream events) and median wall ms of `passes`
    calls of fn(set index), going round the copies."""
    import torch

    HipEvent = pkg._lib.HipEvent
    ev = [(HipEvent(timing=True, fence=False), HipEvent(timing=True, fence=False))
          for _ in range(passes)]
    for i in range(warm):
        fn(i % nsets)
    torch.cuda.synchronize()
    wall = []
    for i, (e0, e1) in enumerate(ev):
        t0 = time.perf_counter()
        e0.record()
        fn((i + warm) % nsets)
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return statistics.median(ms), min(ms), max(ms), statistics.median(wall)


def shape_rows(pkg, name, launches, loop_launches):
    import torch

    import hbm_probe

    eng = pkg.engine
    nbank, nchan, nif, nt, blocks = SHAPES[name]
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

    def whole(s):
        return eng.band_kurtosis(sets[s]) if band else eng.kurtosis(sets[s][0])

    probe = hbm_probe.read_probe(nbytes, launches=launches, pkg=pkg, copies=copies)
    wmed, wlo, whi, wwall = time_passes(pkg, whole, copies, launches, 3)
    rows = [{"shape": name, "what": "whole window", "banks": nbank, "nchan": nchan, "nif": nif,
             "ntime": nt, "copies": copies, "path": eng.kurtosis_plan(sets[0][0])["path"],
             "ms": round(wmed, 5), "ms_min": round(wlo, 5), "ms_max": round(whi, 5),
             "wall_ms": round(wwall, 4), "GBps": round(nbytes / (wmed * 1e-3) / 1e9, 1),
             "probe_read_GBps": probe["GBps"], "probe_read_ms": probe["ms"]}]
    print(json.dumps(rows[-1]), flush=True)
    for M in blocks:
        nb = nt // M
        plan = eng.kurtosis_blocks_plan(sets[0][0], M)
        wins = [[0, nchan, 1, 0, nif, 1, b * M, M, 1] for b in range(nb)]

        def blocked(s):
            return (eng.band_kurtosis(sets[s], tblock=M) if band
                    else eng.kurtosis(sets[s][0], tblock=M))

        def loop(s):
            if band:
                return [eng.band_kurtosis(sets[s], w) for w in wins]
            x = sets[s][0]
            return [eng.kurtosis(x, w) for w in wins]

        # the two routes' results on copy 0
        got = blocked(0)
        ref = loop(0)
        worst = 0.0
        for k in range(nbank):
            g = (got[k] if band else got).permute(2, 1, 0).contiguous().cpu().numpy()
            r = torch.stack([(q[k] if band else q).t() for q in ref]).cpu().numpy()
            assert np.array_equal(np.isnan(g), np.isnan(r))
            if plan["path"] == "regs":
                assert np.array_equal(g[~np.isnan(g)], r[~np.isnan(r)]), "regs: not the loop's bits"
            fin = np.isfinite(r)
            assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)])
            if fin.any():
                worst = max(worst, float((np.abs(g[fin] - r[fin]) / np.abs(r[fin] + 3.0)).max()))
        del got, ref
        amed, alo, ahi, awall = time_passes(pkg, blocked, copies, launches, 3)
        lp = launches if nb <= 4096 else loop_launches
        bmed, blo, bhi, bwall = time_passes(pkg, loop, copies, lp, 1)
        obytes = 8 * nbank * nchan * nif * nb
        rows.append({
            "shape": name, "what": "blocks", "tblock": M, "blocks": nb, "banks": nbank,
            "copies": copies, "path": plan["path"], "fused": plan["fused"],
            "loop_path": eng.kurtosis_plan(sets[0][0], wins[0])["path"],
            "ms": round(amed, 5), "ms_min": round(alo, 5), "ms_max": round(ahi, 5),
            "wall_ms": round(awall, 4),
            "GBps": round((nbytes + obytes) / (amed * 1e-3) / 1e9, 1),
            "loop_ms": round(bmed, 4), "loop_ms_min": round(blo, 4), "loop_ms_max": round(bhi, 4),
            "loop_wall_ms": round(bwall, 3), "loop_passes": lp,
            "blocked_over_loop": round(amed / bmed, 5),
            "blocked_over_whole": round(amed / wmed, 3),
            "blocked_over_probe": round(amed / probe["ms"], 3),
            "max_rel_diff_vs_loop": worst,
        })
        print(json.dumps(rows[-1]), flush=True)
    del sets
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--loop-launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("kurt_blocks_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = []
    for name in a.shapes:
        rows += shape_rows(pkg, name, a.launches, a.loop_launches)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/kurt_blocks_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "loop_launches": a.loop_launches, "rows": rows},
                      fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
