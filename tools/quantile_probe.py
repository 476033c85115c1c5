#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): fqavfunc / tavfunc ("quantile", 0.25)
(csrc/stats.hip, csrc/tstats.hip with the quantile selector) beside "median"
and "mad" on the same tensors in the same process.  median is timed twice,
first and last; the spread of its two runs is what a ratio has to be read
against.

No prepared handle exists for a quantile, so every op is timed the same way:
two events around each engine call on the stream, the ~10 us launch latency
included.  Channel axis: the 8-bank 0002 band at fqavby = 64 and one bank of the
0000 band at fqavby = 1024, the calls going round copies totalling >= 1 GiB
("cold").  Time axis: the 0002 band at tavby = 16 and 272, one 0001 bank at
tavby = 1024; all beyond the 256 MB Infinity Cache.  A row is the median of
``--launches`` calls after 3 untimed ones.

--ops median mad --lib PATH times another build of the library (the parent
commit's, which has no quantile) on the same shapes: its rows are the
yardstick for "the median and mad instantiations are unchanged".

    python tools/quantile_probe.py [--ops median quantile mad] [--lib PATH] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

P = 0.25
# name: (banks, nchan, nif, ntime, fqavby)
CHAN_SHAPES = {
    "band0002": (8, 65536, 1, 272, 64),     # the 8-bank 0002 band
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


def time_calls(fns, launches):
    """`launches` timed calls going round `fns` (one per copy of the data)."""
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


def opval(op):
    return ("quantile", P) if op == "quantile" else op


def order(ops):
    """median, quantile, mad, median again."""
    runs = [("first", "median")] if "median" in ops else []
    runs += [("only", op) for op in ("quantile", "mad") if op in ops]
    if "median" in ops and len(runs) > 1:
        runs.append(("again", "median"))
    return runs


def finish(rows, runs, common, nbytes, obytes):
    """The rows of one shape from its runs [(label, op, timing)], with op / median
    and the spread of the two median runs."""
    med = [t["ms"] for label, op, t in runs if op == "median"]
    base = statistics.mean(med) if med else None
    spread = round(abs(med[1] - med[0]) / min(med), 4) if len(med) == 2 else None
    for label, op, t in runs:
        row = {**common, "op": op, "run": label, **t,
               "GBps": round((nbytes + obytes) / (t["ms"] * 1e-3) / 1e9, 1)}
        if op == "quantile":
            row["p"] = P
        if op != "median" and base:
            row["over_median"] = round(t["ms"] / base, 3)
            row["median_spread"] = spread
        rows.append(row)
        print(json.dumps(row), flush=True)


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
    out = eng.fb_empty(nb * nchan // F, nif, nt, device="cuda:0")
    torch.cuda.synchronize()

    def fns(op):
        if nb > 1:
            return [lambda s=s: eng.band_reduce(s, F, 1, opval(op), out=out) for s in sets]
        return [lambda s=s: eng.reduce(s[0], F, 1, opval(op), out=out) for s in sets]

    rows = []
    runs = [(label, op, time_calls(fns(op), launches)) for label, op in order(ops)]
    common = {"axis": "channel", "shape": name, "banks": nb, "nchan": nchan, "nif": nif,
              "ntime": nt, "fqavby": F, "cache": "cold", "copies": copies,
              "path": eng.plan(sets[0][0], F, 1, "median")["path"]}
    finish(rows, runs, common, nbytes, nbytes // F)
    del sets, out
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

        def fns(op):
            return [(lambda: eng.band_tstat(banks, T, opval(op), out=out)) if nb > 1 else
                    (lambda: eng.tstat(banks[0], T, opval(op), out=out))]

        runs = [(label, op, time_calls(fns(op), launches)) for label, op in order(ops)]
        plan = eng.tstat_plan(banks[0], T, "median")
        common = {"axis": "time", "shape": name, "banks": nb, "nchan": nchan, "nif": nif,
                  "ntime": nt, "tavby": T, "path": plan["path"], "median_passes": plan["passes"]}
        if "quantile" in ops:
            common["quantile_passes"] = eng.tstat_plan(banks[0], T, opval("quantile"))["passes"]
        finish(rows, runs, common, nbytes, nbytes // T)
        del out
    del banks
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chan", nargs="*", default=sorted(CHAN_SHAPES), choices=sorted(CHAN_SHAPES))
    ap.add_argument("--time", nargs="*", default=sorted(TIME_SHAPES), choices=sorted(TIME_SHAPES))
    ap.add_argument("--ops", nargs="*", default=["median", "quantile", "mad"],
                    choices=["median", "quantile", "mad"])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--lib", default=None, help="another build of libbldp_hip.so to time")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("quantile_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.lib:  # (before the first call loads it; a build from before quantile lacks its symbols)
        pkg._lib.LIB_PATH = os.path.abspath(a.lib)
        if "quantile" not in a.ops:
            for name in [n for n in pkg._lib.SIGNATURES if n.startswith("bldp_quantile_")
                         or n == "bldp_band_quantile_f32"]:
                del pkg._lib.SIGNATURES[name]
    rows = []
    for name in a.chan:
        rows += chan_rows(pkg, name, a.ops, a.launches)
    for name in a.time:
        rows += time_rows(pkg, name, a.ops, a.launches)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/quantile_probe.py", "device": torch.cuda.get_device_name(0),
                       "library": "the tree's" if not a.lib else os.path.basename(a.lib),
                       "launches": a.launches, "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
