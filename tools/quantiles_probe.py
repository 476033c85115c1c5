#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): quantiles((0.25, 0.5, 0.75)) in one call
(csrc/stats.hip, csrc/tstats.hip with the rank set) beside the three
("quantile", p) calls it replaces and beside one ("quantile", 0.5) call, on the
same tensors in the same process.

Per shape, in this order: (c) one quantile(0.5) call, (a) the one quantiles
call, (b) the three quantile calls inside one timed region, (c) again, and
"median" twice around them.  The spread of the two (c) runs is what a ratio has
to be read against: the feature's claim is (a) < (b) by more than that spread.
A row is the median of ``--launches`` calls after 3 untimed ones; every call is
timed with two events on the stream, the launch latency included.

The shapes are tools/quantile_probe.py's (the 8-bank 0002 band at fqavby = 64
and tavby = 16 / 272, one 0000 bank at fqavby = 1024, one 0001 bank at tavby =
1024) plus the stream form, fqavby = 65536 on the 0002 band.  Channel-axis calls
go round copies totalling >= 1 GiB ("cold"); the time-axis tensors are beyond
the 256 MB Infinity Cache.

--parent --lib PATH times another build of the library (the parent commit's,
which has no quantiles) on the same shapes: quantile(0.5) and median only, the
yardstick for "the existing instantiations did not move".

    python tools/quantiles_probe.py [--parent --lib PATH] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from quantile_probe import time_calls  # noqa: E402

PS = (0.25, 0.5, 0.75)
# name: (banks, nchan, nif, ntime, fqavby)
CHAN_SHAPES = {
    "band0002": (8, 65536, 1, 272, 64),           # sorted in registers
    "bank0000": (1, 1 << 26, 1, 16, 1024),        # register select
    "band0002_stream": (8, 65536, 1, 272, 65536),  # stream select
}
# name: (banks, nchan, nif, ntime, tavby values)
TIME_SHAPES = {
    "band0002": (8, 65536, 1, 272, (16, 272)),
    "bank0001": (1, 512, 1, 879616, (1024,)),
}


def runs_of(parent):
    runs = [("first", "median"), ("first", "c")]
    if not parent:
        runs += [("only", "a"), ("only", "b")]
    return runs + [("again", "c"), ("again", "median")]


def finish(rows, runs, common, nbytes):
    t = {}
    for label, what, r in runs:
        t.setdefault(what, []).append(r["ms"])
    c = statistics.mean(t["c"])
    spread = round(abs(t["c"][1] - t["c"][0]) / min(t["c"]), 4)
    for label, what, r in runs:
        row = {**common, "what": {"a": "quantiles(ps), one call", "b": "3 quantile(p) calls",
                                  "c": "quantile(0.5)", "median": "median"}[what],
               "run": label, **r, "read_GBps": round(nbytes / (r["ms"] * 1e-3) / 1e9, 1)}
        if what in ("a", "b"):
            row["over_c"] = round(r["ms"] / c, 3)
            row["c_spread"] = spread
        if what == "a":
            row["a_over_b"] = round(r["ms"] / t["b"][0], 3) if "b" in t else None
        if what == "b":  # (a) ran before (b)
            row["a_less_than_b_beyond_spread"] = bool(t["a"][0] < r["ms"] * (1.0 - spread))
        if what == "median" and label == "again":
            row["c_over_median"] = round(c / statistics.mean(t["median"]), 3)
            row["median_spread"] = round(abs(t["median"][1] - t["median"][0]) / min(t["median"]), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)


def chan_rows(pkg, name, parent, launches):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, F = CHAN_SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=max(min(F, 1024), 4), seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    dims = (nb * nchan // F, nif, nt)
    out = eng.fb_empty(*dims, device="cuda:0")
    torch.cuda.synchronize()

    def one(s, op, o):
        return eng.band_reduce(s, F, 1, op, out=o) if nb > 1 else eng.reduce(s[0], F, 1, op, out=o)

    fns = {"median": [lambda s=s: one(s, "median", out) for s in sets],
           "c": [lambda s=s: one(s, ("quantile", 0.5), out) for s in sets]}
    common = {"axis": "channel", "shape": name, "banks": nb, "nchan": nchan, "nif": nif,
              "ntime": nt, "fqavby": F, "cache": "cold", "copies": copies,
              "path": eng.plan(sets[0][0], F, 1, "median")["path"]}
    if not parent:
        planes = eng.planes_empty(*dims, len(PS), device="cuda:0")
        fns["a"] = [lambda s=s: one(s, ("quantiles", PS), planes) for s in sets]
        fns["b"] = [lambda s=s: [one(s, ("quantile", p), planes[..., k])
                                 for k, p in enumerate(PS)] for s in sets]
        plan = eng.quantiles_plan(sets[0][0], F, PS)
        common.update(ranks=plan["ranks"], reads=plan["reads"])
    rows = []
    runs = [(label, w, time_calls(fns[w], launches)) for label, w in runs_of(parent)]
    finish(rows, runs, common, nbytes)
    del sets, out, fns
    torch.cuda.empty_cache()
    return rows


def time_rows(pkg, name, parent, launches):
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
        dims = (nb * nchan, nif, nt // T)
        out = eng.fb_empty(*dims, device="cuda:0")

        def one(op, o):
            return eng.band_tstat(banks, T, op, out=o) if nb > 1 else \
                eng.tstat(banks[0], T, op, out=o)

        fns = {"median": [lambda: one("median", out)], "c": [lambda: one(("quantile", 0.5), out)]}
        plan = eng.tstat_plan(banks[0], T, "median")
        common = {"axis": "time", "shape": name, "banks": nb, "nchan": nchan, "nif": nif,
                  "ntime": nt, "tavby": T, "path": plan["path"], "median_passes": plan["passes"],
                  "quantile_passes": eng.tstat_plan(banks[0], T, ("quantile", 0.5))["passes"]}
        if not parent:
            planes = eng.planes_empty(*dims, len(PS), device="cuda:0")
            fns["a"] = [lambda: one(("quantiles", PS), planes)]
            fns["b"] = [lambda: [one(("quantile", p), planes[..., k]) for k, p in enumerate(PS)]]
            qp = eng.quantiles_plan(banks[0], T, PS, 2)
            common.update(ranks=qp["ranks"], reads=qp["reads"], channel_lanes=qp["channel_lanes"])
        runs = [(label, w, time_calls(fns[w], launches)) for label, w in runs_of(parent)]
        finish(rows, runs, common, nbytes)
        del out, fns
    del banks
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chan", nargs="*", default=list(CHAN_SHAPES), choices=list(CHAN_SHAPES))
    ap.add_argument("--time", nargs="*", default=list(TIME_SHAPES), choices=list(TIME_SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--parent", action="store_true",
                    help="a build without quantiles: quantile(0.5) and median only")
    ap.add_argument("--lib", default=None, help="another build of libbldp_hip.so to time")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quantiles",
                                                  "quantiles_probe.json"))
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("quantiles_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.lib:  # (before the first call loads it)
        pkg._lib.LIB_PATH = os.path.abspath(a.lib)
    if a.parent:  # (a build from before quantiles lacks its symbols)
        for name in [n for n in pkg._lib.SIGNATURES if "quantiles" in n]:
            del pkg._lib.SIGNATURES[name]
    rows = []
    for name in a.chan:
        rows += chan_rows(pkg, name, a.parent, a.launches)
    for name in a.time:
        rows += time_rows(pkg, name, a.parent, a.launches)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/quantiles_probe.py", "device": torch.cuda.get_device_name(0),
                   "library": "the tree's" if not a.lib else os.path.basename(a.lib),
                   "ps": list(PS), "launches": a.launches, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
