#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): the hits list (csrc/hits.hip) on the
shapes of the three bands, beside three things on the same buffers in the same
process:

  (a) the plain "sum" reduce of the family's fqavby and tavby for the shape, timed
      twice (before and after the rest: the spread of the two runs says what a
      ratio is worth);
  (b) ``torch.nonzero`` of the (expanded) mask plus a gather of the samples, the
      device route a caller had before (row-major order, allocating, synchronising);
  (c) the host route: the mask copied back as it is and ``np.flatnonzero`` of it
      (wall time, once).

Masks: empty; random at densities 1e-5, 1e-3 and 5 %; a 1 % bad-channel list
(nc, 1, 1); ``outliers``' own mask at nsigma = 5 over the whole time range.

Every call sits between two device events recorded on its stream; a row is the
median of ``--launches`` calls after 3 untimed ones.  Calls rotate over copies of
the buffers (data and masks) totalling >= 1 GiB of data ("cold").  The count-only
call (cap = 0: two launches) and the full call (three) are timed separately; the
three kernels' own times come from a ``--trace`` pass of this tool under a kernel
trace (``--trace-csv`` folds that trace's CSV into the JSON).

    python tools/hits_probe.py [--shapes file bank0001 bank0000 band] [--out profiles/hits/hits_probe.json]
"""
from __future__ import annotations

import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from argext_probe import timed  # noqa: E402

# name -> (banks, nchan, nif, ntime, (fqavby, tavby) of the yardstick sum)
SHAPES = {
    "file": (1, 65536, 1, 272, (64, 16)),          # one 0002 file
    "bank0001": (1, 512, 1, 879616, (8, 1024)),    # one 0001 bank
    "bank0000": (1, 1 << 26, 1, 16, (1024, 16)),   # one 0000 bank
    "band": (8, 65536, 1, 272, (64, 16)),          # the 8-bank 0002 band
}
MASKS = ("empty", "d1e-5", "d1e-3", "d5e-2", "bad_channels_1pct", "outliers_5sigma")
TRACE_CALLS = 4


def make_mask(pkg, name, banks, seed):
    """A device mask over the vcat window of ``banks``."""
    import torch

    eng = pkg.engine
    nb = len(banks)
    nc, ni, nt = banks[0].shape
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    if name == "bad_channels_1pct":
        m = eng.fb_empty(nb * nc, 1, 1, device="cuda:0", dtype=torch.uint8)
        m.copy_((torch.rand(nb * nc, 1, 1, device="cuda:0", generator=g) < 0.01).to(torch.uint8))
        return m
    if name == "outliers_5sigma":
        o = eng.band_outliers(banks, None, axis=2, nsigma=5.0, mask=True, which=("count",)) \
            if nb > 1 else eng.outliers(banks[0], None, axis=2, nsigma=5.0, mask=True,
                                        which=("count",))
        return o["mask"]
    m = eng.fb_empty(nb * nc, ni, nt, device="cuda:0", dtype=torch.uint8)
    flat = m.permute(2, 1, 0).reshape(-1)   # (the storage, in linear window order)
    assert flat.data_ptr() == m.data_ptr()
    flat.zero_()
    p = {"empty": 0.0, "d1e-5": 1e-5, "d1e-3": 1e-3, "d5e-2": 5e-2}[name]
    if p > 0:
        step = 1 << 26
        for o in range(0, flat.numel(), step):
            n = min(step, flat.numel() - o)
            flat[o:o + n] = (torch.rand(n, device="cuda:0", generator=g) < p).to(torch.uint8)
    return m


def hits_launchers(pkg, sets, masks, caps):
    """(count-only closures, full closures), one per copy, into lists made once."""
    import torch

    eng, L = pkg.engine, pkg._lib.lib()
    count, full = [], []
    for banks, m, cap in zip(sets, masks, caps):
        nb = len(banks)
        nc, ni, nt = banks[0].shape
        mptr, ld = eng._mask_arg(m, (nb * nc, ni, nt), banks[0].device, "hits_probe")
        idx = torch.empty(max(cap, 1), dtype=torch.int64, device="cuda:0")
        val = torch.empty(max(cap, 1), dtype=torch.float32, device="cuda:0")
        total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        head = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, mptr, ld)

        def go(tail, head=head, keep=(ptrs, idx, val, total, m, ld)):
            pkg._lib.check(L.bldp_band_hits_f32(*head, *tail, pkg._lib.stream_ptr()),
                           "bldp_band_hits_f32")

        count.append(lambda go=go, t=total: go((0, None, None, t.data_ptr())))
        full.append(lambda go=go, c=cap, i=idx, v=val, t=total:
                    go((max(c, 1), i.data_ptr(), v.data_ptr(), t.data_ptr())))
    return count, full


def nonzero_launchers(sets, masks):
    """torch.nonzero of the expanded mask and a gather of the flagged samples."""
    import torch

    def go(banks, m):
        out = []
        nc = banks[0].shape[0]
        for b, x in enumerate(banks):
            mb = m[b * nc:(b + 1) * nc] if m.shape[0] > 1 else m
            nz = torch.nonzero(mb.expand(x.shape))
            out.append((nz, x[nz[:, 0], nz[:, 1], nz[:, 2]]))
        return out

    return [lambda banks=banks, m=m: go(banks, m) for banks, m in zip(sets, masks)]


def host_route_ms(m, wshape):
    """The mask copied back as it is, then np.flatnonzero of the broadcast mask."""
    import numpy as np
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = m.permute(2, 1, 0).contiguous().cpu().numpy().transpose(2, 1, 0)
    t1 = time.perf_counter()
    idx = np.flatnonzero(np.broadcast_to(h, wshape).reshape(-1, order="F"))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(idx.size)


def make_sets(pkg, name):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, _ = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets = []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=1024, seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
    torch.cuda.synchronize()
    return sets, nbytes, copies


def totals_of(pkg, sets, masks):
    return [pkg.engine.band_hits(banks, m, maxhits=0)["total"] for banks, m in zip(sets, masks)]


def rows_of(pkg, name, launches, out_lines, which):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, (F, T) = SHAPES[name]
    sets, nbytes, copies = make_sets(pkg, name)
    N = nb * nchan * nif * nt

    def plain():
        preps = [eng.PreparedBandReduce(banks, F, T, "sum") if nb > 1
                 else eng.PreparedReduce(banks[0], F, T, "sum") for banks in sets]
        r = timed([p.launch for p in preps], launches, pkg)
        for p in preps:
            p.close()
        return r

    rows = []
    sum1 = plain()
    res = {}
    for mname in which:
        masks = [make_mask(pkg, mname, banks, 7 + c) for c, banks in enumerate(sets)]
        totals = totals_of(pkg, sets, masks)
        count, full = hits_launchers(pkg, sets, masks, totals)
        t_count = timed(count, launches, pkg)
        t_full = timed(full, launches, pkg)
        t_nz = timed(nonzero_launchers(sets, masks), max(launches // 3, 5), pkg)
        copy_ms, np_ms, nhost = host_route_ms(masks[0], (nb * nchan, nif, nt))
        assert nhost == totals[0], (nhost, totals[0])
        plan = eng.hits_plan(sets[0][0], masks[0][:nchan] if masks[0].shape[0] > 1 else masks[0])
        res[mname] = (t_count, t_full, t_nz, copy_ms, np_ms, totals, plan,
                      int(masks[0].numel()))
        del masks, count, full
        torch.cuda.empty_cache()
    sum2 = plain()
    base = min(sum1[0], sum2[0])
    for mname, (tc, tf, tz, copy_ms, np_ms, totals, plan, mbytes) in res.items():
        hits = statistics.mean(totals)
        moved = mbytes * 2 + 12 * hits + 4 * hits  # mask twice, 12 B a hit out, its sample in
        row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt,
               "mask": mname, "mask_bytes": mbytes, "hits_mean": round(hits, 1),
               "density": round(hits / N, 8), "cache": "cold", "copies": copies,
               "mask_loads": plan["mask_loads"], "flags_per_load": plan["flags_per_load"],
               "tile_elems_one_bank": plan["tile_elems"],
               "count_only_ms": round(tc[0], 5), "count_only_ms_min": round(tc[1], 5),
               "count_only_ms_max": round(tc[2], 5),
               "call_ms": round(tf[0], 5), "call_ms_min": round(tf[1], 5),
               "call_ms_max": round(tf[2], 5),
               "bytes_moved": int(moved), "call_GBps": round(moved / (tf[0] * 1e-3) / 1e9, 1),
               "sum_fqavby": F, "sum_tavby": T, "sum_bytes": nbytes,
               "sum_ms_run1": round(sum1[0], 5), "sum_ms_run2": round(sum2[0], 5),
               "sum_spread": round(abs(sum1[0] - sum2[0]) / base, 3),
               "call_over_sum": round(tf[0] / base, 3),
               "count_only_over_sum": round(tc[0] / base, 3),
               "torch_nonzero_gather_ms": round(tz[0], 4),
               "torch_nonzero_over_call": round(tz[0] / tf[0], 1),
               "host_mask_copy_ms": round(copy_ms, 3), "host_flatnonzero_ms": round(np_ms, 3),
               "host_route_over_call": round((copy_ms + np_ms) / tf[0], 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if out_lines:
            with open(out_lines, "a") as fh:
                fh.write(json.dumps(row) + "\n")
    del sets
    torch.cuda.empty_cache()
    return rows


def trace_run(pkg, name, which):
    """The launches of a kernel-trace pass only: per mask, TRACE_CALLS full calls
    on one copy (3 dispatches each, in order)."""
    import torch

    nb, nchan, nif, nt, _ = SHAPES[name]
    eng = pkg.engine
    banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
    for b, v in enumerate(banks):
        eng.synth(nchan, nif, nt, nfpc=1024, seed=b, kind=0, out=v)
    for mname in which:
        m = make_mask(pkg, mname, banks, 7)
        tot = totals_of(pkg, [banks], [m])
        _, full = hits_launchers(pkg, [banks], [m], tot)
        torch.cuda.synchronize()
        for _ in range(TRACE_CALLS):
            full[0]()
        torch.cuda.synchronize()
        del m, full
        torch.cuda.empty_cache()


def fold_trace(path, shapes, which):
    """Per (shape, mask): the median microseconds of k_hits_count, k_hits_scan and
    k_hits_write over the trace pass's TRACE_CALLS full calls (the dispatches of
    the hits kernels in time order: the count-only call that sizes the lists
    comes first for every mask and is skipped)."""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    recs = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "k_hits_" in r["Kernel_Name"]:
                    recs.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                                 r["Kernel_Name"]))
    recs.sort()
    out, pos = [], 0
    for s in shapes:
        for mname in which:
            pos += 2  # the sizing call: count and scan
            d = {"count": [], "scan": [], "write": []}
            for _ in range(TRACE_CALLS):
                for key in ("count", "scan", "write"):
                    t0, t1, kn = recs[pos]
                    assert "k_hits_" + key in kn, (pos, key, kn)
                    d[key].append((t1 - t0) / 1e3)
                    pos += 1
            out.append({"shape": s, "mask": mname, "calls": TRACE_CALLS,
                        **{"k_hits_%s_us" % k: round(statistics.median(v), 2)
                           for k, v in d.items()}})
    assert pos == len(recs), (pos, len(recs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true", help="the launches of a kernel-trace pass only")
    ap.add_argument("--trace-csv", default="", help="fold this trace pass's output directory into --out")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--masks", nargs="*", default=list(MASKS), choices=MASKS)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "hits", "hits_probe.json"))
    ap.add_argument("--lines", default="", help="also append every row to this file as it is measured")
    a = ap.parse_args()
    if a.trace_csv:
        with open(a.out) as fh:
            doc = json.load(fh)
        doc["kernels"] = fold_trace(a.trace_csv, a.shapes, a.masks)
        doc["kernels_timing"] = "kernel trace of a pass of its own (--trace), warm, one copy"
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        return
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("hits_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.trace:
        for name in a.shapes:
            trace_run(pkg, name, a.masks)
        return
    rows = []
    for name in a.shapes:
        rows += rows_of(pkg, name, a.launches, a.lines, a.masks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/hits_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "timing": "events recorded around each call",
                       "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
