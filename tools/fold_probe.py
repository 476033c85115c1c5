#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): the fold (csrc/fold.hip, "sum", T = nt)
without a mask, with a dense random 5 % mask and with a bad-channel list, and the
unfold, beside four things on the same buffers in the same process:

  (a) the plain "sum" reduce over fqavby x nt blocks of the same tensor, timed
      twice (before and after the rest: the spread of the two runs says what a
      ratio is worth);
  (b) ``masked_reduce`` of those blocks with the dense mask, and "argmax";
  (c) the torch route, ``x.view(nto, T, ni, J, nfpc).sum((1, 3))`` (Float32 sums);
  (d) the copy-back route: the window to the host and NumPy's Float64 sum there
      (once, wall clock).

Every launch sits between two device events recorded on its stream; a row is the
median of ``--launches`` launches after 3 untimed ones.  Launches rotate over
copies of the buffers (masks included) totalling >= 1 GiB ("cold"), so the 256 MB
Infinity Cache serves none of the reads.

--parent --lib PATH times (a) and (b) alone with another build of the library (the
parent commit's) on the same shapes; --parent-json FILE then sets those rows beside
this build's.

    python tools/fold_probe.py [--shapes file band bank0000 bank0001] [--out FILE]
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

from argext_probe import SHAPES, argext_launchers, timed  # noqa: E402
from masked_probe import make_masks, masked_launchers  # noqa: E402

# fine channels per coarse channel of each product (64 coarse channels a bank)
NFPC = {"file": 1024, "band": 1024, "bank0000": 1 << 20, "bank0001": 8}


def fold_launchers(pkg, sets, masks, nfpc):
    """One closure per copy: the band (or single-bank) fold sum into buffers made once."""
    import torch

    eng, L = pkg.engine, pkg._lib.lib()
    out = []
    for banks, m in zip(sets, masks):
        nb = len(banks)
        nc, ni, nt = banks[0].shape
        data = eng.fb_empty(nfpc, ni, 1, device="cuda:0")
        kept = eng.fb_empty(nfpc, ni, 1, device="cuda:0", dtype=torch.int32)
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        mptr, ld = eng._fold_mask(m, (nb * nc, ni, nt), banks[0].device, "fold_probe")
        args = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, nfpc, nt, 0, mptr, ld,
                data.data_ptr(), kept.data_ptr())

        def go(args=args, keep=(ptrs, data, kept, m, ld)):
            pkg._lib.check(L.bldp_band_fold_f32(*args, pkg._lib.stream_ptr()), "bldp_band_fold_f32")

        out.append(go)
    return out


def unfold_launchers(pkg, sets, nfpc):
    """One closure per copy: the band unfold by the band's own mean profile into one
    output made once (shared by the copies: it is written, never read)."""
    eng, L = pkg.engine, pkg._lib.lib()
    nb = len(sets[0])
    nc, ni, nt = sets[0][0].shape
    dst = eng.fb_empty(nb * nc, ni, nt, device="cuda:0")
    out = []
    for banks in sets:
        prof = eng.band_fold(banks, nfpc, None, "mean")["data"]
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        args = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, nfpc, nt, 0, prof.data_ptr(),
                nfpc, nfpc * ni, dst.data_ptr())

        def go(args=args, keep=(ptrs, prof, dst)):
            pkg._lib.check(L.bldp_band_unfold_f32(*args, pkg._lib.stream_ptr()),
                           "bldp_band_unfold_f32")

        out.append(go)
    return out


def torch_launchers(sets, nfpc):
    import torch

    out = []
    for banks in sets:
        nc, ni, nt = banks[0].shape

        def go(banks=banks, nc=nc, ni=ni, nt=nt):
            parts = [x.permute(2, 1, 0).view(1, nt, ni, nc // nfpc, nfpc).sum((1, 3)) for x in banks]
            return parts[0] if len(parts) == 1 else torch.stack(parts).sum(0)

        out.append(go)
    return out


def copy_back_ms(pkg, banks, nfpc):
    """The window to the host and NumPy's Float64 fold there: wall clock, once."""
    import numpy as np
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = 0.0
    for x in banks:
        h = x.permute(2, 1, 0).contiguous().cpu().numpy()  # (nt, ni, nc)
        nt, ni, nc = h.shape
        s = s + h.reshape(nt, ni, nc // nfpc, nfpc).sum(axis=(0, 2), dtype=np.float64)
    return (time.perf_counter() - t0) * 1e3


def plain_sum(pkg, sets, F, T, launches):
    eng = pkg.engine
    nb = len(sets[0])
    preps = [eng.PreparedBandReduce(banks, F, T, "sum") if nb > 1
             else eng.PreparedReduce(banks[0], F, T, "sum") for banks in sets]
    r = timed([p.launch for p in preps], launches, pkg)
    for p in preps:
        p.close()
    return r


def rows_of(pkg, name, launches, parent):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, F, _ = SHAPES[name]
    nfpc = NFPC[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets, masks = [], []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=nfpc, seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
        masks.append(make_masks(nb, nchan, nif, nt, c))
    torch.cuda.synchronize()
    T = nt
    sum1 = plain_sum(pkg, sets, F, T, launches)
    arg = timed(argext_launchers(pkg, sets, F, T, False), launches, pkg)
    msk = timed(masked_launchers(pkg, sets, [m["dense"] for m in masks], F, T), launches, pkg)
    row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt, "nfpc": nfpc,
           "fqavby": F, "tavby": T, "cache": "cold", "copies": copies, "bytes_in": nbytes,
           "argmax_ms": round(arg[0], 5), "masked_reduce_ms": round(msk[0], 5)}
    if not parent:
        fold = {k: timed(fold_launchers(pkg, sets, [m.get(k) if k else None for m in masks], nfpc),
                         launches, pkg) for k in ("", "dense", "channels")}
        unf = timed(unfold_launchers(pkg, sets, nfpc), launches, pkg)
        torch.cuda.empty_cache()
        tor = timed(torch_launchers(sets, nfpc), max(launches // 3, 5), pkg)
        back = copy_back_ms(pkg, sets[0], nfpc)
        x = sets[0][0]
        plans = {k or "none": eng.fold_plan(x, nfpc, None, mask=(masks[0][k][:x.shape[0]] if k else None))
                 for k in ("", "dense", "channels")}
    sum2 = plain_sum(pkg, sets, F, T, launches)
    base = min(sum1[0], sum2[0])
    row.update({"sum_ms_run1": round(sum1[0], 5), "sum_ms_run2": round(sum2[0], 5),
                "sum_spread": round(abs(sum1[0] - sum2[0]) / base, 3),
                "masked_reduce_over_sum": round(msk[0] / base, 3),
                "argmax_over_sum": round(arg[0] / base, 3),
                "sum_TBps": round(nbytes / (base * 1e-3) / 1e12, 3)})
    if not parent:
        tb = lambda ms, moved: round(moved / (ms * 1e-3) / 1e12, 3)  # noqa: E731
        row.update({
            "plan": plans["none"], "plan_dense": {k: plans["dense"][k] for k in ("mask_loads",)},
            "plan_channels": {k: plans["channels"][k] for k in ("mask_loads",)},
            "fold_ms": round(fold[""][0], 5), "fold_ms_min": round(fold[""][1], 5),
            "fold_ms_max": round(fold[""][2], 5),
            "fold_dense_ms": round(fold["dense"][0], 5),
            "fold_channels_ms": round(fold["channels"][0], 5),
            "unfold_ms": round(unf[0], 5), "torch_route_ms": round(tor[0], 5),
            "copy_back_numpy_ms": round(back, 2),
            "fold_over_sum": round(fold[""][0] / base, 3),
            "fold_dense_over_sum": round(fold["dense"][0] / base, 3),
            "fold_channels_over_sum": round(fold["channels"][0] / base, 3),
            "fold_dense_over_masked_reduce": round(fold["dense"][0] / msk[0], 3),
            "unfold_over_sum": round(unf[0] / base, 3),
            "torch_route_over_fold": round(tor[0] / fold[""][0], 2),
            "copy_back_over_fold": round(back / fold[""][0], 1),
            "fold_TBps_in": tb(fold[""][0], nbytes),
            "fold_dense_TBps_in": tb(fold["dense"][0], nbytes),
            "unfold_TBps_in": tb(unf[0], nbytes), "unfold_TBps_moved": tb(unf[0], 2 * nbytes)})
    print(json.dumps(row), flush=True)
    del sets, masks
    torch.cuda.empty_cache()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--parent", action="store_true",
                    help="a build without the fold: sum, masked_reduce and argmax only")
    ap.add_argument("--lib", default=None, help="another build of libbldp_hip.so to time")
    ap.add_argument("--parent-json", default=None, help="the JSON of a --parent --lib run")
    ap.add_argument("--out", default=os.path.join("profiles", "fold", "fold_probe.json"))
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("fold_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.lib:  # (before the first call loads it)
        pkg._lib.LIB_PATH = os.path.abspath(a.lib)
    if a.parent:  # (a build from before the fold lacks its symbols)
        for name in [n for n in pkg._lib.SIGNATURES if "fold" in n]:
            del pkg._lib.SIGNATURES[name]
    rows = []
    for name in a.shapes:
        rows += rows_of(pkg, name, a.launches, a.parent)
    if a.parent_json:
        with open(a.parent_json) as fh:
            old = {r["shape"]: r for r in json.load(fh)["rows"]}
        for r in rows:
            p = old.get(r["shape"])
            if p:
                r["parent"] = {k: p[k] for k in ("sum_ms_run1", "sum_ms_run2", "sum_spread",
                                                 "masked_reduce_ms", "argmax_ms")}
                for k, mine in (("sum", min(r["sum_ms_run1"], r["sum_ms_run2"])),
                                ("masked_reduce", r["masked_reduce_ms"]), ("argmax", r["argmax_ms"])):
                    theirs = (min(p["sum_ms_run1"], p["sum_ms_run2"]) if k == "sum"
                              else p[k + "_ms"])
                    r["parent"][k + "_this_over_parent"] = round(mine / theirs, 3)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/fold_probe.py", "device": torch.cuda.get_device_name(0),
                       "library": "the tree's" if not a.lib else os.path.basename(a.lib),
                       "launches": a.launches, "timing": "events recorded around each launch",
                       "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
