#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): the masked reduce (csrc/masked.hip, "sum")
with a dense random 5 % mask and with a bad-channel list ({1, 0, 0} strides),
beside three things on the same buffers in the same process:

  (a) the plain "sum" reduce of the same F and T, timed twice (before and after
      the rest: the spread of the two runs says what a ratio is worth);
  (b) "argmax", which makes the same walk;
  (c) the route through torch: ``where(mask, 0, x)`` and ``(mask == 0).float()``
      as full-size temporaries, the plain reduce of each.

and beside what a kernel that only reads reaches for the bytes moved: the window,
the mask and both outputs (tools/hbm_probe.py).

Every launch sits between two device events recorded on its stream; a row is the
median of ``--launches`` launches after 3 untimed ones.  Launches rotate over
copies of the buffers (masks included) totalling >= 1 GiB ("cold"), so the 256 MB
Infinity Cache serves none of the reads.

    python tools/masked_probe.py [--shapes file band bank0000 bank0001] [--out profiles/masked/masked_probe.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from argext_probe import SHAPES, argext_launchers, timed  # noqa: E402


def make_masks(nb, nchan, nif, nt, seed):
    """The dense 5 % mask of the stitched window (channel-fastest strides) and a
    5 % bad-channel list."""
    import torch

    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    nc = nb * nchan
    flat = (torch.rand(nc * nif * nt, device="cuda:0", generator=g) < 0.05).to(torch.uint8)
    dense = flat.view(nt, nif, nc).permute(2, 1, 0)
    chans = (torch.rand(nc, device="cuda:0", generator=g) < 0.05).to(torch.uint8).view(nc, 1, 1)
    return {"dense": dense, "channels": chans}


def masked_launchers(pkg, sets, masks, F, T):
    """One closure per copy: the band (or single-bank) masked sum into buffers made once."""
    import torch

    eng, L = pkg.engine, pkg._lib.lib()
    out = []
    for banks, m in zip(sets, masks):
        nb = len(banks)
        nco, ni, nto = eng.out_shape(tuple(banks[0].shape), None, F, T)
        nc, _, nt = banks[0].shape
        data = eng.fb_empty(nb * nco, ni, nto, device="cuda:0")
        kept = eng.fb_empty(nb * nco, ni, nto, device="cuda:0", dtype=torch.int32)
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        mptr, ld = eng._mask_arg(m, (nb * nc, ni, nt), banks[0].device, "masked_probe")
        args = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, F, T, 0, mptr, ld,
                data.data_ptr(), kept.data_ptr())

        def go(args=args, keep=(ptrs, data, kept, m, ld)):
            pkg._lib.check(L.bldp_band_masked_reduce_f32(*args, pkg._lib.stream_ptr()),
                           "bldp_band_masked_reduce_f32")

        out.append(go)
    return out


def torch_launchers(pkg, sets, masks, F, T):
    """One closure per copy: the route a caller had before the masked reduce."""
    import torch

    eng = pkg.engine
    out = []
    for banks, m in zip(sets, masks):
        nc = banks[0].shape[0]

        def go(banks=banks, m=m, nc=nc):
            # (on the (nt, ni, nc) storage order, so that the temporaries keep the
            # channel-fastest layout the reduce takes)
            ms = [m[b * nc:(b + 1) * nc].permute(2, 1, 0) for b in range(len(banks))]
            ts = [x.permute(2, 1, 0) for x in banks]
            xs = [torch.where(mb != 0, 0.0, x).contiguous().permute(2, 1, 0)
                  for x, mb in zip(ts, ms)]
            ws = [(mb == 0).float().expand(x.shape).contiguous().permute(2, 1, 0)
                  for x, mb in zip(ts, ms)]
            if len(banks) > 1:
                return eng.band_reduce(xs, F, T, "sum"), eng.band_reduce(ws, F, T, "sum")
            return eng.reduce(xs[0], F, T, "sum"), eng.reduce(ws[0], F, T, "sum")

        out.append(go)
    return out


def rows_of(pkg, name, launches):
    import torch

    import hbm_probe

    eng = pkg.engine
    nb, nchan, nif, nt, F, Ts = SHAPES[name]
    nbytes = 4 * nb * nchan * nif * nt
    copies = 1 if nbytes >= (1 << 30) else max(2, -(-(1 << 30) // nbytes))
    sets, masks = [], []
    for c in range(copies):
        banks = eng.band_empty(nb, nchan, nif, nt, device="cuda:0")
        for b, v in enumerate(banks):
            eng.synth(nchan, nif, nt, nfpc=max(F, 4), seed=100 * c + b, kind=0, out=v)
        sets.append(banks)
        masks.append(make_masks(nb, nchan, nif, nt, c))
    torch.cuda.synchronize()
    rows = []
    for T in Ts:
        nout = nbytes // 4 // (F * T)

        def plain():
            preps = [eng.PreparedBandReduce(banks, F, T, "sum") if nb > 1
                     else eng.PreparedReduce(banks[0], F, T, "sum") for banks in sets]
            r = timed([p.launch for p in preps], launches, pkg)
            for p in preps:
                p.close()
            return r

        sum1 = plain()
        arg = timed(argext_launchers(pkg, sets, F, T, False), launches, pkg)
        res = {}
        for kind in ("dense", "channels"):
            ms = [m[kind] for m in masks]
            res[kind] = (timed(masked_launchers(pkg, sets, ms, F, T), launches, pkg),
                         timed(torch_launchers(pkg, sets, ms, F, T), max(launches // 3, 5), pkg))
            torch.cuda.empty_cache()
        sum2 = plain()
        base = min(sum1[0], sum2[0])
        for kind, (msk, tor) in res.items():
            mbytes = masks[0][kind].numel()
            moved = nbytes + mbytes + 8 * nout
            probe = hbm_probe.read_probe(moved, launches=launches, pkg=pkg, copies=copies)
            x = sets[0][0]
            mplan = eng.masked_reduce_plan(x, masks[0][kind][:x.shape[0]], F, T)
            row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt,
                   "fqavby": F, "tavby": T, "mask": kind, "cache": "cold", "copies": copies,
                   "path": mplan["path"], "mask_loads": mplan["mask_loads"],
                   "ms": round(msk[0], 5), "ms_min": round(msk[1], 5), "ms_max": round(msk[2], 5),
                   "sum_ms_run1": round(sum1[0], 5), "sum_ms_run2": round(sum2[0], 5),
                   "sum_spread": round(abs(sum1[0] - sum2[0]) / base, 3),
                   "argmax_ms": round(arg[0], 5), "torch_route_ms": round(tor[0], 5),
                   "time_over_sum": round(msk[0] / base, 3),
                   "argmax_over_sum": round(arg[0] / base, 3),
                   "time_over_argmax": round(msk[0] / arg[0], 3),
                   "torch_route_over_masked": round(tor[0] / msk[0], 2),
                   "bytes_moved": moved, "GBps": round(moved / (msk[0] * 1e-3) / 1e9, 1),
                   "probe_read_GBps": probe["GBps"],
                   "share_of_probe": round(moved / (msk[0] * 1e-3) / 1e9 / probe["GBps"], 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    del sets, masks
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "masked", "masked_probe.json"))
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("masked_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    rows = []
    for name in a.shapes:
        rows += rows_of(pkg, name, a.launches)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/masked_probe.py", "device": torch.cuda.get_device_name(0),
                       "launches": a.launches, "timing": "events recorded around each launch",
                       "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
