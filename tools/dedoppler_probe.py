#!/usr/bin/env python3
"""MEASUREMENT TOOL (not product code): the dedoppler (csrc/dedoppler.hip) on the
shapes of the products, beside three things on the same buffers in the same process:

  (a) the plain "sum" reduce with the same tavby, timed twice (before and after the
      rest: the spread of the two runs says what a ratio is worth).  It reads the
      window once: the HBM floor;
  (b) the model's two bounds: the window read once from HBM at 6.29 TB/s (with the
      outputs written), and K * T LDS reads of 4 bytes per output at 128 bytes per
      clock and CU (ds_read_b32), 256 CUs at 2.4 GHz;
  (c) the route a caller had before: K * T shifted torch adds into a (nc, ni, nb)
      accumulator, timed for a few drifts and scaled to K (labelled as scaled).

--check times "sum", "argmax" and "histogram" alone (with --lib PATH: on another
build of the library, the parent commit's), for runs of both builds alternating in
one session; --check-json FILES... sets those rows beside each other.

Every launch sits between two device events recorded on its stream; a row is the
median of ``--launches`` launches after 3 untimed ones.  Launches rotate over
copies of the buffers totalling >= 1 GiB ("cold"), so the 256 MB Infinity Cache
serves none of the reads.

    python tools/dedoppler_probe.py [--shapes ...] [--out profiles/dedoppler/dedoppler_probe.json]
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

from argext_probe import timed  # noqa: E402

HBM_BPS = 6.29e12                    # measured float4 copy
LDS_BPS = 256 * 128 * 2.4e9          # ds_read_b32: 128 B / clk / CU

# name -> (banks, nchan, nif, ntime, tavby, maxdrift, seg, sums)
SHAPES = {
    "bank0000_d8": (1, 1 << 26, 1, 16, 16, 8, 1 << 20, False),      # one 0000 bank
    "bank0000_d64": (1, 1 << 26, 1, 16, 16, 64, 1 << 20, False),
    "bank0000_d512": (1, 1 << 26, 1, 16, 16, 512, 1 << 20, False),
    "band0000_d64": (8, 1 << 26, 1, 16, 16, 64, 1 << 20, False),    # the 8-bank 0000 band
    "file0002_d16": (1, 65536, 1, 272, 16, 16, 1024, False),        # one 0002 file
    "zoom4096_sums": (1, 4096, 1, 4096, 16, 64, 0, True),           # a zoom window, with the sums
}


def make_sets(eng, nb, nchan, nif, nt):
    import torch

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


def plain_sum(pkg, sets, T, launches):
    eng = pkg.engine
    nb = len(sets[0])
    preps = [eng.PreparedBandReduce(banks, 1, T, "sum") if nb > 1
             else eng.PreparedReduce(banks[0], 1, T, "sum") for banks in sets]
    r = timed([p.launch for p in preps], launches, pkg)
    for p in preps:
        p.close()
    return r


def dedop_launchers(pkg, sets, T, D, seg, sums):
    """One closure per copy: the band (or single-bank) dedoppler into buffers made once."""
    import torch

    eng, L = pkg.engine, pkg._lib.lib()
    nb = len(sets[0])
    nc, ni, nt = sets[0][0].shape
    dims = (nb * nc, ni, nt // T)
    best = eng.fb_empty(*dims, device="cuda:0")
    drift = eng.fb_empty(*dims, device="cuda:0", dtype=torch.int32)
    S = eng.planes_empty(*dims, 2 * D + 1, device="cuda:0") if sums else None
    out = []
    for banks in sets:
        ptrs = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in banks])
        geo = eng._abi_dims(banks[0])[1:]
        args = (nb, ctypes.cast(ptrs, ctypes.c_void_p), *geo, None, T, D, seg, best.data_ptr(),
                drift.data_ptr(), S.data_ptr() if sums else None)

        def go(args=args, keep=(ptrs, best, drift, S)):
            pkg._lib.check(L.bldp_band_dedoppler_f32(*args, pkg._lib.stream_ptr()),
                           "bldp_band_dedoppler_f32")

        out.append(go)
    return out


def torch_route_ms(pkg, banks, T, D, seg, launches, ndrifts=3):
    """K * T shifted adds in torch (no segment bounds: the cheaper form), timed for
    ``ndrifts`` drifts of bank 0 and scaled to every drift of every bank."""
    x = banks[0]
    nc, ni, nt = x.shape
    nblk = nt // T
    tab = pkg.engine.drift_offsets(D, T)
    ks = sorted({0, D, 2 * D})[:ndrifts]
    acc = pkg.engine.fb_empty(nc, ni, nblk, device="cuda:0")

    def go():
        for k in ks:
            acc.zero_()
            for t in range(T):
                o = int(tab[k, t])
                lo, hi = max(0, -o), min(nc, nc - o)
                src = x[lo + o:hi + o, :, t::T]
                acc[lo:hi] += src

    ms = timed([go], max(launches // 3, 3), pkg)[0]
    K = 2 * D + 1
    return ms * K / len(ks) * len(banks), len(ks), K


def rows_of(pkg, name, launches):
    import torch

    eng = pkg.engine
    nb, nchan, nif, nt, T, D, seg, sums = SHAPES[name]
    sets, nbytes, copies = make_sets(eng, nb, nchan, nif, nt)
    K = 2 * D + 1
    sum1 = plain_sum(pkg, sets, T, launches)
    d = timed(dedop_launchers(pkg, sets, T, D, seg, sums), launches, pkg)
    old_ms, old_done, _ = torch_route_ms(pkg, sets[0], T, D, seg, launches)
    sum2 = plain_sum(pkg, sets, T, launches)
    base = min(sum1[0], sum2[0])
    p = eng.dedoppler_plan(sets[0][0], D, T, seg)
    nout = nb * nchan * nif * (nt // T)
    out_bytes = nout * 8 + (nout * K * 4 if sums else 0)
    hbm_ms = (nbytes + out_bytes) / HBM_BPS * 1e3
    lds_ms = 4.0 * nb * nchan * nif * nt * K / LDS_BPS * 1e3
    bound = max(hbm_ms, lds_ms)
    row = {"shape": name, "banks": nb, "nchan": nchan, "nif": nif, "ntime": nt, "tavby": T,
           "maxdrift": D, "drifts": K, "seg": seg, "sums": sums, "cache": "cold", "copies": copies,
           "path": p["path"], "tile_channels": p["tile_channels"], "halo": p["halo"],
           "rows_per_chunk": p["rows_per_chunk"], "groups": p["groups"],
           "lds_bytes": p["lds_bytes"], "workgroups_per_bank": p["workgroups"],
           "vector_loads": p["vector_loads"],
           "ms": round(d[0], 5), "ms_min": round(d[1], 5), "ms_max": round(d[2], 5),
           "sum_ms_run1": round(sum1[0], 5), "sum_ms_run2": round(sum2[0], 5),
           "sum_spread": round(abs(sum1[0] - sum2[0]) / base, 3),
           "time_over_sum": round(d[0] / base, 2),
           "model_hbm_ms": round(hbm_ms, 4), "model_lds_ms": round(lds_ms, 4),
           "model_bound": "lds" if lds_ms > hbm_ms else "hbm",
           "time_over_bound": round(d[0] / bound, 2),
           "lds_read_TBps": round(4.0 * nb * nchan * nif * nt * K / (d[0] * 1e-3) / 1e12, 2),
           "read_GBps": round(nbytes / (d[0] * 1e-3) / 1e9, 1),
           "old_route": "K*T shifted torch adds, scaled from %d of %d drifts of one bank" % (old_done, K),
           "old_route_ms": round(old_ms, 3), "old_route_over_dedoppler": round(old_ms / d[0], 1)}
    print(json.dumps(row), flush=True)
    del sets
    torch.cuda.empty_cache()
    return [row]


def check_rows(pkg, launches):
    """sum, argmax and histogram on one 0000 bank and one 0002 file: what a relinked
    library must leave where it was."""
    import torch

    from argext_probe import argext_launchers
    from histogram_probe import hist_launchers, lo_hi

    eng = pkg.engine
    rows = []
    for name, (nb, nchan, nif, nt, F, T) in {"bank0000": (1, 1 << 26, 1, 16, 1024, 16),
                                            "file0002": (1, 65536, 1, 272, 64, 16)}.items():
        sets, nbytes, copies = make_sets(eng, nb, nchan, nif, nt)
        lo, hi = lo_hi(sets[0][0])
        s1 = plain_sum(pkg, sets, T, launches)
        am = timed(argext_launchers(pkg, sets, F, T, False), launches, pkg)
        hg = timed(hist_launchers(pkg, sets, F, T, 64, lo, hi), launches, pkg)
        s2 = plain_sum(pkg, sets, T, launches)
        row = {"shape": name, "sum_ms_run1": round(s1[0], 5), "sum_ms_run2": round(s2[0], 5),
               "sum_spread": round(abs(s1[0] - s2[0]) / min(s1[0], s2[0]), 3),
               "argmax_ms": round(am[0], 5), "histogram_ms": round(hg[0], 5)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del sets
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--check", action="store_true", help="sum, argmax and histogram alone")
    ap.add_argument("--lib", default=None, help="another build of libbldp_hip.so to time")
    ap.add_argument("--check-json", nargs="*", default=None,
                    help="the JSONs of --check runs (this build's and the parent's, in the order "
                         "they ran) to set beside the rows")
    ap.add_argument("--out", default=os.path.join("profiles", "dedoppler", "dedoppler_probe.json"))
    a = ap.parse_args()
    import torch

    import __graft_entry__ as entry

    if not torch.cuda.is_available():
        raise SystemExit("dedoppler_probe needs the GPU: nothing is measured without one")
    pkg = entry.load_package()
    if a.lib:  # (before the first call loads it; a build from before lacks the new symbols)
        pkg._lib.LIB_PATH = os.path.abspath(a.lib)
        for name in [n for n in pkg._lib.SIGNATURES if "dedoppler" in n]:
            del pkg._lib.SIGNATURES[name]
    doc = {"tool": "tools/dedoppler_probe.py", "device": torch.cuda.get_device_name(0),
           "library": "the tree's" if not a.lib else os.path.basename(a.lib),
           "launches": a.launches, "timing": "events recorded around each launch"}
    if a.check:
        doc["rows"] = check_rows(pkg, a.launches)
    else:
        rows = []
        for name in a.shapes:
            rows += rows_of(pkg, name, a.launches)
        doc["rows"] = rows
        doc["model"] = {"hbm_bytes_per_s": HBM_BPS, "lds_bytes_per_s": LDS_BPS,
                        "lds_reads_per_output": "K * T of 4 bytes (ds_read_b32)"}
        if a.check_json:
            doc["parent_check"] = []
            for f in a.check_json:
                with open(f) as fh:
                    j = json.load(fh)
                doc["parent_check"].append({"library": j["library"], "rows": j["rows"]})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
