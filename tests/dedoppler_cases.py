"""The case table of tests/test_gpu_dedoppler.py, kept apart so that the CPU suite
can ask bldp_dedoppler_plan_f32 which kernels the GPU cases run
(test_dedoppler_host.py).

A case is a window of nc channels, ni IFs and nt spectra searched over blocks of T
spectra up to maxdrift D inside segments of ``seg`` channels (0: the whole window),
and how the window lies in its array.  ``plan`` is what the library plans for it
with 256-byte aligned tensors: (path, vector loads, tile channels).

Windows: "full" the whole array; "c0" channels from 1 (off the float4 boundary);
"cs2" every second channel; "rev" the channels reversed; "tsub" spectra 2 .. nt + 1
of nt + 5.

The planner's constants the shapes are chosen around: a tile of TILE = 256 channels
while 2 D <= 256 (512, then 1024 beyond), GROUP = 8 drifts a group, a resident block
up to 160 KiB of LDS and chunks of 64 KiB beyond."""
from __future__ import annotations

import ctypes
from collections import namedtuple

TILE, GROUP = 256, 8
LDS_RESIDENT, LDS_CHUNK = 160 * 1024, 64 * 1024

Case = namedtuple("Case", "nc ni nt T D seg win plan")

R, C = "resident", "chunked"
CASES = [
    # nc around the tile: C - 1, C, C + 1, 2C + 3, and an aligned partial tile
    Case(TILE - 1, 1, 16, 16, 3, 0, "full", (R, 0, 256)),
    Case(TILE, 1, 16, 16, 3, 0, "full", (R, 1, 256)),
    Case(TILE + 1, 1, 16, 16, 3, 0, "full", (R, 0, 256)),
    Case(2 * TILE + 3, 2, 16, 16, 3, 0, "full", (R, 0, 256)),
    Case(TILE + 4, 2, 16, 16, 5, 0, "full", (R, 1, 256)),
    # a tile no path leaves (the body without the per-lane bounds), vector and scalar
    Case(800, 1, 32, 16, 8, 0, "full", (R, 1, 256)),
    Case(801, 1, 17, 17, 8, 0, "full", (R, 0, 256)),
    # the halo beyond the window on both sides; one channel
    Case(5, 1, 4, 4, 70, 0, "full", (R, 0, 256)),
    Case(1, 1, 3, 3, 2, 0, "full", (R, 0, 256)),
    # D around the group
    Case(300, 1, 16, 16, 0, 0, "full", (R, 1, 256)),
    Case(300, 1, 16, 16, 1, 0, "full", (R, 1, 256)),
    Case(300, 1, 16, 16, GROUP - 1, 0, "full", (R, 1, 256)),
    Case(300, 1, 16, 16, GROUP, 0, "full", (R, 1, 256)),
    Case(300, 1, 16, 16, GROUP + 1, 0, "full", (R, 1, 256)),
    # large D: the wider tiles
    Case(512, 1, 4, 4, 64, 0, "full", (R, 1, 256)),
    Case(600, 1, 4, 4, 200, 0, "full", (R, 1, 512)),
    Case(512, 1, 4, 4, 1024, 0, "full", (R, 1, 1024)),
    Case(260, 1, 4, 4, 1024, 64, "c0", (R, 0, 1024)),
    # T: 2, 3, 16, 17; blocks and IFs that do not mix
    Case(300, 2, 6, 2, 5, 0, "full", (R, 1, 256)),
    Case(300, 2, 9, 3, 5, 0, "full", (R, 1, 256)),
    Case(300, 2, 48, 16, 5, 0, "full", (R, 1, 256)),
    Case(300, 2, 51, 17, 20, 0, "full", (R, 1, 256)),
    # T against the LDS (a row of 96 + 2 * 8 ... : 272 words, 1088 bytes): one above
    # what 64 KiB hold (resident, above 64 KiB), one above what 160 KiB hold (chunked,
    # the last chunk partial), 272 (chunked)
    Case(96, 1, 61, 61, 8, 0, "full", (R, 1, 256)),
    Case(96, 1, 151, 151, 8, 0, "full", (C, 1, 256)),
    Case(96, 2, 272, 272, 8, 0, "full", (C, 1, 256)),
    Case(97, 1, 544, 272, 9, 16, "full", (C, 0, 256)),
    # segments: 16 with D = 20, one that does not divide the tile, one that does not
    # divide nc
    Case(300, 1, 16, 16, 20, 16, "full", (R, 1, 256)),
    Case(600, 2, 16, 16, 12, 100, "full", (R, 1, 256)),
    Case(300, 1, 16, 16, 9, 7, "full", (R, 1, 256)),
    # the window in its array
    Case(300, 2, 16, 16, 6, 0, "c0", (R, 0, 256)),
    Case(300, 1, 16, 16, 6, 50, "cs2", (R, 0, 256)),
    Case(300, 2, 16, 16, 6, 0, "rev", (R, 0, 256)),
    Case(300, 2, 32, 16, 6, 0, "tsub", (R, 1, 256)),
]


def case_id(c):
    return "nc%d-ni%d-nt%d-T%d-D%d-seg%d-%s" % (c.nc, c.ni, c.nt, c.T, c.D, c.seg, c.win)


def array_shape(c):
    """(nchan, nif, ntime) of the array that holds the case's window."""
    return {"full": (c.nc, c.ni, c.nt), "c0": (c.nc + 4, c.ni, c.nt),
            "cs2": (2 * c.nc, c.ni, c.nt), "rev": (c.nc, c.ni, c.nt),
            "tsub": (c.nc, c.ni, c.nt + 5)}[c.win]


def window(c):
    """The 9-entry window {c0, nc, cs, i0, ni, is, t0, nt, ts}, or None for the whole array."""
    w = [0, c.nc, 1, 0, c.ni, 1, 0, c.nt, 1]
    if c.win == "full":
        return None
    if c.win == "c0":
        w[0] = 1
    elif c.win == "cs2":
        w[2] = 2
    elif c.win == "rev":
        w[0], w[2] = c.nc - 1, -1
    elif c.win == "tsub":
        w[6] = 2
    return w


PLAN_KEYS = ("path", "tile", "halo", "rows", "G", "groups", "lds", "wgs", "vec", "ws")


def plan(pkg, L, dims, T, D, seg=0, win=None, ptr=None):
    """bldp_dedoppler_plan_f32 as a dict; ``ptr``: the input address (None: aligned)."""
    info = (ctypes.c_int64 * 10)(*([-1] * 10))
    keep, wp = pkg._lib.win_arg(win)
    rc = L.bldp_dedoppler_plan_f32(ptr, *dims, wp, T, D, seg, info)
    assert rc == 0, pkg._lib.last_error()
    p = dict(zip(PLAN_KEYS, (int(v) for v in info)))
    p["path"] = pkg._lib.DEDOPPLER_PATHS[p["path"]]
    return p


def case_plan(pkg, L, c):
    return plan(pkg, L, array_shape(c), c.T, c.D, c.seg, window(c))
