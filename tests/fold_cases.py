"""The case table of tests/test_gpu_fold.py, kept apart so that the CPU suite can
ask bldp_fold_plan_f32 which kernels the GPU cases run (test_fold_host.py).

A case is a window of J coarse channels of nfpc fine channels, ni IFs and nt
spectra folded over blocks of T spectra (None: the whole selected time range),
how the window lies in its array, and the mask.  ``plan`` is what the library
plans for it on a 256-CU device with 256-byte aligned tensors: (path, vector
loads, mask load form, chunked).

Windows: "full" the whole array; "c0" channels from 1 (off the float4 boundary);
"cs2" every second channel; "rev" the channels reversed; "ts3" every third
spectrum; "if1" IF 1 of 2 picked by index.
Masks: None, or a name of test_gpu_fold.masks()."""
from __future__ import annotations

from collections import namedtuple

Case = namedtuple("Case", "nfpc J ni nt T win mask plan")

CASES = [
    Case(1, 1, 1, 6, 1, "full", None, ("rows", 0, "none", False)),
    Case(1, 64, 2, 34, 17, "full", "random", ("rows", 0, "byte", False)),
    Case(2, 7, 1, 48, 16, "full", "zero", ("rows", 0, "byte", False)),
    Case(3, 3, 2, 9, 3, "full", "all", ("rows", 0, "byte", False)),
    Case(3, 64, 1, 40, None, "full", "bad_channels", ("rows", 0, "byte", True)),
    Case(4, 2, 2, 6, 2, "full", "random", ("rows", 1, "dword", False)),
    Case(4, 1, 1, 20000, None, "full", "random", ("rows", 1, "dword", True)),
    Case(5, 7, 1, 51, 17, "full", "bad_spectra", ("rows", 0, "row", False)),
    Case(8, 4, 2, 4099, None, "full", "random", ("rows", 1, "dword", True)),
    Case(8, 64, 1, 32, 16, "full", "odd_address", ("rows", 1, "byte", False)),
    Case(12, 3, 2, 4, 1, "full", "bool", ("rows", 1, "dword", False)),
    Case(64, 7, 1, 6, 3, "full", None, ("rows", 1, "none", False)),
    Case(64, 2, 2, 34, None, "c0", "random", ("rows", 0, "byte", True)),
    Case(256, 3, 1, 8, 2, "full", "bad_spectra", ("rows", 1, "row", False)),
    Case(256, 2, 2, 6, 3, "cs2", "random", ("cols", 0, "byte", False)),
    Case(1024, 5, 1, 273, None, "full", "random", ("cols", 1, "dword", True)),
    Case(1024, 2, 2, 32, 16, "full", "bad_channels", ("cols", 1, "dword", False)),
    Case(1028, 3, 1, 17, None, "full", "odd_address", ("cols", 1, "byte", True)),
    Case(2048, 1, 2, 4, 1, "full", None, ("cols", 1, "none", False)),
    Case(2048, 7, 1, 6, 2, "rev", "random", ("cols", 0, "byte", False)),
    Case(4100, 2, 1, 9, 3, "ts3", "zero", ("cols", 1, "dword", False)),
    Case(4100, 1, 1, 34, None, "if1", "bad_spectra", ("cols", 1, "row", True)),
    Case(12, 64, 1, 16, 16, "full", "bad_spectra", ("rows", 1, "row", False)),
    Case(256, 2, 1, 6, 2, "cs2", "bad_spectra", ("cols", 0, "row", False)),
    Case(1024, 3, 1, 4, 2, "c0", None, ("cols", 0, "none", False)),
]

# the band of three banks (one profile over all of them) and the unfold's windows
BAND_CASES = [Case(8, 4, 2, 40, None, "full", "random", None),
              Case(1024, 2, 1, 6, 3, "full", None, None),
              Case(3, 5, 1, 4, 2, "full", "bad_channels", None)]
UNFOLD_CASES = [(Case(8, 4, 2, 6, 2, "full", None, None), 1),
                (Case(1024, 2, 1, 6, 3, "full", None, None), 1),
                (Case(3, 5, 2, 4, 2, "full", None, None), 0),
                (Case(64, 2, 1, 5, None, "c0", None, None), 0),
                (Case(64, 2, 2, 6, 1, "cs2", None, None), 0),
                (Case(4, 3, 1, 9, 3, "ts3", None, None), 1)]


def case_id(c):
    return "nfpc%d-J%d-ni%d-nt%d-T%s-%s-%s" % (c.nfpc, c.J, c.ni, c.nt, c.T or "nt", c.win,
                                               c.mask or "nomask")


def array_shape(c):
    """(nchan, nif, ntime) of the array that holds the case's window."""
    nc = c.nfpc * c.J
    return {"full": (nc, c.ni, c.nt), "c0": (nc + 4, c.ni, c.nt), "cs2": (2 * nc, c.ni, c.nt),
            "rev": (nc, c.ni, c.nt), "ts3": (nc, c.ni, 3 * c.nt), "if1": (nc, 2, c.nt)}[c.win]


def window(c):
    """The 9-entry window {c0, nc, cs, i0, ni, is, t0, nt, ts}, or None for the whole array."""
    nc = c.nfpc * c.J
    w = [0, nc, 1, 0, c.ni, 1, 0, c.nt, 1]
    if c.win == "full":
        return None
    if c.win == "c0":
        w[0] = 1
    elif c.win == "cs2":
        w[2] = 2
    elif c.win == "rev":
        w[0], w[2] = nc - 1, -1
    elif c.win == "ts3":
        w[8] = 3
    elif c.win == "if1":
        assert c.ni == 1
        w[3] = 1
    return w


def mask_ld(c, nbank=1):
    """(mask address, mask_ld) of the case's mask as the plan call takes them: an
    address of None is an aligned mask; (None, None) no mask."""
    nc = nbank * c.nfpc * c.J
    if c.mask is None:
        return None, None
    if c.mask == "bad_channels":
        return None, [1, 0, 0]
    if c.mask == "bad_spectra":
        return None, [0, 0, 1]
    return ((1 << 20) + 1 if c.mask == "odd_address" else None), [1, nc, nc * c.ni]
