"""CPU: the codes and messages of the time-moment family (kurtosis over blocks,
skewness, moments: device, band and host entries, plans and the shape query)
for calls that return before any launch, and which of two errors wins when a
call is wrong twice.  The table is what the library answered at 0b0421b, before
the family went through one planner and one runner; it was recorded by running
that library, not derived from the code.  Pointers that are not null are
made-up addresses: nothing dereferences them on these paths."""
from __future__ import annotations

import ctypes

import pytest

P, I64 = ctypes.c_void_p, ctypes.c_int64
DIMS = (512, 1, 1024)  # (nchan, nif, ntime) of every call
A = 0x10000000  # the input (bank k at A + k MiB)
O = [0x40000000 + q * 0x1000000 for q in range(4)]  # the output planes
WINS = {"oob": (0, 512, 1, 0, 1, 1, 1000, 32, 1),  # past the last spectrum
        "empty": (0, 0, 1, 0, 1, 1, 0, 64, 1),  # no channels
        "nospectra": (0, 512, 1, 0, 1, 1, 5, 0, 1)}  # no blocks
PREFIX = {"kurtosis_blocks": "tblock kurtosis: ", "skewness": "skewness: ", "moments": "moments: ",
          "kurtosis": ""}
GROUPS = {"KB": "kb bkb kbh", "SK": "sk bsk skh", "MO": "mo bmo moh", "ONE": "kb sk mo",
          "BAND": "bkb bsk bmo", "HOST": "kbh skh moh", "ALL": "kb bkb kbh sk bsk skh mo bmo moh"}
ENTRY = {"kb": ("kurtosis_blocks", ""), "bkb": ("kurtosis_blocks", "band"),
         "kbh": ("kurtosis_blocks", "host"), "sk": ("skewness", ""), "bsk": ("skewness", "band"),
         "skh": ("skewness", "host"), "mo": ("moments", ""), "bmo": ("moments", "band"),
         "moh": ("moments", "host"), "kh": ("kurtosis", "host")}

# faults: tneg / tnd = tblock -1 / 3 (no divisor), nb0 / nb65 = nbank, nullarr =
# null pointer array, nullbank = a null bank (the only one, or bank 1 of 3),
# oob / empty / nospectra = WINS, nullout = every output null, ldi / ldb =
# out_ld_i / out_ld_b 511, ovl = planes 1 and 3 one element apart, ovin = plane 2
# inside the input.  "{p}" is the family's PREFIX.
# (faults, tblock, entries, code, message)
TABLE = [
    ("tneg", 16, "KB", -1, "tblock=-1 must be >= 1"),
    ("tneg", 16, "SK MO", -1, "{p}tblock=-1 must be >= 0"),
    ("tnd", 16, "ALL", -2, "DimensionMismatch: tblock=3 does not divide ntime=1024"),
    ("nb0", 16, "BAND", -1, "nbank=0 outside 1..64"),
    ("nb65", 16, "BAND", -1, "nbank=65 outside 1..64"),
    ("nullarr", 16, "BAND", -1, "{p}null input pointer array"),
    ("nullbank", 16, "ONE", -1, "{p}null input pointer (bank 0)"),
    ("nullbank", 16, "BAND", -1, "{p}null input pointer (bank 1)"),
    ("nullbank", 16, "HOST", -1, "{p}null pointer"),
    ("oob", 16, "ALL", -6, "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("empty", 16, "ALL", 0, ""),
    ("nospectra", 16, "ALL", 0, ""),
    ("nullout", 16, "kb bkb sk bsk", -1, "{p}null output pointer"),
    ("nullout", 16, "kbh skh", -1, "{p}null pointer"),
    ("nullout", 16, "MO", -1, "{p}every output plane is null"),
    ("ldi", 16, "ONE", -1, "{p}out strides (511, 512) overlap for a (512, 1, 64) result"),
    ("ldb", 16, "ONE", -1, "{p}out strides (512, 511) overlap for a (512, 1, 64) result"),
    ("ovl", 16, "mo bmo", -1, "{p}output planes 1 and 3 overlap"),
    ("ovl", 16, "moh", -1, "{p}output planes overlap"),
    ("ovin", 16, "mo bmo", -1, "{p}output plane 2 overlaps the input (bank 0)"),
    # wrong twice
    ("tneg+nb0", 16, "bkb", -1, "tblock=-1 must be >= 1"),
    ("tneg+nb0", 16, "bsk bmo", -1, "{p}tblock=-1 must be >= 0"),
    ("tneg+nullarr", 16, "bkb", -1, "{p}null input pointer array"),
    ("tneg+nullarr", 16, "bsk bmo", -1, "{p}tblock=-1 must be >= 0"),
    ("nb0+tnd", 16, "bkb bsk", -2, "DimensionMismatch: tblock=3 does not divide ntime=1024"),
    ("nb0+tnd", 16, "bmo", -1, "nbank=0 outside 1..64"),
    ("nb65+oob", 16, "bkb bsk", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("nb65+oob", 16, "bmo", -1, "nbank=65 outside 1..64"),
    ("nullarr+oob", 16, "BAND", -1, "{p}null input pointer array"),
    ("nullarr+nb0", 16, "BAND", -1, "{p}null input pointer array"),
    ("tnd+oob", 16, "ALL", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("oob+nullbank", 16, "ALL", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("nb65+nullbank", 16, "BAND", -1, "nbank=65 outside 1..64"),
    ("empty+nullout", 16, "ALL", 0, ""),
    ("nullbank+nullout", 16, "ONE", -1, "{p}null input pointer (bank 0)"),
    ("nullbank+nullout", 16, "BAND", -1, "{p}null input pointer (bank 1)"),
    ("nullbank+nullout", 16, "kbh skh", -1, "{p}null pointer"),
    ("nullbank+nullout", 16, "moh", -1, "{p}every output plane is null"),
    ("nullbank+ldi", 16, "ONE", -1, "{p}null input pointer (bank 0)"),
    ("nullout+ldi", 16, "kb sk", -1, "{p}null output pointer"),
    ("nullout+ldi", 16, "mo", -1, "{p}out strides (511, 512) overlap for a (512, 1, 64) result"),
    ("nullout+ldb", 16, "kb sk", -1, "{p}null output pointer"),
    ("nullout+ldb", 16, "mo", -1, "{p}out strides (512, 511) overlap for a (512, 1, 64) result"),
    ("ldi+ovl", 16, "mo", -1, "{p}out strides (511, 512) overlap for a (512, 1, 64) result"),
    ("ldb+ovin", 16, "mo", -1, "{p}out strides (512, 511) overlap for a (512, 1, 64) result"),
    ("ldi+ldb", 16, "ONE", -1, "{p}out strides (511, 511) overlap for a (512, 1, 64) result"),
    # tblock = 0: the whole window, except for the kurtosis over blocks
    ("", 0, "KB", -1, "tblock=0 must be >= 1"),
    ("nb65", 0, "bkb", -1, "tblock=0 must be >= 1"),
    ("nb65", 0, "bsk bmo", -1, "nbank=65 outside 1..64"),
    ("nullbank", 0, "KB", -1, "tblock=0 must be >= 1"),
    ("nullbank", 0, "sk mo", -1, "{p}null input pointer (bank 0)"),
    ("nullbank", 0, "bsk bmo", -1, "{p}null input pointer (bank 1)"),
    ("nullbank", 0, "skh moh", -1, "{p}null pointer"),
    ("nullbank", None, "kh", -1, "null pointer"),
    ("oob", 0, "ALL", -6, "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("oob", None, "kh", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("empty", 0, "KB", -1, "tblock=0 must be >= 1"),
    ("empty", 0, "SK MO", 0, ""),
    ("empty", None, "kh", 0, ""),
    ("nullout", 0, "KB", -1, "tblock=0 must be >= 1"),
    ("nullout", 0, "sk bsk", -1, "{p}null output pointer"),
    ("nullout", 0, "skh", -1, "{p}null pointer"),
    ("nullout", 0, "MO", -1, "{p}every output plane is null"),
    ("nullout", None, "kh", -1, "null pointer"),
    ("ldi", 0, "kb", -1, "tblock=0 must be >= 1"),
    ("ldi", 0, "sk", -1, "{p}out strides (511, 0) overlap for a (512, 1) result"),
    ("ldi", 0, "mo", -1, "{p}out strides (511, 512) overlap for a (512, 1, 1) result"),
    ("ovl", 0, "mo bmo", -1, "{p}output planes 1 and 3 overlap"),
    ("ovl", 0, "moh", -1, "{p}output planes overlap"),
    ("nb0+oob", 0, "bkb bsk", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("nb0+oob", 0, "bmo", -1, "nbank=0 outside 1..64"),
    ("nullbank+nullout", 0, "KB", -1, "tblock=0 must be >= 1"),
    ("nullbank+nullout", 0, "sk mo", -1, "{p}null input pointer (bank 0)"),
    ("nullbank+nullout", 0, "bsk bmo", -1, "{p}null input pointer (bank 1)"),
    ("nullbank+nullout", 0, "skh", -1, "{p}null pointer"),
    ("nullbank+nullout", 0, "moh", -1, "{p}every output plane is null"),
    ("nullbank+nullout", None, "kh", -1, "null pointer"),
    ("nullout+ldi", 0, "kb", -1, "tblock=0 must be >= 1"),
    ("nullout+ldi", 0, "sk", -1, "{p}null output pointer"),
    ("nullout+ldi", 0, "mo", -1, "{p}out strides (511, 512) overlap for a (512, 1, 1) result"),
    ("ldi+ovin", 0, "mo", -1, "{p}out strides (511, 512) overlap for a (512, 1, 1) result"),
]

# The plan entries and bldp_kurtosis_blocks_shape ("ksh") with a null input:
# (window, tblock, null info / dims, entries, code, message)
PLANS = [
    (None, 16, True, "kbp skp mop", -1, "null info"),
    (None, -1, True, "ksh", -1, "null dims"),
    ("oob", 3, True, "kbp skp mop", -1, "null info"),
    (None, -1, False, "kbp ksh", -1, "tblock=-1 must be >= 1"),
    (None, -1, False, "skp mop", -1, "{p}tblock=-1 must be >= 0"),
    (None, 0, False, "kbp ksh", -1, "tblock=0 must be >= 1"),
    (None, 0, False, "skp mop", 0, ""),
    (None, 3, False, "kbp skp mop ksh", -2,
     "DimensionMismatch: tblock=3 does not divide ntime=1024"),
    (None, 16, False, "kbp skp mop ksh", 0, ""),
    ("oob", -1, False, "kbp ksh", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("oob", -1, False, "skp mop", -1, "{p}tblock=-1 must be >= 0"),
    ("oob", 3, False, "kbp skp mop ksh", -6,
     "BoundsError: window 1001:1:1032 (1-based) outside axis 3 of size 1024"),
    ("empty", 3, False, "kbp skp mop ksh", -2,
     "DimensionMismatch: tblock=3 does not divide ntime=64"),
    ("nospectra", 3, False, "kbp skp mop ksh", 0, ""),
    ("nospectra", 0, False, "kbp ksh", -1, "tblock=0 must be >= 1"),
]


def entries(spec):
    return " ".join(GROUPS.get(tok, tok) for tok in spec.split()).split()


def window(faults):
    w = next((WINS[k] for k in WINS if k in faults), None)
    wa = (I64 * 9)(*w) if w else None
    return wa, ctypes.cast(wa, P) if w else None


def call(L, entry, faults, tblock):
    kind, form = ENTRY[entry]
    f = set(faults.split("+")) - {""}
    if "tneg" in f:
        tblock = -1
    if "tnd" in f:
        tblock = 3
    nbank = 0 if "nb0" in f else 65 if "nb65" in f else 3 if form == "band" else 1
    ptrs = [A + 0x100000 * k for k in range(max(nbank, 1))]
    if "nullbank" in f:
        ptrs[min(1, len(ptrs) - 1)] = None
    arr = (P * len(ptrs))(*ptrs)
    keep, wp = window(f)
    planes = list(O) if kind == "moments" else [O[0]]
    if "nullout" in f:
        planes = [None] * len(planes)
    if "ovl" in f:
        planes = [None, O[0], None, O[0] + 8]
    if "ovin" in f:
        planes = [None, None, A + 4096, None]
    tb = () if tblock is None else (tblock,)
    if form == "host":
        return getattr(L, f"bldp_{kind}_host_f32")(0, ptrs[0], *DIMS, wp, *tb, *planes)
    if form == "band":
        inp = None if "nullarr" in f else ctypes.cast(arr, P)
        return getattr(L, f"bldp_band_{kind}_f32")(nbank, inp, *DIMS, wp, *tb, *planes, None)
    return getattr(L, f"bldp_{kind}_f32")(ptrs[0], *DIMS, wp, *tb, *planes,
                                          511 if "ldi" in f else 512, 511 if "ldb" in f else 512,
                                          None)


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def test_codes_and_messages(pkg, L):
    for faults, tblock, spec, code, msg in TABLE:
        for e in entries(spec):
            rc = call(L, e, faults, tblock)
            got = pkg._lib.last_error() if rc else ""
            assert (rc, got) == (code, msg.format(p=PREFIX[ENTRY[e][0]])), (faults, tblock, e)


def test_plan_codes_and_messages(pkg, L):
    names = {"kbp": "kurtosis_blocks", "skp": "skewness", "mop": "moments"}
    for wname, tblock, null, spec, code, msg in PLANS:
        keep, wp = window({wname})
        for e in spec.split():
            if e == "ksh":
                rc = L.bldp_kurtosis_blocks_shape(*DIMS, wp, tblock, None if null else (I64 * 3)())
                p = ""
            else:
                rc = getattr(L, f"bldp_{names[e]}_plan_f32")(None, *DIMS, wp, tblock,
                                                             None if null else (I64 * 4)())
                p = PREFIX[names[e]]
            got = pkg._lib.last_error() if rc else ""
            assert (rc, got) == (code, msg.format(p=p)), (wname, tblock, null, e)
