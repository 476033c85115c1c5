"""CPU: the codes and messages of the block operations (reduce, tstat, quantile,
quantiles, outliers, argext, masked reduce, histogram, hits, fold, unfold: plan,
single, band and host entries, and the two shape queries) for calls that return
before any launch, and which of two refusals wins when a call is wrong twice.
The answers in golden/block_family_errors.json are what the library answered at
4ff0163, before the families shared one front end; they were recorded by running
that library, not derived from the code.  Pointers that are not null are
made-up addresses: nothing dereferences them on these paths (the host forms'
`total` of a hits call is written, so it is a real word)."""
from __future__ import annotations

import ctypes
import itertools
import json
import os

import pytest

P, I64, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "block_family_errors.json")
DIMS = (512, 2, 64)  # (nchan, nif, ntime)
BIG = (1 << 20, 1, 1 << 12)  # an array whose one block is 2^32 samples
A = 0x10000000  # the input (bank k at A + k MiB)
O = [0x40000000 + q * 0x1000000 for q in range(4)]  # the outputs
M = 0x60000000  # the mask, or the profile
WINS = {"oob": (0, 512, 1, 0, 2, 1, 60, 8, 1),  # past the last spectrum
        "empty": (0, 0, 1, 0, 2, 1, 0, 64, 1),  # no channels
        "rev": (383, 128, -2, 1, 1, 1, 8, 32, 1)}  # channels 384, 382, ..., 130 (1-based), IF 2
REV_LO, REV_HI = 129 + 512 * (1 + 2 * 8), 383 + 512 * (1 + 2 * 39)  # its lowest / highest element

# family: (entry name, message prefix, outputs, aux ("mask" / "prof" / None), has out strides,
#          31-bit block check, axis)
FAMILIES = {
    "reduce": ("reduce", "", ["out"], None, False, False, None),
    "tstat": ("tstat", "tstat: ", ["out"], None, True, False, None),
    "quantile0": ("quantile", "quantile: ", ["out"], None, False, False, 0),
    "quantile2": ("quantile", "quantile: ", ["out"], None, True, False, 2),
    "quantiles0": ("quantiles", "quantiles: ", ["out"], None, False, False, 0),
    "quantiles2": ("quantiles", "quantiles: ", ["out"], None, True, False, 2),
    "outliers0": ("outliers", "outliers: ", ["med", "mad", "count", "mask"], None, True, False, 0),
    "outliers2": ("outliers", "outliers: ", ["med", "mad", "count", "mask"], None, True, False, 2),
    "argext": ("argext", "argext: ", ["idx", "val"], None, True, True, None),
    "masked": ("masked_reduce", "masked reduce: ", ["out", "kept"], "mask", True, True, None),
    "histogram": ("histogram", "histogram: ", ["out"], None, True, True, None),
    "hits": ("hits", "hits: ", ["idx", "val", "total"], "mask", False, False, None),
    "fold": ("fold", "fold: ", ["out", "kept"], "mask", True, True, None),
    "unfold": ("unfold", "unfold: ", ["out"], "prof", True, False, None),
}
FORMS = ("plan", "single", "band", "host")

# faults: badop = the family's own first check (an unknown op, axis, np, n, nbins,
# cap or nfpc); nb0 / nb65 = nbank; nullarr = null pointer array; nullbank = a null
# bank (the only one, or bank 1 of 3); nullout = every output null; no:X = output
# X null (no fault by itself); nullaux = null mask / profile; oob / empty / rev =
# WINS; fnd / tnd = a channel / time factor that does not divide; big = a block of
# 2^32 samples; ldi / ldt / ldq = an output stride one too short; pldi = a
# negative profile stride; negm0..2 = a negative mask stride; in0:X / inL:X =
# output X inside the window of bank 0 / of the last bank; last:X = X starting at
# the last element of the window "rev", first:X = X ending in its first; aux:X = X
# inside the mask / profile; pair:X:Y = Y four bytes behind X; nullinfo = the plan
# entries' null info.
GROUP = {"badop": "op", "nb0": "nbank", "nb65": "nbank", "oob": "window", "empty": "window",
         "fnd": "factors", "tnd": "factors", "big": "factors", "nullarr": "null",
         "nullbank": "null", "nullout": "null", "nullaux": "null", "nullinfo": "null",
         "ldi": "strides", "ldt": "strides", "ldq": "strides", "pldi": "strides",
         "negm0": "strides", "negm1": "strides", "negm2": "strides", "in0": "overlaps",
         "inL": "overlaps", "last": "overlaps", "first": "overlaps", "aux": "overlaps",
         "pair": "overlaps"}


def faults_of(fam, form):
    """The single faults that `form` of `fam` refuses (or answers 0 for: empty)."""
    name, _, outs, aux, strides, big, axis = FAMILIES[fam]
    base = name.rstrip("02")
    f = ["badop", "oob", "fnd", "tnd"]
    if base in ("tstat",) or axis == 2:
        f.remove("fnd")
    if axis == 0 or base == "hits":
        f.remove("tnd")
    if base == "hits":
        f.remove("fnd")
    if big:
        f.append("big")
    # (the masked reduce's plan entry takes no op; the reduce's host form leaves
    # the op to the device call it makes after staging)
    if (base == "masked_reduce" and form == "plan") or (base == "reduce" and form == "host"):
        f.remove("badop")
    if aux == "mask":
        f += ["negm0", "negm1", "negm2"]
    if form == "plan":
        return f + ["empty", "nullinfo"]
    f.append("nullout")
    if not (base == "hits" and form != "host"):  # (the device forms clear `total`: a launch)
        f.append("empty")
    f.append("nullbank")
    if aux and base != "fold":  # (a fold without a mask is a fold)
        f.append("nullaux")
    if form == "host":
        return f
    if form == "band":
        f += ["nb0", "nb65", "nullarr"]
    if form == "single" and strides:
        f += ["ldi", "ldt"]
        if base == "histogram":
            f.append("ldq")
    if form == "single" and base == "quantiles":
        f.append("ldq")
    if base == "unfold":
        f.append("pldi")
    if base in ("argext", "masked_reduce", "histogram", "hits", "fold", "unfold", "outliers"):
        for o in outs:
            f.append(f"in0:{o}")
            if form == "band":
                f.append(f"inL:{o}")
            if aux:
                f.append(f"aux:{o}")
        if base != "outliers":  # (outliers checks the whole arrays, not the window)
            f += [f"last:{outs[0]}", f"first:{outs[0]}"]
        f += [f"pair:{x}:{y}" for x, y in itertools.combinations(outs, 2)]
    return f


def pairs_of(fam, form):
    """Calls that are wrong twice: one fault of every group against one of every
    other, and the pairs within the null pointers and within the overlaps."""
    singles = faults_of(fam, form)
    rep = {}
    for s in singles:
        if s not in ("empty", "big", "nullinfo"):
            rep.setdefault(GROUP[s.split(":")[0]], s)
    out = [f"{a}+{b}" for a, b in itertools.combinations(rep.values(), 2)]
    extra = [("empty", "nullout"), ("empty", "nullbank"), ("nullbank", "nullout"),
             ("nullout", "nullaux"), ("nullbank", "nullaux"), ("nullarr", "nb0"),
             ("nullarr", "nullbank"), ("big", "negm0"), ("big", "oob"), ("big", "nullbank"),
             ("negm1", "nullbank"), ("negm2", "ldi"), ("ldi", "ldt"), ("nullinfo", "oob"),
             ("nullinfo", "badop"), ("nb65", "nullbank")]
    ovl = [s for s in singles if GROUP[s.split(":")[0]] == "overlaps"]
    outs = FAMILIES[fam][2]
    for a, b in itertools.combinations(ovl, 2):
        ka, kb = a.split(":"), b.split(":")
        # two overlaps that move different outputs (a pair moves its second)
        if ka[0] in ("last", "first") or kb[0] in ("last", "first") or ka[-1] == kb[-1]:
            continue
        if ka[0] == kb[0] and ka[0] != "pair":
            continue
        extra.append((a, b))
    for o in outs[:-1]:
        extra.append((f"no:{o}", f"in0:{outs[-1]}"))
    for a, b in extra:
        ok = all(x in singles or x.startswith("no:") for x in (a, b))
        if ok and f"{a}+{b}" not in out and not (fam == "hits" and "empty" in (a, b)
                                                  and form != "host" and form != "plan"):
            out.append(f"{a}+{b}")
    # a pair that leaves no fault behind is no row: a null output cannot overlap
    return [p for p in out if not p.startswith("nullout+") or GROUP[p.split("+")[1].split(":")[0]]
            != "overlaps"]


def rows():
    for fam in FAMILIES:
        for form in FORMS:
            for f in faults_of(fam, form) + pairs_of(fam, form):
                yield fam, form, f
    for sh in ("reduce_shape", "fold_shape"):
        for f in ("nullinfo", "oob", "empty", "fnd", "tnd", "nullinfo+oob", "oob+fnd", "fnd+tnd",
                  "empty+tnd") + (("badop", "badop+oob") if sh == "fold_shape" else ()):
            yield sh, "shape", f


def call(L, fam, form, faults, keep):
    """Make the call; `keep` holds the ctypes objects it points to."""
    f = set(faults.split("+"))
    has = lambda k: any(x.split(":")[0] == k for x in f)  # noqa: E731
    dims = BIG if "big" in f else DIMS
    wname = next((k for k in WINS if k in f), "rev" if has("last") or has("first") else None)
    win = WINS.get(wname)
    if win and dims is BIG:
        win = (0, BIG[0], 1, 0, 1, 1, BIG[2] - 4, 8, 1)
    wp = None
    if win:
        keep.append((I64 * 9)(*win))
        wp = ctypes.cast(keep[-1], P)
    F, T = (BIG[0], BIG[2]) if "big" in f else (8, 4)
    if "big" in f and fam == "fold":  # (nfpc 1: every channel is a coarse one)
        F = 1
    if "fnd" in f:
        F = 7
    if "tnd" in f:
        T = 5
    if fam.endswith("_shape"):
        sh = None if "nullinfo" in f else (I64 * 3)()
        if fam == "fold_shape" and "badop" in f:
            F = 0
        return getattr(L, f"bldp_{fam}")(*dims, wp, F, T, sh)
    name, _, outs, aux, _, _, axis = FAMILIES[fam]
    base = name
    nbank = 0 if "nb0" in f else 65 if "nb65" in f else 3 if form == "band" else 1
    ptrs = [A + 0x100000 * k for k in range(max(nbank, 1))]
    if "nullbank" in f:
        ptrs[min(1, len(ptrs) - 1)] = None
    keep.append((P * len(ptrs))(*ptrs))
    arr = None if "nullarr" in f else ctypes.cast(keep[-1], P)
    head = {"plan": (ptrs[0],), "single": (ptrs[0],), "band": (nbank, arr),
            "host": (0, ptrs[0])}[form] + (*dims, wp)
    # the window's counts and the result's dense shape
    wc = (win[1], win[4], win[7]) if win else dims
    nc, ni, nt = wc
    if base in ("reduce", "argext", "masked_reduce", "histogram"):
        d = (nc // F, ni, nt // T)
    elif base == "tstat" or axis == 2:
        d = (nc, ni, nt // T)
    elif axis == 0:
        d = (nc // F, ni, nt)
    elif base == "fold":
        d = (F, ni, nt // T)
    else:  # unfold (hits has no strides)
        d = (nbank * nc, ni, nt)
    li, lt = d[0], d[0] * d[1]
    lq = lt * d[2]
    if "ldi" in f:
        li -= 1
    if "ldt" in f:
        lt = (d[1] - 1) * li + d[0] - 1
    if "ldq" in f:
        lq = (d[2] - 1) * lt + (d[1] - 1) * li + d[0] - 1
    o = dict(zip(outs, O))
    if form == "host" and base == "hits":
        keep.append(ctypes.c_uint64(7))
        o["total"] = ctypes.addressof(keep[-1])
    last = ptrs[-1] if ptrs[-1] else A
    for x in f:
        k = x.split(":")
        if k[0] == "in0":
            o[k[1]] = A + 64
        elif k[0] == "inL":
            o[k[1]] = last + 64
        elif k[0] == "last":
            o[k[1]] = A + 4 * REV_HI
        elif k[0] == "first":  # (an 8-byte entry of a hits idx ends there too)
            o[k[1]] = A + 4 * REV_LO - (4 if base == "hits" else 0)
        elif k[0] == "aux":
            o[k[1]] = M + 8
    for x in f:
        k = x.split(":")
        if k[0] == "pair":
            o[k[2]] = o[k[1]] + 4
    if "nullout" in f:
        o = dict.fromkeys(outs)
    for x in f:
        if x.startswith("no:"):
            o[x[3:]] = None
    ov = [o[k] for k in outs]
    mask = None if "nullaux" in f else M
    ml = None
    NC = nbank * nc
    for ax in range(3):
        if f"negm{ax}" in f:
            mld = [1, NC, NC * ni]
            mld[ax] = -1
            keep.append((I64 * 3)(*mld))
            ml = ctypes.cast(keep[-1], P)
    info = None if "nullinfo" in f else ctypes.cast((I64 * 10)(), P)
    if info:
        keep.append(info)
    bad = "badop" in f
    st = {"plan": (), "single": (li, lt, None), "band": (None,), "host": ()}[form]
    if base == "reduce":
        body = (F, T, 99 if bad else 0)
        fn = {"plan": "bldp_reduce_plan_f32", "single": "bldp_reduce_strided_f32",
              "band": "bldp_band_reduce_f32", "host": "bldp_reduce_host_f32"}[form]
        return getattr(L, fn)(*head, *body, *ov, *((info,) if form == "plan" else st))
    fn = getattr(L, {"plan": f"bldp_{base}_plan_f32", "single": f"bldp_{base}_f32",
                     "band": f"bldp_band_{base}_f32", "host": f"bldp_{base}_host_f32"}[form])
    if base == "tstat":
        body = (T, 0 if bad else 6)
        return fn(*head, *body, *ov, *((info,) if form == "plan" else st))
    if base == "quantile":
        body = (1 if bad else axis, F if axis == 0 else T, D(0.25))
        return fn(*head, *body, *ov, *((info,) if form == "plan" else st))
    if base == "quantiles":
        keep.append((D * 3)(0.25, 0.5, 0.9))
        body = (axis, F if axis == 0 else T, 0 if bad else 3, ctypes.cast(keep[-1], P))
        st = {"plan": (info,), "single": (li, lt, lq, None), "band": (None,), "host": ()}[form]
        return fn(*head, *body, *ov, *st)
    if base == "outliers":
        n = 1 if bad else F if axis == 0 else T
        if form == "plan":
            return fn(*head, axis, n, 1, info)
        return fn(*head, axis, n, D(3.0), *ov, *st)
    if base == "argext":
        body = (F, T, 5 if bad else 0)
        if form == "plan":
            return fn(*head, *body, ov[0], info)
        return fn(*head, *body, *ov, *st)
    if base == "masked_reduce":
        if form == "plan":
            return fn(*head, F, T, mask, ml, info)
        return fn(*head, F, T, 2 if bad else 0, mask, ml, *ov, *st)
    if base == "histogram":
        body = (F, T, 0 if bad else 16, D(0.0), D(1.0))
        st = {"plan": (info,), "single": (li, lt, lq, None), "band": (None,), "host": ()}[form]
        return fn(*head, *body, *(ov if form != "plan" else ()), *st)
    if base == "hits":
        cap = -1 if bad else 100
        if form == "plan":
            return fn(*head, mask, ml, cap, info)
        return fn(*head, mask, ml, cap, *ov, *(() if form == "host" else (None,)))
    if base == "fold":
        if form == "plan":
            return fn(*head, 0 if bad else F, T, mask, ml, info)
        return fn(*head, F, T, 2 if bad else 0, mask, ml, *ov, *st)
    # unfold: the profile is dense (nfpc, ni, nto)
    pli, plt = (-1 if "pldi" in f else F), F * ni
    if form == "plan":
        return fn(*head, 0 if bad else F, T, mask, pli, plt, ov[0], li, lt, info)
    if form == "host":
        return fn(*head, F, T, 7 if bad else 0, mask, *ov)
    return fn(*head, F, T, 7 if bad else 0, mask, pli, plt, *ov,
              *((li, lt, None) if form == "single" else (None,)))


def answers(pkg):
    """{family/form/faults: [code, message]} of the loaded library."""
    L = pkg._lib.lib()
    got = {}
    for fam, form, faults in rows():
        keep = []
        rc = call(L, fam, form, faults, keep)
        got[f"{fam}/{form}/{faults}"] = [rc, pkg._lib.last_error() if rc else ""]
    return got


def unpack():
    """The recorded table: golden holds the distinct answers once, and for every
    family its faults with the index of each form's answer."""
    with open(GOLDEN) as fh:
        g = json.load(fh)
    want = {}
    for fam, by_fault in g["rows"].items():
        for faults, by_form in by_fault.items():
            for form, k in by_form.items():
                want[f"{fam}/{form}/{faults}"] = g["answers"][k]
    return want


# The rows whose answer differs from the recording on purpose.  bldp_hits_f32 and
# bldp_band_hits_f32 now test every output against the input windows and the mask
# before they test the outputs against each other, as the masked reduce and the
# fold always did; only a call with two overlap faults can tell, and the code is
# BLDP_EINVAL either way.  golden keeps what 4ff0163 answered ("was").
_IN, _AUX = "hits: {} overlaps the input window (bank {})", "hits: {} overlaps the mask"
REORDERED = {
    "hits/single/in0:val+pair:idx:total": [-1, _IN.format("val", 0)],  # was idx and total overlap
    "hits/band/in0:val+pair:idx:total": [-1, _IN.format("val", 0)],  # was idx and total overlap
    "hits/band/inL:val+pair:idx:total": [-1, _IN.format("val", 2)],  # was idx and total overlap
    "hits/single/aux:val+pair:idx:total": [-1, _AUX.format("val")],  # was idx and total overlap
    "hits/band/aux:val+pair:idx:total": [-1, _AUX.format("val")],  # was idx and total overlap
    "hits/single/in0:total+pair:idx:val": [-1, _IN.format("total", 0)],  # was idx and val overlap
    "hits/band/in0:total+pair:idx:val": [-1, _IN.format("total", 0)],  # was idx and val overlap
    "hits/band/inL:total+pair:idx:val": [-1, _IN.format("total", 2)],  # was idx and val overlap
    "hits/single/aux:total+pair:idx:val": [-1, _AUX.format("total")],  # was idx and val overlap
    "hits/band/aux:total+pair:idx:val": [-1, _AUX.format("total")],  # was idx and val overlap
}


@pytest.fixture(scope="module")
def got(pkg):
    return answers(pkg)


def test_table_is_whole(got):
    want = unpack()
    assert sorted(want) == sorted(got)
    assert len(want) > 1500


def test_no_row_reaches_a_launch():
    # a refusal, or the 0 of an empty window: never a HIP call's failure, and
    # never the 0 of a call that went through
    for key, (rc, msg) in unpack().items():
        faults = key.split("/")[2].split("+")
        assert rc in (0, -1, -2, -6) and "device" not in msg, key
        assert (msg == "" and "empty" in faults) if rc == 0 else msg, key


def test_codes_and_messages(got):
    want = unpack()
    want.update(REORDERED)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} rows differ, e.g. {sorted(wrong.items())[:5]}"
