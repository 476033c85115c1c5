"""The table behind test_engine_front_errors.py (CPU tensors) and
test_gpu_engine_front.py (device tensors): every block operation of engine.py
(reduce, tstat, quantile, quantiles, outliers, argext, masked reduce, histogram,
hits, fold, unfold) in its four forms (single, plan, band, host), called wrong
once and wrong twice on one small geometry, and what Python answered: the
exception's class, its ``code`` where it has one, and its message.

One array of (16, 2, 8), fqavby 4, tavby 2, nfpc 4, nbins 4, ps (0.25, 0.5), two
banks.  With CPU inputs a call that gets as far as the device reports ``REACHED``;
with device inputs it launches a 256-element window and reports ``"ok"``."""
from __future__ import annotations

import itertools
import json

import numpy as np

GEO = (16, 2, 8)
F, T, NFPC, NBINS, PS, NB = 4, 2, 4, 4, (0.25, 0.5), 2
OOB = (0, 16, 1, 0, 2, 1, 6, 4, 1)  # past the last spectrum
FORMS = ("single", "plan", "band", "host")
REACHED = ["BLDPError", -3, "(reached the device)"]

# family: the four entry points, the dense result of the single form (None: no
# out argument), its planes, the mask / profile it takes, its axis, its faults
# of the "op" group per form ("-x": not in that form)
FAMILIES = {
    "reduce": (("reduce", "plan", "band_reduce", "reduce_host"), (4, 2, 4), 0, None, None,
               ["badop"]),
    "tstat": (("tstat", "tstat_plan", "band_tstat", "tstat_host"), (16, 2, 4), 0, None, None,
              ["badop"]),
    "quantile0": (("quantile", "quantile_plan", "band_quantile", "quantile_host"), (4, 2, 8), 0,
                  None, 0, ["badaxis", "badp"]),
    "quantile2": (("quantile", "quantile_plan", "band_quantile", "quantile_host"), (16, 2, 4), 0,
                  None, 2, ["badaxis", "badp"]),
    "quantiles0": (("quantiles", "quantiles_plan", "band_quantiles", "quantiles_host"), (4, 2, 8),
                   2, None, 0, ["badaxis", "badps"]),
    "quantiles2": (("quantiles", "quantiles_plan", "band_quantiles", "quantiles_host"),
                   (16, 2, 4), 2, None, 2, ["badaxis", "badps"]),
    "outliers0": (("outliers", "outliers_plan", "band_outliers", "outliers_host"), None, 0, None,
                  0, ["badaxis", "badn", "-plan:badnsigma", "-plan:badwhich", "-plan:noout"]),
    "outliers2": (("outliers", "outliers_plan", "band_outliers", "outliers_host"), None, 0, None,
                  2, ["badaxis", "badn", "-plan:badnsigma", "-plan:badwhich", "-plan:noout"]),
    "argext": (("argext", "argext_plan", "band_argext", "argext_host"), (4, 2, 4), 0, None, None,
               ["badop"]),
    "masked": (("masked_reduce", "masked_reduce_plan", "band_masked_reduce",
                "masked_reduce_host"), None, 0, "mask", None, ["-plan:badop"]),
    "histogram": (("histogram", "histogram_plan", "band_histogram", "histogram_host"), (4, 2, 4),
                  NBINS + 3, None, None, ["badnbins", "badnbinst", "badlohi"]),
    "hits": (("hits", "hits_plan", "band_hits", "hits_host"), None, 0, "mask", None,
             ["badmaxhits", "badmaxhitst"]),
    "fold": (("fold", "fold_plan", "band_fold", "fold_host"), None, 0, "mask", None,
             ["-plan:badop", "badnfpc"]),
    "unfold": (("unfold", "unfold_plan", "band_unfold", "unfold_host"), (16, 2, 8), 0, "prof",
               None, ["-plan:badop", "badnfpc"]),
}
# the forms that take a caller's out
TAKES_OUT = {"reduce": ("single", "band"), "tstat": ("single", "band"),
             "quantile0": ("single", "band"), "quantile2": ("single", "band"),
             "quantiles0": ("single", "band"), "quantiles2": ("single", "band"),
             "argext": ("single",), "histogram": ("single", "band"), "unfold": ("single", "plan")}
# faults only a device tensor reaches (test_gpu_engine_front.py)
GPU_ONLY = {"hostx", "ohost", "mhost", "phost", "bankshape", "banklayout", "oldi", "oldt",
            "ondense"}
GROUP = {"f64": "dtype", "nd2": "dtype", "corder": "dtype", "nobanks": "dtype", "hostx": "dtype",
         "bankshape": "dtype", "banklayout": "dtype", "oob": "window", "fnd": "factors",
         "tnd": "factors", "mdtype": "aux", "mrank": "aux", "mshape": "aux", "mneg": "aux",
         "mhost": "aux", "pdtype": "aux", "pshape": "aux", "pstrides": "aux", "phost": "aux",
         "otype": "out", "odtype": "out", "oshape": "out", "orank": "out", "ostrides": "out",
         "oplanes": "out", "ohost": "out", "oldi": "out", "oldt": "out", "ondense": "out",
         "lddiff": "out", "nonpair": "out", "vdtype": "out"}


def group(fault):
    return GROUP.get(fault, "op")


def faults_of(fam, form, gpu):
    """The single faults of one form of one family."""
    _, dims, K, aux, axis, ops = FAMILIES[fam]
    f = [o.split(":")[-1] for o in ops if not o.startswith(f"-{form}:")]
    f += ["f64", "nd2"]
    f.append({"host": "corder", "band": "nobanks"}.get(form, "hostx"))
    if form == "band":
        f += ["hostx", "bankshape", "banklayout"]
    f.append("oob")
    if fam != "hits" and fam != "tstat" and axis != 2:
        f.append("fnd")
    if fam != "hits" and axis != 0:
        f.append("tnd")
    if aux == "mask":
        f += ["mdtype", "mrank", "mshape"] + (["mneg"] if form == "host" else ["mhost"])
    if aux == "prof" and (form != "plan"):
        f += ["pdtype", "pshape", "pstrides"] + ([] if form == "host" else ["phost"])
    if aux == "prof" and form == "plan":
        f += ["pdtype", "pshape", "pstrides", "phost"]
    if form in TAKES_OUT.get(fam, ()):
        f += ["otype", "odtype", "oshape", "orank", "ostrides"]
        # (band_reduce does not ask where its out lies: a host out would reach the kernel)
        if not (fam == "reduce" and form == "band"):
            f.append("ohost")
        if form == "band":
            f.append("ondense")
        else:
            f += ["oldi", "oldt"]
        if K:
            f.append("oplanes")
        if fam == "argext":
            f += ["lddiff", "nonpair", "vdtype"]
    return [x for x in f if gpu or x not in GPU_ONLY]


def rows(gpu):
    """(family, form, faults): every single fault, then every pair of faults from
    different groups."""
    for fam in FAMILIES:
        for form in FORMS:
            singles = faults_of(fam, form, gpu)
            for s in singles:
                yield fam, form, s
            for a, b in itertools.combinations(singles, 2):
                if group(a) != group(b):
                    yield fam, form, f"{a}+{b}"


def _dense(torch, shape, dtype, dev):
    """A channel-fastest tensor of ``shape`` (fb_empty's layout, planes_empty's in 4-D)."""
    n = len(shape)
    return torch.zeros(tuple(reversed(shape)), dtype=dtype, device=dev).permute(
        *range(n - 1, -1, -1))


def _out(torch, dev, dims, K, dtype, fault):
    nc, ni, nt = dims
    full = (*dims, K) if K else tuple(dims)
    buf = torch.zeros(8192, dtype=dtype, device=dev)
    tail = (nc * ni * nt,) if K else ()
    if fault == "otype":
        return np.zeros(full, np.dtype(str(dtype).replace("torch.", "")), order="F")
    if fault == "odtype":
        return _dense(torch, full, torch.float64, dev)
    if fault == "oshape":
        return _dense(torch, (nc + 1, *full[1:]), dtype, dev)
    if fault == "orank":
        return _dense(torch, full, dtype, dev)[..., 0]
    if fault == "ostrides":
        return torch.zeros(full, dtype=dtype, device=dev)
    if fault == "ohost":
        return _dense(torch, full, dtype, "cpu")
    if fault == "oplanes":
        return torch.as_strided(buf, full, (1, nc, nc * ni, nc * ni * nt - 1))
    if fault == "oldi":
        return torch.as_strided(buf, full, (1, nc - 1, 2 * nc * ni) + tuple(2 * t for t in tail))
    if fault == "oldt":
        return torch.as_strided(buf, full, (1, nc, nc * ni - 1) + tail)
    if fault == "ondense":
        return _dense(torch, (nc + 1, *full[1:]), dtype, dev)[:nc]
    return _dense(torch, full, dtype, dev)


def build(torch, fam, form, faults, dev, with_out=False):
    """(entry point's name, args, kwargs) of the call with ``faults``."""
    f = set(faults.split("+")) if faults else set()
    fns, dims, K, aux, axis, _ = FAMILIES[fam]
    name = fns[FORMS.index(form)]
    base = fam.rstrip("02")
    nb = NB if form == "band" else 1
    # the data
    if form == "host":
        X = np.zeros(GEO, np.float32, order="F")
        X[1, 0, 0] = 3.0
        if "f64" in f:
            X = X.astype(np.float64)
        if "nd2" in f:
            X = np.asfortranarray(X[:, 0, :])
        if "corder" in f:
            X = np.ascontiguousarray(X)
    else:
        def bank(k):
            x = _dense(torch, GEO, torch.float32, "cpu" if "hostx" in f and k == nb - 1 else dev)
            if k == nb - 1:
                if "f64" in f:
                    x = x.double()
                if "nd2" in f:
                    x = x[:, 0, :]
                if form == "band" and "bankshape" in f:
                    x = x[:, :, :4]
                if form == "band" and "banklayout" in f:
                    x = _dense(torch, (20, 2, 8), torch.float32, dev)[:16]
            return x
        X = [bank(k) for k in range(nb)] if form == "band" else bank(0)
        if "nobanks" in f:
            X = []
    fq, tv = (3 if "fnd" in f else F), (3 if "tnd" in f else T)
    n = fq if axis == 0 else tv
    kw = {"win": OOB} if "oob" in f else {}
    # the mask or the profile
    A = None
    if aux == "mask":
        shape = (nb * GEO[0], GEO[1], GEO[2])
        if "mshape" in f:
            shape = (shape[0] - 1, *shape[1:])
        if "mrank" in f:
            shape = shape[:2]
        if form == "host":
            A = np.zeros(shape, np.float32 if "mdtype" in f else np.uint8, order="F")
            A[(1,) + (0,) * (len(shape) - 1)] = 1
            if "mneg" in f:
                A = A[::-1]
        else:
            A = _dense(torch, shape, torch.float32 if "mdtype" in f else torch.uint8,
                       "cpu" if "mhost" in f else dev)
            A[(1,) + (0,) * (len(shape) - 1)] = 1
    if aux == "prof":
        shape = (NFPC, GEO[1], GEO[2] // T - (1 if "pshape" in f else 0))
        if form == "host":
            A = np.ones(shape, np.float64 if "pdtype" in f else np.float32,
                        order="C" if "pstrides" in f else "F")
        else:
            pdev, pdt = ("cpu" if "phost" in f else dev), \
                (torch.float64 if "pdtype" in f else torch.float32)
            A = torch.ones(shape, dtype=pdt, device=pdev) if "pstrides" in f else \
                _dense(torch, shape, pdt, pdev) + 1
    # the caller's out
    ofault = next((x for x in f if group(x) == "out"), None)
    if form in TAKES_OUT.get(fam, ()) and (ofault or with_out):
        odims = (nb * dims[0], *dims[1:])
        odt = torch.int32 if fam in ("argext", "histogram") else torch.float32
        if fam == "argext" and ofault in ("lddiff", "nonpair", "vdtype"):
            kw["values"] = True
            idx = _out(torch, dev, odims, 0, torch.int32, None)
            val = _out(torch, dev, odims, 0, torch.float32, None)
            if ofault == "lddiff":
                val = _dense(torch, (odims[0] + 1, *odims[1:]), torch.float32, dev)[:odims[0]]
            if ofault == "vdtype":
                val = val.double()
            kw["out"] = idx if ofault == "nonpair" else (idx, val)
        else:
            kw["out"] = _out(torch, dev, odims, K, odt, ofault)
    elif fam == "argext" and form != "plan":
        kw["values"] = True
    if base == "reduce":
        return name, (X, fq, tv, "nope" if "badop" in f else "sum"), kw
    if base == "tstat":
        return name, (X, tv, "sum" if "badop" in f else "median"), kw
    if base == "quantile":
        return name, (X, n, 1.5 if "badp" in f else 0.25, 1 if "badaxis" in f else axis), kw
    if base == "quantiles":
        return name, (X, n, () if "badps" in f else PS, 1 if "badaxis" in f else axis), kw
    if base == "outliers":
        ax = 1 if "badaxis" in f else axis
        n = 1 if "badn" in f else n
        if form == "plan":
            return name, (X, n, ax), dict(kw, mask=True)
        which = ("x",) if "badwhich" in f else () if "noout" in f else ("median", "mad", "count")
        return name, (X, n, ax, -1.0 if "badnsigma" in f else 3.0), \
            dict(kw, mask="noout" not in f, which=which)
    if base == "argext":
        return name, (X, fq, tv, "nope" if "badop" in f else "argmax"), kw
    if base == "masked":
        if form == "plan":
            return name, (X, A, fq, tv), kw
        return name, (X, A, fq, tv, "max" if "badop" in f else "sum"), kw
    if base == "histogram":
        nbins = 0 if "badnbins" in f else 2.5 if "badnbinst" in f else NBINS
        return name, (X, nbins, 1.0 if "badlohi" in f else 0.0, 1.0, fq, tv), kw
    if base == "hits":
        return name, (X, A, -1 if "badmaxhits" in f else 2.5 if "badmaxhitst" in f else 8), kw
    nfpc = 0 if "badnfpc" in f else 3 if "fnd" in f else NFPC
    if base == "fold":
        if form == "plan":
            return name, (X, nfpc, tv), dict(kw, mask=A)
        return name, (X, nfpc, tv, "max" if "badop" in f else "mean", A), kw
    if form == "plan":  # unfold
        return name, (X, nfpc, tv), dict(kw, prof=A)
    return name, (X, A, nfpc, tv, "nope" if "badop" in f else "divide"), kw


def describe(r):
    """A result's dtypes, shapes and strides; a plan's keys, values and their types."""
    if isinstance(r, dict):
        return {k: describe(v) for k, v in r.items()}
    if isinstance(r, (tuple, list)):
        return [describe(v) for v in r]
    if isinstance(r, np.ndarray):
        return ["ndarray", str(r.dtype), list(r.shape), list(r.strides)]
    if hasattr(r, "stride"):
        return ["tensor", str(r.dtype), list(r.shape), list(r.stride())]
    return [type(r).__name__, r]


def answer(pkg, torch, fam, form, faults, dev, with_out=False):
    """What the call answers: [class, code, message], or ["ok", description].  With
    CPU inputs a call that passes every check of Python's (a host form) is
    ``REACHED``, whether the machine has a device to run it on or not."""
    name, args, kw = build(torch, fam, form, faults, dev, with_out)
    try:
        r = getattr(pkg.engine, name)(*args, **kw)
    except Exception as e:  # noqa: BLE001 (the answer is whatever is raised)
        code = getattr(e, "code", None)
        if code == pkg._lib.BLDP_EHIP or (dev == "cpu" and "device 0 not available" in str(e)):
            return list(REACHED)
        return [type(e).__name__, code if isinstance(code, int) else None, str(e)]
    return list(REACHED) if dev == "cpu" else ["ok", describe(r)]


def answers(pkg, torch, dev, gpu):
    return {f"{fam}/{form}/{faults}": answer(pkg, torch, fam, form, faults, dev)
            for fam, form, faults in rows(gpu)}


def good(pkg, torch, dev):
    """One good call of every family and form, and again with a caller's out."""
    got = {}
    for fam in FAMILIES:
        for form in FORMS:
            got[f"{fam}/{form}"] = answer(pkg, torch, fam, form, "", dev)
            if form in TAKES_OUT.get(fam, ()):
                got[f"{fam}/{form}/out"] = answer(pkg, torch, fam, form, "", dev, with_out=True)
    return got


def pack(table):
    """The golden file's form: the distinct answers once, and every row's index."""
    distinct, index, rows_ = [], {}, {}
    for key, a in table.items():
        k = json.dumps(a, sort_keys=True)
        if k not in index:
            index[k] = len(distinct)
            distinct.append(a)
        fam, form, faults = (key.split("/", 2) + [""])[:3]
        rows_.setdefault(fam, {}).setdefault(faults, {})[form] = index[k]
    return {"answers": distinct, "rows": rows_}


def unpack(g):
    want = {}
    for fam, by_fault in g["rows"].items():
        for faults, by_form in by_fault.items():
            for form, k in by_form.items():
                want[f"{fam}/{form}/{faults}" if faults else f"{fam}/{form}"] = g["answers"][k]
    return want
