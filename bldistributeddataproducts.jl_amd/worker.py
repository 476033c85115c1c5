"""Mirror of ``GBT.WorkerFunctions`` (src/gbtworkerfunctions.jl) — the
worker-side read + reduce, with the reduction moved onto the MI355X.

Same names, argument meanings and error behaviour as the reference:

* ``fqav(A, n, f="sum")``  — :16-20 (array) and :27-33 (range);
* ``sanitizeidxs``          — :167-169 (re-exported from .idxs);
* ``getdata(fname, idxs, fqavby=1, fqavfunc="sum")`` — :191-195, plus the
  additive ``tavby`` time integration and its own function ``tavfunc``
  (var / std / median / mad over blocks of spectra included, csrc/tstats.hip);
* ``getfbdata`` / ``getfbh5data`` — :171-177 / :179-189;
* ``getkurtosis``            — :197-202;
* ``getinventory`` / headers — :35-159 (host metadata, see .readers).

``fqavfunc`` is one of ``"sum" | "mean" | "max" | "min"`` (or the Python
builtins ``sum``/``max``/``min``, ``numpy.sum``/``mean``/``max``/``min``), or
the tuple ``("quantile", p)`` (``quantile(p)`` makes it: Statistics.quantile of
every block, Julia's default type 7, by the rule of include/bldp.h; a bad ``p``
is a ValueError before any GPU work), or
the tuple ``("quantiles", (p1, ..., pK))`` (``quantiles(ps)`` makes it: Julia's
vector form, every block read and selected once; the result has K planes on a
new last axis, plane k bit for bit ``("quantile", pk)``'s; as ``tavfunc`` it is
the last stage, as ``fqavfunc`` it takes no ``tavfunc``: TypeError), or
one of the strings ``"var" | "std" | "median" | "mad"``: Julia's ``Statistics``
(the corrected variance, its root, and the median with ``middle(a, b) = a/2 +
b/2`` of an even block) and StatsBase's normalised median absolute deviation
(the median, by the same rule, of ``|x - median(x)|`` with the difference
rounded once, times ``1.4826022185056018`` in Float64; a block holding a NaN,
or more than half one infinity, gives NaN)
on the GPU for Float32 data, without time integration
(``tavby > 1`` is a TypeError); data of other element types get the same
rules on the host in Float64, as Julia's result type is.  Only the strings
select them: ``numpy.std`` is the population form, not Julia's.
The strings ``"argmax" | "argmin"`` give where in each fqavby x tavby block the
extreme lies (Julia's ``argmax`` / ``argmin`` with ``dims``, the position half
of ``findmax``): an int32 array of 0-based offsets ``k + fqavby * tt`` into the
block in Julia's column-major order, the first of the isless-greatest (least)
elements and the first NaN when the block holds one; Float32 data on the GPU
(csrc/argext.hip), other element types by the same rule on the host.
``findmax`` / ``findmin`` return the values and the offsets from one pass.
``numpy.argmax`` is NumPy's rule and stays a host callable.
Any other callable is applied on the host exactly like the reference's
generic ``f(reshape(A, ...); dims=1)`` path (README.md:192-195) — that is the
reference behaviour for functions the GPU does not implement, not a fallback
of the GPU path.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib, engine, readers
from .idxs import COLON, JRange, sanitizeidxs, to_window  # noqa: F401  (re-exports)

__all__ = [
    "fqav", "FRange", "sanitizeidxs", "getdata", "getfbdata", "getfbh5data", "getkurtosis", "getskewness", "getmoments",
    "getinventory", "getfbheader", "getfbh5header", "getheader", "findmax", "findmin",
]


@dataclass(frozen=True)
class FRange:
    """Julia ``range(first; step, length)`` (a StepRangeLen) — the type
    ``fqav(r::AbstractRange, n)`` returns (src/gbtworkerfunctions.jl:32)."""

    first: float
    step: float
    length: int

    def __len__(self):
        return self.length

    @property
    def last(self) -> float:
        return self.first + (self.length - 1) * self.step

    def values(self) -> np.ndarray:
        return self.first + self.step * np.arange(self.length, dtype=np.float64)


def _opname(f):
    """The GPU op of an fqavfunc / tavfunc: a name of _lib.OPS, the tuple
    ``("quantile", p)`` or ``("quantiles", ps)`` (every p checked here:
    ValueError before any GPU work), or None for a host callable."""
    if isinstance(f, str):
        if f not in _lib.OPS:
            raise ValueError(f"fqavfunc {f!r} not one of {sorted(_lib.OPS)} or "
                             f"(\"quantile\", p)")
        return f
    if isinstance(f, tuple):
        ps = _lib.quantiles_of(f)
        if ps is not None:
            return ("quantiles", ps)
        p = _lib.quantile_of(f)
        if p is None:
            raise ValueError(f"fqavfunc {f!r} is not (\"quantile\", p) or (\"quantiles\", ps)")
        return ("quantile", p)
    names = {sum: "sum", max: "max", min: "min", np.sum: "sum", np.mean: "mean",
             np.max: "max", np.min: "min", np.amax: "max", np.amin: "min"}
    return names.get(f)


def _argop(f) -> str | None:
    """"argmax" / "argmin" for those strings (Julia's rule, csrc/argext.hip),
    else None: numpy.argmax and friends stay host callables with NumPy's rule."""
    return f if isinstance(f, str) and f in _lib.ARG_OPS else None


def _is_path(x) -> bool:
    return isinstance(x, (str, bytes)) or hasattr(x, "__fspath__")


def _is_tensor(x) -> bool:
    try:
        import torch
    except ImportError:  # pragma: no cover
        return False
    return isinstance(x, torch.Tensor)


def fqav_range(r, n: int):
    """fqav(r::AbstractRange, n) (src/gbtworkerfunctions.jl:27-33)."""
    if isinstance(r, JRange):
        first, step, length = float(r.first), float(r.step), len(r)
    elif isinstance(r, FRange):
        first, step, length = r.first, r.step, r.length
    else:
        raise TypeError("range expected")
    if n <= 1:  # :28
        return r
    import ctypes

    f, s, l = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    _lib.check(_lib.lib().bldp_fqav_range(first, step, length, int(n), ctypes.byref(f),
                                          ctypes.byref(s), ctypes.byref(l)), "bldp_fqav_range")
    return FRange(f.value, s.value, l.value)


def _host_generic(A: np.ndarray, n: int, f) -> np.ndarray:
    """Reference semantics for an arbitrary Julia-style f(X; dims=1): the
    result is whatever f returns, in f's own element type (fqav returns
    dropdims(f(reshape(A, ...); dims=1); dims=1), src/gbtworkerfunctions.jl:19:
    e.g. median or std of an integer array is Float64)."""
    if A.shape[0] % n:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: fqavby={n} does not divide {A.shape[0]}")
    R = np.asarray(A).reshape((n, A.shape[0] // n) + A.shape[1:], order="F")
    return np.asfortranarray(np.asarray(f(R, axis=0)))


def _host_stat(a: np.ndarray, n: int, op: str, win=None, axis: int = 0) -> np.ndarray:
    """Julia's var / std / median / mad of every n channels (``axis=0``,
    fqavfunc) or every n spectra (``axis=2``, tavfunc) in Float64, for the
    element types the GPU ops do not take (integers, Float64): the corrected
    two-pass variance about the mean, its root, and the median ordered by
    isless (-0.0 < 0.0), the middle element of an odd block, a/2 + b/2 of an
    even one, NaN when the block holds a NaN; mad is that median of
    |x - median(x)| times StatsBase's mad_constant (n <= 1: the block itself).
    ``("quantile", p)``: Statistics.quantile (type 7) by the rule of
    include/bldp.h with every step in Float64 (d a Float64 difference).
    ``("quantiles", ps)``: that per p, the K results on a new last axis."""
    ps = _lib.quantiles_of(op)
    if ps is not None:
        planes = [_host_stat(a, n, ("quantile", p), win, axis) for p in ps]
        return np.asfortranarray(np.stack(planes, axis=-1))
    a = np.asarray(a)
    if win is not None:
        a = a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1])
                       for k in range(3)])]
    n = max(int(n), 1)
    if a.shape[axis] % n:
        raise _lib.DimensionMismatch(
            _lib.BLDP_EDIM, f"DimensionMismatch: {'fqavby' if axis == 0 else 'tavby'}={n} does "
                            f"not divide {a.shape[axis]}")
    # the reduced axis first: blocks of n along it, whatever axis it was
    m = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    R = np.asfortranarray(m).reshape((n, m.shape[0] // n) + m.shape[1:], order="F")

    def median(R):
        bits = R.view(np.int64)
        key = np.where(bits < 0, bits ^ np.int64(0x7FFFFFFFFFFFFFFF), bits)  # isless order
        S = np.take_along_axis(R, np.argsort(key, axis=0, kind="stable"), axis=0)
        r = S[n // 2] if n % 2 else S[n // 2 - 1] / 2 + S[n // 2] / 2
        return np.where(np.isnan(R).any(axis=0), np.nan, r)

    def quantile(R, p):
        j, g = _lib.quantile_rank(n, p)
        bits = R.view(np.int64)
        key = np.where(bits < 0, bits ^ np.int64(0x7FFFFFFFFFFFFFFF), bits)  # isless order
        S = np.take_along_axis(R, np.argsort(key, axis=0, kind="stable"), axis=0)
        lo, hi = S[j - 1], S[j]
        fin = np.isfinite(lo) & np.isfinite(hi)
        r = np.where(fin, lo + g * (hi - lo), (1.0 - g) * lo + g * hi)
        return np.where(np.isnan(R).any(axis=0), np.nan, r)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if _lib.quantile_of(op) is not None and n > 1:
            r = quantile(R, op[1])
        elif _lib.quantile_of(op) is not None:
            r = R[0]
        elif op == "var":
            r = np.var(R, axis=0, ddof=1)
        elif op == "std":
            r = np.std(R, axis=0, ddof=1)
        elif op == "mad" and n > 1:
            # the median (NaN wins again: Inf - Inf) of |x - median(x)|, normalised
            r = median(np.abs(R - median(R)[None])) * _lib.MAD_CONSTANT
        else:
            r = median(R)
    return np.asfortranarray(np.moveaxis(r, 0, axis))


def _host_argext(a: np.ndarray, fqavby, tavby, op: str, win=None, values=False):
    """Julia's argmax / argmin of every fqavby x tavby block for the element
    types the GPU op does not take (integers, Float64): the int32 offset
    ``k + fqavby * tt`` of the winner in its block (column-major), the first of
    the isless-greatest (least) elements (-0.0 < 0.0), and the first NaN when
    the block holds one; with ``values`` also the winning elements."""
    a = np.asarray(a)
    if win is not None:
        a = a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1])
                       for k in range(3)])]
    F, T = max(int(fqavby), 1), max(int(tavby), 1)
    nc, ni, nt = a.shape
    if nc % F:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: fqavby={F} does not divide nchan={nc}")
    if nt % T:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: tavby={T} does not divide ntime={nt}")
    if F * T > 2 ** 31 - 1:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL, f"blocks of {F} x {T} are beyond 2^31 - 1")
    # (F*T, nco, ni, nto): a block along axis 0 in Julia's order, channel fastest
    R = np.asfortranarray(a).reshape((F, nc // F, ni, T, nt // T), order="F")
    B = np.asfortranarray(np.moveaxis(R, 3, 1)).reshape((F * T, nc // F, ni, nt // T), order="F")
    if B.dtype.kind == "f":
        ut = {4: np.uint32, 8: np.uint64}[B.dtype.itemsize]
        top = ut(1) << ut(8 * B.dtype.itemsize - 1)
        u = B.view(ut)
        key = np.where(u & top != 0, ~u, u | top)  # isless order as unsigned order
        if op == "argmin":
            key = ~key
        key = np.where(np.isnan(B), ut(np.iinfo(ut).max), key)  # any NaN wins
        idx = np.argmax(key, axis=0)  # (first occurrence)
    else:
        idx = np.argmax(B, axis=0) if op == "argmax" else np.argmin(B, axis=0)
    val = np.take_along_axis(B, idx[None], axis=0)[0] if values else None
    idx = np.asfortranarray(idx.astype(np.int32))
    return (idx, np.asfortranarray(val)) if values else idx


def _argext_array(x, idxs, fqavby, tavby, aop, device, values=False):
    """argmax / argmin of an in-memory filterbank: a device tensor stays on the
    device, a Float32 host array goes through the GPU, other element types get
    the same rule on the host."""
    idxs = sanitizeidxs(idxs)
    if _is_tensor(x):
        return engine.argext(x, fqavby, tavby, aop, to_window(idxs, x.shape), values=values)
    a = np.asarray(x)
    if a.ndim != 3:
        raise ValueError("filterbank arrays are 3-D (nchan, nif, ntime)")
    win = to_window(idxs, a.shape)
    if a.dtype == np.float32:
        return engine.argext_host(np.asfortranarray(a), fqavby, tavby, aop, win, values=values,
                                  device=device)
    if engine._dtype_code(a.dtype) is None:
        raise TypeError(f"element type {a.dtype} is not supported")
    engine._check_bounds(win, a.shape)
    return _host_argext(a, fqavby, tavby, aop, win, values=values)


def _argext_file(fname, idxs, fqavby, tavby, aop, device, values=False):
    """argmax / argmin of a file's window: read onto the GPU the way getdata
    reads it (window_on_device) and reduced there; only the offsets (and the
    values) come back."""
    got = window_on_device(fname, idxs, device)
    if got is not None:
        import torch

        x, rwin = got
        with torch.cuda.device(x.device):
            r = engine.argext(x, fqavby, tavby, aop, rwin, values=values)
            return tuple(engine.fb_to_numpy(t) for t in r) if values else engine.fb_to_numpy(r)
    # not Float32, or an empty window: the host-array path
    if readers.ishdf5(fname):
        return _argext_array(readers.fbh5_read(fname, idxs), (COLON, COLON, COLON), fqavby, tavby,
                             aop, device, values)
    _, data = readers.fil_mmap(fname)
    try:
        return _argext_array(data, idxs, fqavby, tavby, aop, device, values)
    finally:
        del data


def _findext(src, idxs, fqavby, tavby, device, aop):
    assert len(idxs) == 3, "idxs must have exactly three indices"
    if _is_path(src):
        idx, val = _argext_file(src, sanitizeidxs(idxs), fqavby, tavby, aop, device, values=True)
    else:
        idx, val = _argext_array(src, idxs, fqavby, tavby, aop, device, values=True)
    return val, idx


def findmax(x_or_fname, idxs=(COLON, COLON, COLON), fqavby=1, tavby=1, device=0):
    """Julia's ``findmax`` over every fqavby x tavby block of the window, in
    one pass: ``(values, idx)`` with ``idx`` as ``fqavfunc="argmax"`` gives it
    (int32, 0-based ``k + fqavby * tt``) and ``values`` the elements there (a
    NaN where the block holds one).  A file or host array gives host arrays, a
    device tensor device tensors."""
    return _findext(x_or_fname, idxs, fqavby, tavby, device, "argmax")


def findmin(x_or_fname, idxs=(COLON, COLON, COLON), fqavby=1, tavby=1, device=0):
    """``findmax``'s counterpart for the isless-least element (``"argmin"``)."""
    return _findext(x_or_fname, idxs, fqavby, tavby, device, "argmin")


def fqav(A, n: int, f="sum"):
    """Reduce every ``n`` elements of the first dimension of ``A`` with ``f``
    (src/gbtworkerfunctions.jl:16-20).  ``n <= 1`` returns ``A`` itself (:17).
    Device tensors stay on the device; host arrays go through the GPU and
    come back as host arrays."""
    if isinstance(A, (JRange, FRange)):
        return fqav_range(A, n)
    if n <= 1:
        ps = _lib.quantiles_of(f) if isinstance(f, tuple) else None
        return A if ps is None else _planes(A, len(ps))
    aop = _argop(f)
    if aop is not None:  # where in each block of n the extreme lies (int32 offsets)
        if _is_tensor(A):
            return engine.argext(A, n, 1, aop)
        A = np.asarray(A)
        if A.ndim > 3:
            raise ValueError("fqav arrays are at most 3-D (nchan, nif, ntime)")
        a3 = A.reshape(A.shape + (1,) * (3 - A.ndim), order="F")
        out = _argext_array(a3, (COLON, COLON, COLON), n, 1, aop, 0)
        return out.reshape((out.shape[0],) + A.shape[1:], order="F")
    op = _opname(f)
    if _is_tensor(A):
        if op is None:
            raise TypeError("only sum/mean/max/min/var/std/median/mad and (\"quantile\", p) run "
                            "on device tensors")
        return engine.reduce(A, n, 1, op)
    A = np.asarray(A)
    if op is None:
        return _host_generic(A, n, f)
    a3 = A.reshape(A.shape + (1,) * (3 - A.ndim), order="F") if A.ndim < 3 else A
    if a3.ndim != 3:
        raise ValueError("fqav arrays are at most 3-D (nchan, nif, ntime)")
    out = _reduce_host(a3, n, 1, op, None, 0)
    # (quantiles: the planes' axis stays last)
    return out.reshape((out.shape[0],) + A.shape[1:] + out.shape[3:], order="F")


def _planes(A, K: int):
    """fqav's n <= 1 rule for quantiles(ps): the array itself in each of K planes
    on a new last axis, in its own element type, plane after plane."""
    if _is_tensor(A):
        import torch

        r = torch.empty((K,) + tuple(reversed(A.shape)), dtype=A.dtype, device=A.device)
        r = r.permute(*reversed(range(r.dim())))
        r.copy_(A.unsqueeze(-1).expand(r.shape))
        return r
    return np.asfortranarray(np.stack([np.asarray(A)] * K, axis=-1))


def _reduce_host(a, fqavby, tavby, op, win, device):
    """A host array through the GPU with fqav's Julia result type: Float32
    stays Float32; integer and Float64 arrays take the typed kernels (sum
    widened to (U)Int64, mean Float64, max / min the input type,
    src/gbtworkerfunctions.jl:19).  Nothing is converted on the way.
    var / std / median of those arrays are Float64 from the host (_host_stat)."""
    engine._check_stat(op, tavby)
    if a.dtype == np.float32:
        return engine.reduce_host(np.asfortranarray(a), fqavby, tavby, op, win, device=device)
    if engine._dtype_code(a.dtype) is None:
        raise TypeError(f"fqav: element type {a.dtype} is not supported (Float32, Float64, "
                        f"8- to 64-bit integers)")
    if _lib.stat_op(op):
        return _host_stat(a, fqavby, op, win)
    return engine.reduce_host_typed(a, fqavby, tavby, op, win, device=device)


def _check_argop(fqavfunc, tavfunc):
    """fqavfunc's arg op, or None; an arg op's result is an index, which no
    tavfunc can integrate (TypeError, as Julia's MethodError)."""
    aop = _argop(fqavfunc)
    if aop is not None and tavfunc is not None:
        raise TypeError(f"fqavfunc {aop!r} gives block offsets: it takes tavby, not a tavfunc")
    # quantiles(ps) gives K planes, which no second stage takes: it is the last stage
    if tavfunc is not None and isinstance(fqavfunc, tuple) and \
            _lib.quantiles_of(fqavfunc) is not None:
        raise TypeError("fqavfunc quantiles(ps) gives a plane per p: it takes no tavfunc (as "
                        "tavfunc it is the last stage, after any fqavfunc)")
    return aop


def _reduce_array(x, idxs, fqavby, fqavfunc, tavby, device, tavfunc=None):
    aop = _check_argop(fqavfunc, tavfunc)
    if aop is not None:
        if fqavby <= 1 and tavby <= 1:  # fqav(A, n <= 1) returns A whatever f is (:17)
            return _reduce_array(x, idxs, 1, "sum", 1, device)
        return _argext_array(x, idxs, fqavby, tavby, aop, device)
    if tavfunc is not None:
        return _tav_array(x, idxs, fqavby, fqavfunc, tavby, tavfunc, device)
    idxs = sanitizeidxs(idxs)
    win = to_window(idxs, x.shape)
    op = _opname(fqavfunc)
    if op is None:
        if tavby > 1:
            raise TypeError("tavby needs fqavfunc in sum/mean/max/min")
        a = np.asarray(x)
        if win is not None:
            ax = [win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1]) for k in range(3)]
            a = a[np.ix_(*ax)]
        return fqav(a, fqavby, fqavfunc)
    if _is_tensor(x):
        return engine.reduce(x, fqavby, tavby, op, win)
    a = np.asarray(x)
    if a.dtype != np.float32 and fqavby <= 1 and tavby <= 1:
        # fqav(A, n <= 1) returns A (:17): the window itself, in its own type
        if engine._dtype_code(a.dtype) is None:
            raise TypeError(f"element type {a.dtype} is not supported")
        engine._check_bounds(win, a.shape)
        if win is not None:
            ax = [win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1]) for k in range(3)]
            a = np.asfortranarray(a[np.ix_(*ax)])
        ps = _lib.quantiles_of(op)
        return a if ps is None else _planes(a, len(ps))
    return _reduce_host(a, fqavby, tavby, op, win, device)


def _tav_ops(fqavby, fqavfunc, tavfunc):
    """The two ops of getdata(...; tavfunc): R = tav(fqav(A, fqavby; f=fqavfunc),
    tavby; f=tavfunc), tav being fqav's rule on axis 3."""
    op2 = _opname(tavfunc) if isinstance(tavfunc, (str, tuple)) or callable(tavfunc) else None
    if op2 is None:
        raise TypeError(f"tavfunc {tavfunc!r} is not one of {sorted(_lib.OPS)} or "
                        f"(\"quantile\", p)")
    op1 = _opname(fqavfunc)
    if op1 is None and fqavby > 1:
        raise TypeError("tavfunc needs fqavfunc in sum/mean/max/min/var/std/median/mad or "
                        "(\"quantile\", p)")
    return op1 or "sum", op2


def _tav_device(x, win, fqavby, op1, tavby, op2, out=None):
    """Both stages on a device tensor, the window staying on the GPU: stage 1
    is the reduce with tavby = 1 (skipped for fqavby <= 1, its result a
    temporary device tensor), stage 2 the reduce with fqavby = 1 for
    sum / mean / max / min and engine.tstat for var / std / median (skipped
    for tavby <= 1: fqav's n <= 1 rule; quantiles(ps) then copies stage 1's
    result into its planes)."""
    if tavby <= 1 and _lib.quantiles_of(op2) is None:
        return engine.reduce(x, fqavby, 1, op1 if fqavby > 1 else "sum", win, out=out)
    if fqavby > 1:
        x, win = engine.reduce(x, fqavby, 1, op1, win), None
    if _lib.stat_op(op2):
        return engine.tstat(x, tavby, op2, win, out=out)
    return engine.reduce(x, 1, tavby, op2, win, out=out)


def _tav_host(a, win, fqavby, op1, tavby, op2, device):
    """Both stages for a host array of an element type the GPU statistics do
    not take: var / std / median on the host in Float64 (_host_stat, Julia's
    result type), sum / mean / max / min through the typed GPU reduce."""
    if engine._dtype_code(a.dtype) is None:
        raise TypeError(f"element type {a.dtype} is not supported")
    engine._check_bounds(win, a.shape)
    engine.out_shape(a.shape, win, fqavby, tavby)  # DimensionMismatch before any work
    if fqavby > 1:
        a = _reduce_host(a, fqavby, 1, op1, win, device)
    elif win is not None:
        a = np.asfortranarray(a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1])
                                         for k in range(3)])])
    if tavby <= 1:
        ps = _lib.quantiles_of(op2)
        return a if ps is None else _planes(a, len(ps))
    if _lib.stat_op(op2):
        return _host_stat(a, tavby, op2, axis=2)
    return _reduce_host(np.asfortranarray(a), 1, tavby, op2, None, device)


def _tav_array(x, idxs, fqavby, fqavfunc, tavby, tavfunc, device):
    """getdata(...; tavfunc) of an in-memory filterbank (host array: result on
    the host; device tensor: result on the device)."""
    op1, op2 = _tav_ops(fqavby, fqavfunc, tavfunc)
    idxs = sanitizeidxs(idxs)
    if _is_tensor(x):
        return _tav_device(x, to_window(idxs, x.shape), fqavby, op1, tavby, op2)
    a = np.asarray(x)
    if a.ndim != 3:
        raise ValueError("filterbank arrays are 3-D (nchan, nif, ntime)")
    win = to_window(idxs, a.shape)
    if a.dtype != np.float32:
        return _tav_host(a, win, fqavby, op1, tavby, op2, device)
    engine._check_bounds(win, a.shape)
    dims = engine.out_shape(a.shape, win, fqavby, tavby)
    if 0 in dims:
        return np.empty(dims, dtype=np.float32, order="F")
    import torch

    xd = engine.fb_from_numpy(a, device=f"cuda:{int(device)}")
    with torch.cuda.device(xd.device):
        return engine.fb_to_numpy(_tav_device(xd, win, fqavby, op1, tavby, op2))


def _tav_file(fname, idxs, fqavby, fqavfunc, tavby, tavfunc, device):
    """getdata(...; tavfunc) of a file: the window is read onto the GPU the way
    getdata reads it (window_on_device: raw preads, chunks decoded on the GPU,
    else libhdf5 / mmap and one copy) and stays there between the two stages."""
    op1, op2 = _tav_ops(fqavby, fqavfunc, tavfunc)
    got = window_on_device(fname, idxs, device)
    if got is not None:
        import torch

        x, rwin = got
        with torch.cuda.device(x.device):
            return engine.fb_to_numpy(_tav_device(x, rwin, fqavby, op1, tavby, op2))
    # not Float32, or an empty window: the host-array path
    if readers.ishdf5(fname):
        return _tav_array(readers.fbh5_read(fname, idxs), (COLON, COLON, COLON), fqavby, fqavfunc,
                          tavby, tavfunc, device)
    _, data = readers.fil_mmap(fname)
    try:
        return _tav_array(data, idxs, fqavby, fqavfunc, tavby, tavfunc, device)
    finally:
        del data


def _raw_to_device(fname, raw, idxs, device):
    """The window of a raw (filter-free, contiguous float32) file on GPU
    ``device``: (Julia-order block tensor, window relative to it), or None for
    an empty window (the host path returns the empty result)."""
    from . import filestream

    base, jshape = raw
    win = to_window(idxs, jshape) or [0, jshape[0], 1, 0, jshape[1], 1, 0, jshape[2], 1]
    if win[1] * win[4] * win[7] == 0:
        filestream.plan_window(jshape, win)  # bounds check only
        return None
    x, _, rwin = filestream.window_to_device(fname, base, jshape, win, f"cuda:{int(device)}")
    return x, rwin


def _reduce_raw_file(fname, raw, idxs, fqavby, op, tavby, device):
    import torch

    got = _raw_to_device(fname, raw, idxs, device)
    if got is None:
        return None
    x, rwin = got
    with torch.cuda.device(x.device):
        return engine.fb_to_numpy(engine.reduce(x, fqavby, tavby, op, rwin))


def getfbdata(fbname, idxs=(COLON, COLON, COLON), fqavby=1, fqavfunc="sum", tavby=1,
              device=0, tavfunc=None):
    """SIGPROC filterbank: mmap, window, reduce (src/gbtworkerfunctions.jl:171-177).
    32-bit data with a GPU reduction: only the window's rows / channel spans
    are read (parallel preads into pinned memory, streamed to the GPU).
    ``tavfunc``: as getdata."""
    assert len(idxs) == 3, "idxs must have exactly three indices"  # :172
    idxs = sanitizeidxs(idxs)
    aop = _check_argop(fqavfunc, tavfunc)
    if aop is not None:
        if fqavby <= 1 and tavby <= 1:  # fqav(A, n <= 1) returns A whatever f is (:17)
            fqavfunc = "sum"
        else:
            return _argext_file(fbname, idxs, fqavby, tavby, aop, device)
    if tavfunc is not None:
        return _tav_file(fbname, idxs, fqavby, fqavfunc, tavby, tavfunc, device)
    op = _opname(fqavfunc)
    if op is not None:
        raw = readers.fil_raw_layout(fbname)
        if raw is not None:
            r = _reduce_raw_file(fbname, raw, idxs, fqavby, op, tavby, device)
            if r is not None:
                return r
    _, data = readers.fil_mmap(fbname)
    try:
        return _reduce_array(data, idxs, fqavby, fqavfunc, tavby, device)
    finally:
        del data  # finalize(parent(dmmap)) (:175)


def getfbh5data(fbh5name, idxs=(COLON, COLON, COLON), fqavby=1, fqavfunc="sum", tavby=1,
                device=0, tavfunc=None):
    """FBH5: read the window (whole dataset for (:,:,:)), then reduce
    (src/gbtworkerfunctions.jl:179-189).  ``tavfunc``: as getdata."""
    assert len(idxs) == 3, "idxs must have exactly three indices"  # :180
    idxs = sanitizeidxs(idxs)
    aop = _check_argop(fqavfunc, tavfunc)
    if aop is not None:
        if fqavby <= 1 and tavby <= 1:  # fqav(A, n <= 1) returns A whatever f is (:17)
            fqavfunc = "sum"
        else:
            return _argext_file(fbh5name, idxs, fqavby, tavby, aop, device)
    if tavfunc is not None:
        return _tav_file(fbh5name, idxs, fqavby, fqavfunc, tavby, tavfunc, device)
    op = _opname(fqavfunc)
    from . import fbh5

    if op is not None and (fbh5.needs_bslz4(fbh5name) or fbh5.raw_chunked(fbh5name)):
        # compressed rawspec product: only the compressed chunks cross PCIe; they
        # are decoded, windowed and reduced on the GPU, the result comes back.
        # Unfiltered chunked data takes the same chunk reader without a decode.
        # (the decoded chunk grid plus the window inside it when the chunks
        # span the window's channels: no gather copy)
        x, rwin = fbh5._read_window_bslz4_dev(fbh5name, idxs, f"cuda:{device}",
                                              raw_chunks=not fbh5.needs_bslz4(fbh5name),
                                              dense=False)
        import torch

        with torch.cuda.device(x.device):
            return engine.fb_to_numpy(engine.reduce(x, fqavby, tavby, op, rwin))
    if op is not None:
        raw = fbh5.raw_layout(fbh5name)  # uncompressed contiguous: preads, no libhdf5 copy
        if raw is not None:
            r = _reduce_raw_file(fbh5name, raw, idxs, fqavby, op, tavby, device)
            if r is not None:
                return r
    data = readers.fbh5_read(fbh5name, idxs)
    return _reduce_array(data, (COLON, COLON, COLON), fqavby, fqavfunc, tavby, device)


def window_on_device(fname, idxs, device=0):
    """The Float32 window of a file (or host / device array) on GPU
    ``device`` as (tensor, window relative to it), reading it the way
    getfbh5data / getfbdata do (compressed chunks decoded on the GPU, raw
    data block preads, else libhdf5 / mmap then one H2D copy); None when the
    data are not Float32 (those keep their own types through the host-array
    path) or the window is empty."""
    import torch

    idxs = sanitizeidxs(idxs)
    dev = f"cuda:{int(device)}"
    if _is_tensor(fname):
        if fname.dtype != torch.float32:
            return None
        return fname, to_window(idxs, fname.shape)
    if isinstance(fname, (str, bytes)) or hasattr(fname, "__fspath__"):
        from . import fbh5

        h5 = readers.ishdf5(fname)
        if h5 and (fbh5.needs_bslz4(fname) or fbh5.raw_chunked(fname)):
            return fbh5._read_window_bslz4_dev(fname, idxs, dev,
                                               raw_chunks=not fbh5.needs_bslz4(fname), dense=False)
        raw = fbh5.raw_layout(fname) if h5 else readers.fil_raw_layout(fname)
        if raw is not None:
            return _raw_to_device(fname, raw, idxs, device)
        if h5:
            a, win = readers.fbh5_read(fname, idxs), None
        else:
            _, a = readers.fil_mmap(fname)
            win = to_window(idxs, a.shape)
    else:
        a = fname
        win = to_window(idxs, np.asarray(a).shape)
    a = np.asarray(a)
    if a.dtype != np.float32:
        return None
    if win is not None:
        a = np.asfortranarray(a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1])
                                         for k in range(3)])])
    if a.size == 0:
        return None
    return engine.fb_from_numpy(a, device=dev), None


def getdata_device(fname, idxs=(COLON, COLON, COLON), fqavby=1, fqavfunc="sum", tavby=1,
                   device=0, out=None, tavfunc=None):
    """getdata with the result left on GPU ``device`` (a Julia-order Float32
    tensor; quantiles(ps): the 4-D plane tensor), written into ``out`` when given — e.g. a bank's slot of a stitched
    band product (GBT.getband); None when the data are not Float32.  With
    ``tavfunc`` (as getdata) the last stage writes ``out``."""
    if _check_argop(fqavfunc, tavfunc) is not None:
        raise TypeError("the device path writes Float32 products: argmax / argmin go through "
                        "getdata or engine.argext")
    if tavfunc is not None:
        op1, op2 = _tav_ops(fqavby, fqavfunc, tavfunc)
        got = window_on_device(fname, idxs, device)
        if got is None:
            return None
        import torch

        with torch.cuda.device(got[0].device):
            return _tav_device(got[0], got[1], fqavby, op1, tavby, op2, out=out)
    op = _opname(fqavfunc)
    if op is None:
        raise TypeError("the device path takes fqavfunc in sum/mean/max/min/var/std/median/mad or "
                        "(\"quantile\", p)")
    got = window_on_device(fname, idxs, device)
    if got is None:
        return None
    x, rwin = got
    import torch

    with torch.cuda.device(x.device):
        return engine.reduce(x, fqavby, tavby, op, rwin, out=out)


def getdata(fname, idxs=(COLON, COLON, COLON), fqavby=1, fqavfunc="sum", tavby=1, device=0,
            tavfunc=None):
    """WorkerFunctions.getdata (src/gbtworkerfunctions.jl:191-195).

    ``fname`` may also be an in-memory filterbank: a Fortran-ordered
    (nchan, nif, ntime) float32 array (result on the host) or a Julia-order
    device tensor (result stays on the device).

    ``tavfunc=None`` (default): ``fqavfunc`` reduces the fqavby x tavby block,
    as ever.  ``tavfunc`` given (a name of ``fqavfunc``'s, var / std / median /
    mad included): the time integration takes its own function, fqav's rule on
    axis 3: ``R = tav(fqav(A, fqavby; f=fqavfunc), tavby; f=tavfunc)`` with
    ``R[c, i, b] = tavfunc(B[c, i, b*tavby : (b+1)*tavby])``.  Either stage is
    skipped when its factor is <= 1; tavby must divide the selected spectra
    (DimensionMismatch).  Float32 data stay on the GPU between the stages;
    var / std / median / mad of other element types are Float64 from the host.

    ``fqavfunc="argmax" | "argmin"``: an int32 array of each block's winner's
    0-based offset ``k + fqavby * tt`` (module docstring); no ``tavfunc``."""
    _check_argop(fqavfunc, tavfunc)  # (the TypeError before any file is touched)
    if not isinstance(fname, (str, bytes)) and not hasattr(fname, "__fspath__"):
        return _reduce_array(fname, idxs, fqavby, fqavfunc, tavby, device, tavfunc)
    idxs = sanitizeidxs(idxs)  # :192
    if readers.ishdf5(fname):  # :193
        return getfbh5data(fname, idxs, fqavby, fqavfunc, tavby, device, tavfunc)
    return getfbdata(fname, idxs, fqavby, fqavfunc, tavby, device, tavfunc)


def getkurtosis(fname, idxs=(COLON, COLON, COLON), device=0, tblock=None):
    """Excess kurtosis of every (channel, IF) row over time, Float64 (nc, ni)
    (src/gbtworkerfunctions.jl:197-202).  With ``tblock=M`` the selected
    spectra are cut into blocks of M and the result is the (nc, ni, nt/M)
    kurtosis of every block (M must divide nt: DimensionMismatch)."""
    idxs = sanitizeidxs(idxs)
    if _is_tensor(fname):
        return engine.kurtosis(fname, to_window(idxs, fname.shape), tblock=tblock)
    if isinstance(fname, (str, bytes)) or hasattr(fname, "__fspath__"):
        from . import fbh5

        h5 = readers.ishdf5(fname)
        if h5 and (fbh5.needs_bslz4(fname) or fbh5.raw_chunked(fname)):
            # compressed / chunked: the chunks go to the GPU, are decoded there
            # and the kurtosis runs on the window inside the chunk grid
            import torch

            x, rwin = fbh5._read_window_bslz4_dev(fname, idxs, f"cuda:{device}",
                                                  raw_chunks=not fbh5.needs_bslz4(fname),
                                                  dense=False)
            with torch.cuda.device(x.device):
                return engine.fb_to_numpy(engine.kurtosis(x, rwin, tblock=tblock))
        raw = fbh5.raw_layout(fname) if h5 else readers.fil_raw_layout(fname)
        got = _raw_to_device(fname, raw, idxs, device) if raw is not None else None
        if got is not None:  # window streamed to the GPU, kurtosis there
            import torch

            x, rwin = got
            with torch.cuda.device(x.device):
                return engine.fb_to_numpy(engine.kurtosis(x, rwin, tblock=tblock))
        if h5:
            a, idxs = readers.fbh5_read(fname, idxs), (COLON, COLON, COLON)
        else:
            _, a = readers.fil_mmap(fname)
    else:
        a = fname
    a = np.asarray(a)
    win = to_window(idxs, a.shape)
    if a.dtype != np.float32:  # StatsBase in Float64 for integer / Float64 rows (:200)
        if engine._dtype_code(a.dtype) is None:
            raise TypeError(f"getkurtosis: element type {a.dtype} is not supported")
        return engine.kurtosis_host_typed(a, win, device=device, tblock=tblock)
    return engine.kurtosis_host(np.asfortranarray(a), win, device=device, tblock=tblock)


def _read_moment(name, takes, fname, idxs, device, on_device, on_host, to_host):
    """The reader of getskewness and getmoments: a device tensor goes to
    ``on_device(x, win)``; a file reaches the GPU as getdata reads it
    (window_on_device) and its result comes back through ``to_host``; a host
    array, or a file window_on_device leaves alone, goes to ``on_host(a, win)``.
    Float32 only: ``name`` and ``takes`` word the TypeError.  ``idxs``: sanitized."""
    if _is_tensor(fname):
        return on_device(fname, to_window(idxs, fname.shape))
    if isinstance(fname, (str, bytes)) or hasattr(fname, "__fspath__"):
        got = window_on_device(fname, idxs, device)
        if got is not None:
            import torch

            x, rwin = got
            with torch.cuda.device(x.device):
                return to_host(on_device(x, rwin))
        # not Float32, or an empty window: the host array tells which
        if readers.ishdf5(fname):
            a, idxs = readers.fbh5_read(fname, idxs), (COLON, COLON, COLON)
        else:
            _, a = readers.fil_mmap(fname)
    else:
        a = fname
    a = np.asarray(a)
    if a.dtype != np.float32:
        engine._need_f32(name, a.dtype, takes)
    return on_host(np.asfortranarray(a), to_window(idxs, a.shape))


def getskewness(fname, idxs=(COLON, COLON, COLON), device=0, tblock=None):
    """Skewness of every (channel, IF) row over time, Float64 (nc, ni): what
    ``map(skewness, eachrow(...))`` in place of src/gbtworkerfunctions.jl:200
    gives (StatsBase.skewness with Julia's Float32 mean).  With ``tblock=M``
    the (nc, ni, nt/M) skewness of every block of M selected spectra (M must
    divide nt: DimensionMismatch).  Files reach the GPU as getdata reads them
    (window_on_device).  Float32 data only: any other element type (host
    array, device tensor, 8/16-bit SIGPROC file) is a TypeError."""
    return _read_moment(
        "getskewness", "skewness", fname, sanitizeidxs(idxs), device,
        lambda x, win: engine.skewness(x, win, tblock=tblock),
        lambda a, win: engine.skewness_host(a, win, device=device, tblock=tblock),
        engine.fb_to_numpy)


def getmoments(fname, idxs=(COLON, COLON, COLON), device=0, tblock=None, which=engine.MOMENTS):
    """Mean, variance, skewness and kurtosis of every (channel, IF) row over
    time from ONE read of the data: an ``engine.Moments`` named tuple of
    Float64 (nc, ni) arrays, or (nc, ni, nt/M) with ``tblock=M`` (M must divide
    nt: DimensionMismatch).  ``skewness`` and ``kurtosis`` are what getskewness
    and getkurtosis give, ``mean`` is Julia's Float32 mean widened and ``var``
    is cm2 / n, the UNCORRECTED variance those two divide by (not Julia's
    ``var``, which divides by n - 1).  A plane not named in ``which`` is
    ``None``.  Files reach the GPU as getdata reads them (window_on_device),
    once.  Float32 data only: any other element type (host array, device
    tensor, 8/16-bit SIGPROC file) is a TypeError."""
    idxs = sanitizeidxs(idxs)
    engine._which_planes(which)  # (the ValueError before any file is touched)
    return _read_moment(
        "getmoments", "moments", fname, idxs, device,
        lambda x, win: engine.moments(x, win, tblock=tblock, which=which),
        lambda a, win: engine.moments_host(a, win, device=device, tblock=tblock, which=which),
        lambda m: engine.Moments(*[None if t is None else engine.fb_to_numpy(t) for t in m]))


def getoutliers(src, idxs=(COLON, COLON, COLON), *, n=None, axis=2, nsigma=5.0, mask=False,
                device=0):
    """Robust outlier flagging of every block of ``n`` selected channels
    (``axis=0``) or spectra (``axis=2``; ``n=None``: the whole selected time
    range) from ONE read of the data: a dict with ``"median"`` and ``"mad"``
    (Float32, what the ``"median"`` and ``"mad"`` statistics give bit for bit),
    ``"count"`` (int32), the samples of each block with ``|x - median| >
    Float32(nsigma * mad)`` (strictly; a NaN median or mad flags nothing), each
    (nc/n, ni, nt) or (nc, ni, nt/n), and with ``mask=True`` ``"mask"``, the uint8
    (nc, ni, nt) flags of the window (engine.outliers; the rule of include/bldp.h).
    Files reach the GPU as getdata reads them (window_on_device) and a host array
    is staged there, both returning host arrays; a device tensor stays on the
    device.  Float32 data only: any other element type (host array, device
    tensor, 8/16-bit SIGPROC file) is a TypeError."""
    engine._outliers_args(axis, nsigma, ())  # (the ValueError before any file is touched)
    kw = dict(n=n, axis=axis, nsigma=nsigma, mask=mask)
    return _read_moment(
        "getoutliers", "outliers", src, sanitizeidxs(idxs), device,
        lambda x, win: engine.outliers(x, win=win, **kw),
        lambda a, win: engine.outliers_host(a, win=win, device=device, **kw),
        lambda r: {k: engine.fb_to_numpy(t) for k, t in r.items()})


def getmasked(src, idxs=(COLON, COLON, COLON), *, mask, fqavby=1, tavby=1, func="sum", device=0):
    """The window integrated over its unflagged samples: a dict with ``"data"``,
    the ``func`` (``"sum"`` or ``"mean"``) of the samples of every fqavby x tavby
    block whose byte of ``mask`` is 0, and ``"kept"`` (int32), how many there
    were: the weight of each product (engine.masked_reduce; the rule of
    include/bldp.h).  ``mask`` has the window's shape (nc, ni, nt), any axis of
    which may be 1 (a bad-channel list is (nc, 1, 1)); uint8 or bool, a host array
    or a device tensor (it goes to where the data is).  Files reach the GPU as
    getdata reads them (window_on_device) and a host array is staged there, both
    returning host arrays; a device tensor stays on the device.  Float32 data
    only: any other element type (host array, device tensor, 8/16-bit SIGPROC
    file) is a TypeError."""
    engine._masked_op(func)  # (the ValueError before any file is touched)
    if _is_tensor(mask):
        mdt, host_mask = str(mask.dtype).replace("torch.", ""), None
    else:
        host_mask = np.asarray(mask)
        mdt = str(host_mask.dtype)
    if mdt not in ("uint8", "bool"):
        raise TypeError(f"getmasked: the mask must be uint8 or bool, not {mdt}")
    kw = dict(fqavby=fqavby, tavby=tavby, op=func)

    def on_device(x, win):
        m = mask
        if host_mask is not None:
            import torch

            m = torch.from_numpy(np.ascontiguousarray(host_mask.view(np.uint8)))
        return engine.masked_reduce(x, m.to(x.device), win=win, **kw)

    def on_host(a, win):
        m = host_mask if host_mask is not None else mask.cpu().numpy()
        return engine.masked_reduce_host(a, m, win=win, device=device, **kw)

    return _read_moment("getmasked", "masked_reduce", src, sanitizeidxs(idxs), device, on_device,
                        on_host, lambda r: {k: engine.fb_to_numpy(t) for k, t in r.items()})


def getclean(src, idxs=(COLON, COLON, COLON), *, fqavby=1, tavby=1, n=None, axis=2, nsigma=5.0,
             func="sum", device=0):
    """Flag and integrate on the device, with no host trip between the two:
    engine.outliers flags every block of ``n`` selected channels (``axis=0``) or
    spectra (``axis=2``; ``n=None``: the whole selected time range) at ``nsigma``
    scaled mads from its median, and engine.masked_reduce takes the ``func``
    (``"sum"`` or ``"mean"``) of every fqavby x tavby block over the samples left.
    A dict with ``"data"``, ``"kept"`` (int32, the weight of each product) and
    ``"count"`` (int32), the flags of every block of ``outliers``.  The mask never
    leaves the device.  Files, host arrays and device tensors as getmasked takes
    them; Float32 data only."""
    engine._outliers_args(axis, nsigma, ("count",))  # (ValueErrors before any file is touched)
    engine._masked_op(func)

    def on_device(x, win):
        o = engine.outliers(x, n=n, axis=axis, nsigma=nsigma, win=win, mask=True,
                            which=("count",))
        r = engine.masked_reduce(x, o["mask"], fqavby=fqavby, tavby=tavby, op=func, win=win)
        r["count"] = o["count"]
        return r

    def on_host(a, win):  # staged whole, so that both halves read one device tensor
        import torch

        dev = f"cuda:{device}"
        with torch.cuda.device(dev):
            return {k: engine.fb_to_numpy(t)
                    for k, t in on_device(engine.fb_from_numpy(a, device=dev), win).items()}

    return _read_moment("getclean", "getclean", src, sanitizeidxs(idxs), device, on_device, on_host,
                        lambda r: {k: engine.fb_to_numpy(t) for k, t in r.items()})


def _hist_dict(r, nbins, edges):
    """The dict of gethistogram from the (nco, ni, nto, nbins + 3) counts: views
    of the one array."""
    return {"counts": r[..., :nbins], "below": r[..., nbins], "above": r[..., nbins + 1],
            "nan": r[..., nbins + 2], "edges": edges}


def gethistogram(src, idxs=(COLON, COLON, COLON), *, nbins, lo, hi, fqavby=1, tavby=None,
                 device=0):
    """The distribution of every fqavby x tavby block of the window
    (``tavby=None``: the whole selected time range, ``fqavby=None``: the whole
    selected channel range) from ONE streaming read of the data: a dict with
    ``"counts"`` (int32, (nc/F, ni, nt/T, nbins)), how many samples of the block
    fall into each of ``nbins`` equal bins of [lo, hi), ``"below"``, ``"above"``
    and ``"nan"`` (int32, (nc/F, ni, nt/T)), the samples under lo, at or over hi
    and the NaNs, all views of one array whose planes add up to F * T, and
    ``"edges"``, the nbins + 1 Float64 bin edges (a reading aid: the rule of
    include/bldp.h decides; engine.histogram).  Counts are exact.  Files reach
    the GPU as getdata reads them (window_on_device) and a host array is staged
    there, both returning host arrays; a device tensor stays on the device.
    Float32 data only: any other element type (host array, device tensor, 8/16-bit
    SIGPROC file) is a TypeError."""
    B, lo, hi = engine._hist_args(nbins, lo, hi)  # (the ValueError before any file is touched)
    edges = engine.hist_edges(B, lo, hi)
    kw = dict(fqavby=fqavby, tavby=tavby)
    return _hist_dict(_read_moment(
        "gethistogram", "histogram", src, sanitizeidxs(idxs), device,
        lambda x, win: engine.histogram(x, B, lo, hi, win=win, **kw),
        lambda a, win: engine.histogram_host(a, B, lo, hi, win=win, device=device, **kw),
        engine.planes_to_numpy), B, edges)


def _mask_to_device(host_mask, device):
    """A host uint8 / bool mask as a uint8 device tensor of the same shape with
    channel-fastest strides (1, nc, nc*ni), whatever the host order was: the
    layout of the window and of ``outliers``' mask, so a dense mask keeps the
    aligned wide flag loads instead of strided bytes."""
    import torch

    m = np.asarray(host_mask).view(np.uint8)
    if m.ndim != 3:  # (engine's checks word the error)
        return torch.from_numpy(np.ascontiguousarray(m)).to(device)
    return torch.from_numpy(np.ascontiguousarray(m.transpose(2, 1, 0))).to(device).permute(2, 1, 0)


def _hits_to_host(r):
    """The dict of getflagged / gethits with host arrays: 3-D planes through
    fb_to_numpy, the lists copied as they are."""
    return {k: v if isinstance(v, int) else engine.fb_to_numpy(v) if v.dim() == 3
            else v.cpu().numpy() for k, v in r.items()}


def _hits_coords(h, wshape):
    """engine.hits' dict with the samples' 0-based (channel, if, time) beside
    the linear index."""
    c, i, t = engine.hits_unravel(h["index"], wshape)
    return {"total": h["total"], "index": h["index"], "channel": c, "if": i, "time": t,
            "value": h["value"]}


def getflagged(src, idxs=(COLON, COLON, COLON), *, mask, maxhits=None, device=0):
    """The samples of the window that ``mask`` flags, as an ordered list: Julia's
    ``findall(!iszero, mask)`` and ``A[mask]`` on the GPU (engine.hits; the rule of
    include/bldp.h).  A dict with ``"total"`` (int), the number of flagged
    samples, always exact, and for the first min(total, maxhits) of them
    (``maxhits=None``: all) in ascending linear window index: ``"index"`` (int64,
    0-based, c + nc*(i + ni*t)), ``"channel"``, ``"if"``, ``"time"`` (int64,
    0-based) and ``"value"`` (float32, the samples' bits untouched).  ``mask`` has
    the window's shape (nc, ni, nt), any axis of which may be 1; uint8 or bool, a
    host array or a device tensor (it goes to where the data is).  Files reach the
    GPU as getdata reads them (window_on_device) and a host array is staged
    there, both returning host arrays; a device tensor's lists stay on the device.
    Float32 data only: any other element type (host array, device tensor, 8/16-bit
    SIGPROC file) is a TypeError."""
    cap = engine._hits_cap(maxhits)  # (the errors before any file is touched)
    if _is_tensor(mask):
        mdt, host_mask = str(mask.dtype).replace("torch.", ""), None
    else:
        host_mask = np.asarray(mask)
        mdt = str(host_mask.dtype)
    if mdt not in ("uint8", "bool"):
        raise TypeError(f"getflagged: the mask must be uint8 or bool, not {mdt}")

    def on_device(x, win):
        m = mask.to(x.device) if host_mask is None else _mask_to_device(host_mask, x.device)
        h = engine.hits(x, m, maxhits=cap, win=win)
        return _hits_coords(h, engine.window_shape(win, tuple(x.shape)))

    def on_host(a, win):
        m = host_mask if host_mask is not None else mask.cpu().numpy()
        h = engine.hits_host(a, m, maxhits=cap, win=win, device=device)
        return _hits_coords(h, engine.window_shape(win, a.shape))

    return _read_moment("getflagged", "hits", src, sanitizeidxs(idxs), device, on_device, on_host,
                        _hits_to_host)


def gethits(src, idxs=(COLON, COLON, COLON), *, n=None, axis=2, nsigma=5.0, maxhits=None,
            device=0):
    """Flag and list on the device: engine.outliers flags every block of ``n``
    selected channels (``axis=0``) or spectra (``axis=2``; ``n=None``: the whole
    selected time range) at ``nsigma`` scaled mads from its median, and
    engine.hits lists the flagged samples of the same device tensor; the mask
    never leaves the device.  A dict with ``"total"`` (int, always exact) and, for
    the first min(total, maxhits) flagged samples in ascending linear window
    index (``maxhits=None``: all), ``"channel"``, ``"if"``, ``"time"`` (int64,
    0-based), ``"value"`` (float32) and ``"snr"`` (float64): (Float64(value) -
    Float64(median_b)) / Float64(mad_b) for the sample's block b, signed, so a
    caller can keep one side; and the ``"median"``, ``"mad"`` and ``"count"``
    planes of ``outliers``.  Files, host arrays and device tensors as getflagged
    takes them; Float32 data only."""
    ax, _, _ = engine._outliers_args(axis, nsigma, engine.OUTLIER_PLANES)  # (errors first)
    cap = engine._hits_cap(maxhits)

    def on_device(x, win):
        wshape = engine.window_shape(win, tuple(x.shape))
        o = engine.outliers(x, n=n, axis=axis, nsigma=nsigma, win=win, mask=True)
        h = _hits_coords(engine.hits(x, o["mask"], maxhits=cap, win=win), wshape)
        nb = engine._outliers_n(n, ax, wshape[0], wshape[2])
        c, i, t = h["channel"], h["if"], h["time"]
        blk = (c // nb, i, t) if ax == 0 else (c, i, t // nb)
        h["snr"] = engine.hits_snr(h["value"], o["median"][blk], o["mad"][blk])
        del h["index"]
        h.update(median=o["median"], mad=o["mad"], count=o["count"])
        return h

    def on_host(a, win):  # staged whole, so that both halves read one device tensor
        import torch

        dev = f"cuda:{device}"
        with torch.cuda.device(dev):
            return _hits_to_host(on_device(engine.fb_from_numpy(a, device=dev), win))

    return _read_moment("gethits", "gethits", src, sanitizeidxs(idxs), device, on_device, on_host,
                        _hits_to_host)


def _source_nfpc(src, nfpc, what):
    """``nfpc`` as given, or the file header's; an array source must name it."""
    if nfpc is not None:
        if int(nfpc) < 1:
            raise ValueError(f"{what}: nfpc={nfpc!r} is less than 1")
        return int(nfpc)
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        return int(readers.getheader(src)["nfpc"])
    raise ValueError(f"{what}: an array source has no header; name nfpc")


def getbandpass(src, idxs=(COLON, COLON, COLON), *, nfpc=None, tavby=None, func="mean", mask=None,
                device=0):
    """The window folded over its coarse channels: a dict with ``"data"``, the
    (nfpc, ni, nto) ``func`` (``"sum"`` or ``"mean"``) over every coarse channel and
    every block of ``tavby`` selected spectra (``None``: the whole selected time
    range) at each fine-channel index, and ``"kept"`` (int32), the samples that went
    into it (engine.fold; the rule of include/bldp.h).  ``nfpc=None`` takes the file
    header's ``nfpc``; an array source must name it.  ``mask``: None, or flags of the
    window's shape as getmasked takes them.  Files reach the GPU as getdata reads
    them and a host array is staged there, both returning host arrays; a device
    tensor stays on the device.  Float32 data only."""
    engine._masked_op(func)  # (the ValueErrors before any file is touched)
    host_mask = None
    if mask is not None:
        if _is_tensor(mask):
            mdt = str(mask.dtype).replace("torch.", "")
        else:
            host_mask = np.asarray(mask)
            mdt = str(host_mask.dtype)
        if mdt not in ("uint8", "bool"):
            raise TypeError(f"getbandpass: the mask must be uint8 or bool, not {mdt}")
    nfpc = _source_nfpc(src, nfpc, "getbandpass")
    kw = dict(nfpc=nfpc, tavby=tavby, op=func)

    def on_device(x, win):
        m = mask
        if host_mask is not None:
            import torch

            m = torch.from_numpy(np.ascontiguousarray(host_mask.view(np.uint8)))
        return engine.fold(x, mask=None if m is None else m.to(x.device), win=win, **kw)

    def on_host(a, win):
        m = host_mask if host_mask is not None or mask is None else mask.cpu().numpy()
        return engine.fold_host(a, mask=m, win=win, device=device, **kw)

    return _read_moment("getbandpass", "fold", src, sanitizeidxs(idxs), device, on_device, on_host,
                        lambda r: {k: engine.fb_to_numpy(t) for k, t in r.items()})


def getflattened(src, idxs=(COLON, COLON, COLON), *, nfpc=None, tavby=None, how="divide", n=None,
                 axis=2, nsigma=None, device=0):
    """Fold and unfold on one device tensor: the window divided by
    (``how="divide"``) or less (``"subtract"``) its own mean profile over the coarse
    channels.  A dict with ``"data"``, the flattened (nc, ni, nt) window,
    ``"profile"``, the (nfpc, ni, nto) mean of engine.fold, and ``"kept"`` (int32).
    With ``nsigma``, engine.outliers first flags every block of ``n`` selected
    channels (``axis=0``) or spectra (``axis=2``; ``n=None``: the whole selected time
    range) and the profile is folded over the unflagged samples alone; the mask
    never leaves the device.  Sources and ``nfpc`` as getbandpass takes them;
    Float32 data only."""
    engine._unfold_op(how)  # (the ValueErrors before any file is touched)
    if nsigma is not None:
        engine._outliers_args(axis, nsigma, ("count",))
    nfpc = _source_nfpc(src, nfpc, "getflattened")

    def on_device(x, win):
        m = None
        if nsigma is not None:
            m = engine.outliers(x, n=n, axis=axis, nsigma=nsigma, win=win, mask=True,
                                which=("count",))["mask"]
        p = engine.fold(x, nfpc, tavby, "mean", mask=m, win=win)
        return {"data": engine.unfold(x, p["data"], nfpc, tavby, how, win=win),
                "profile": p["data"], "kept": p["kept"]}

    def on_host(a, win):  # staged whole, so that every step reads one device tensor
        import torch

        dev = f"cuda:{device}"
        with torch.cuda.device(dev):
            return {k: engine.fb_to_numpy(t)
                    for k, t in on_device(engine.fb_from_numpy(a, device=dev), win).items()}

    return _read_moment("getflattened", "getflattened", src, sanitizeidxs(idxs), device, on_device,
                        on_host, lambda r: {k: engine.fb_to_numpy(t) for k, t in r.items()})


def _dedop_seg(src, nfpc, what):
    """The segment length of a dedoppler: ``nfpc`` as ``_source_nfpc`` takes it, or
    0 for the whole window as one segment."""
    if nfpc is not None and not isinstance(nfpc, bool) and int(nfpc) == 0:
        return 0
    return _source_nfpc(src, nfpc, what)


def _dense_window(x, win):
    """The selected window of a device tensor as a dense Julia-order copy."""
    if win is None:
        return engine.fb_empty(*x.shape, device=x.device).copy_(x)
    import torch

    for ax in range(3):
        st, ct, sp = win[3 * ax: 3 * ax + 3]
        x = x.index_select(ax, st + sp * torch.arange(ct, device=x.device))
    return engine.fb_empty(*x.shape, device=x.device).copy_(x)


def _on_staged(on_device, device, to_host):
    """``on_host`` of a composition: the host window staged whole on ``device`` so
    that every step reads one device tensor."""
    def on_host(a, win):
        import torch

        dev = f"cuda:{device}"
        with torch.cuda.device(dev):
            return to_host(on_device(engine.fb_from_numpy(a, device=dev), win))
    return on_host


def _planes_to_host(r):
    return {k: engine.fb_to_numpy(t) if t.dim() == 3 else engine.planes_to_numpy(t)
            for k, t in r.items()}


def getdedoppler(src, idxs=(COLON, COLON, COLON), *, maxdrift, tavby=None, nfpc=None,
                 despike=False, sums=False, device=0):
    """The drift-rate sums of every channel of the window (engine.dedoppler; the
    rule of include/bldp.h): a dict with ``"best"`` (Float32, (nc, ni, nb)), the
    greatest sum over the drifts -maxdrift .. maxdrift of every channel and block
    of ``tavby`` selected spectra (``None``: the whole selected time range),
    ``"drift"`` (int32), the channels that path moves over a block, and with
    ``sums`` ``"sums"`` ((nc, ni, nb, 2*maxdrift + 1); for zoom windows).  No path
    leaves its coarse channel of ``nfpc`` selected channels: ``nfpc=None`` takes the
    file header's (an array source must name it), ``nfpc=0`` makes the whole
    window one segment.  ``despike=True`` first gives every coarse channel's DC bin
    its left neighbour's value (engine.despike) on a device copy of the window.
    Files reach the GPU as getdata reads them and a host array is staged there,
    both returning host arrays; a device tensor stays on the device.  Float32 data
    only."""
    seg = _dedop_seg(src, nfpc, "getdedoppler")
    if despike and seg < 1:
        raise ValueError("getdedoppler: despike needs the coarse channels (nfpc >= 1)")
    kw = dict(maxdrift=maxdrift, tavby=tavby, seg=seg, sums=sums)

    def on_device(x, win):
        if despike:
            x, win = engine.despike(_dense_window(x, win), seg), None
        return engine.dedoppler(x, win=win, **kw)

    on_host = _on_staged(on_device, device, _planes_to_host) if despike else \
        (lambda a, win: engine.dedoppler_host(a, win=win, device=device, **kw))
    return _read_moment("getdedoppler", "dedoppler", src, sanitizeidxs(idxs), device, on_device,
                        on_host, _planes_to_host)


def getdrifthits(src, idxs=(COLON, COLON, COLON), *, maxdrift, tavby=None, nfpc=None, n=None,
                 nsigma=5.0, maxhits=None, device=0):
    """Search and list on the device: engine.dedoppler gives every channel's best
    drift-rate sum, engine.outliers flags the channels of that plane that lie
    ``nsigma`` scaled mads from the median of their block of ``n`` channels
    (``None``: ``nfpc``, or the whole plane when ``nfpc=0``), and engine.hits lists
    them; nothing but the list leaves the device.  gethits' dict over the (nc, ni,
    nb) best plane (``"time"`` is the block) with ``"drift"`` (int32), each hit's
    channels per block, and, when the source is a file, ``"drift_rate"`` in Hz/s
    (engine.drift_rates with the header's foff, times the window's channel step,
    and tsamp).  ``maxdrift``, ``tavby`` and ``nfpc`` as getdedoppler takes them."""
    engine._outliers_args(0, nsigma, engine.OUTLIER_PLANES)  # (errors first)
    cap = engine._hits_cap(maxhits)
    seg = _dedop_seg(src, nfpc, "getdrifthits")
    idxs = sanitizeidxs(idxs)
    hdr = None
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        hdr = readers.getheader(src)

    def on_device(x, win):
        d = engine.dedoppler(x, maxdrift, tavby, seg, win=win)
        best = d["best"]
        nb = engine._outliers_n(n if n is not None else (seg or best.shape[0]), 0, best.shape[0],
                                best.shape[2])
        o = engine.outliers(best, n=nb, axis=0, nsigma=nsigma, mask=True)
        h = _hits_coords(engine.hits(best, o["mask"], maxhits=cap), tuple(best.shape))
        c, i, t = h["channel"], h["if"], h["time"]
        h["snr"] = engine.hits_snr(h["value"], o["median"][c // nb, i, t], o["mad"][c // nb, i, t])
        h["drift"] = d["drift"][c, i, t]
        if hdr is not None:
            T = x.shape[2] if tavby is None and win is None else \
                (engine.window_shape(win, x.shape)[2] if tavby is None else int(tavby))
            step = idxs[0].step if hasattr(idxs[0], "step") and idxs[0].step else 1
            rates = engine.drift_rates(maxdrift, T, float(hdr["foff"]) * step, hdr["tsamp"])
            h["drift_rate"] = _torch_from(rates, x.device)[h["drift"].long() + int(maxdrift)]
        del h["index"]
        h.update(median=o["median"], mad=o["mad"], count=o["count"])
        return h

    return _read_moment("getdrifthits", "getdrifthits", src, idxs, device, on_device,
                        _on_staged(on_device, device, _hits_to_host), _hits_to_host)


def _torch_from(a, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


getinventory = readers.getinventory
getfbheader = readers.getfbheader
getfbh5header = readers.getfbh5header
getheader = readers.getheader
