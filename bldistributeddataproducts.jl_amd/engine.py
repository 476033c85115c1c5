"""Device-side operations on filterbank tensors, all through libbldp_hip.

Layout: a filterbank is a torch tensor whose LOGICAL shape is Julia's
``(nchan, nif, ntime)`` and whose memory is channel-fastest, i.e. strides
``(1, nchan, nchan*nif)`` — a ``permute(2, 1, 0)`` view of a contiguous
``[ntime][nif][nchan]`` buffer, the on-disk FBH5 order (SURVEY.md §8 notation).
Views with larger pitches (sub-windows of a bigger array) are accepted as-is;
anything else is rejected rather than silently copied.

torch supplies device memory and streams only; every byte of arithmetic runs
in the HIP kernels of libbldp_hip.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from . import _lib
from .idxs import window_shape

__all__ = [
    "fb_empty", "fb_from_numpy", "fb_to_numpy", "reduce", "band_reduce", "PreparedBandReduce",
    "band_reduce_multi",
    "stitch",
    "despike", "kurtosis", "kurtosis_blocks_plan", "band_kurtosis", "synth", "plan", "reduce_host", "kurtosis_host",
    "tstat", "tstat_plan", "band_tstat", "tstat_host",
    "quantile", "quantile_plan", "band_quantile", "quantile_host",
    "quantiles", "quantiles_plan", "band_quantiles", "quantiles_host", "planes_empty",
    "planes_to_numpy",
    "OUTLIER_PLANES", "outliers", "outliers_plan", "band_outliers", "outliers_host",
    "skewness", "skewness_plan", "band_skewness", "skewness_host",
    "Moments", "MOMENTS", "moments", "moments_plan", "band_moments", "moments_host",
    "argext", "argext_plan", "band_argext", "argext_host",
    "init", "finalize", "pinned",
]


def _torch():
    import torch

    return torch


def init(devices=None) -> None:
    """bldp_init: check the devices are gfx950, create their worker streams and
    a warm host-staging pipeline each, enable peer access between them.
    ``None`` = every visible device.  Optional (everything initialises lazily)."""
    L = _lib.lib()
    if devices is None:
        _lib.check(L.bldp_init(0, None), "bldp_init")
        return
    devs = [int(d) for d in devices]
    arr = (ctypes.c_int * len(devs))(*devs)
    _lib.check(L.bldp_init(len(devs), ctypes.cast(arr, ctypes.c_void_p)), "bldp_init")


def finalize() -> None:
    """bldp_finalize: drain the devices and free every library-owned resource."""
    _lib.check(_lib.lib().bldp_finalize(), "bldp_finalize")


class pinned:
    """Context manager page-locking a long-lived host numpy array for the
    host-array entry points (bldp_host_register / bldp_host_unregister)."""

    def __init__(self, a: np.ndarray):
        self.a = a

    def __enter__(self):
        if self.a.nbytes:
            _lib.check(_lib.lib().bldp_host_register(self.a.ctypes.data, self.a.nbytes),
                       "bldp_host_register")
        return self.a

    def __exit__(self, *exc):
        if self.a.nbytes:
            _lib.check(_lib.lib().bldp_host_unregister(self.a.ctypes.data), "bldp_host_unregister")
        return False


def fb_empty(nchan, nif, ntime, device=None, dtype=None):
    """Uninitialised Julia-order (nchan, nif, ntime) Float32 tensor on the GPU."""
    torch = _torch()
    dtype = dtype or torch.float32
    return torch.empty((int(ntime), int(nif), int(nchan)), dtype=dtype,
                       device=device or "cuda").permute(2, 1, 0)


def band_empty(nbank, nchan, nif, ntime, device=None, dtype=None):
    """A band's banks as Julia-order (nchan, nif, ntime) views of ONE device
    slab, bank b at element offset b*nchan*nif*ntime.  Streaming a band out of
    one slab measured 2.4% faster on MI355X than out of per-bank allocations
    (7.03 vs 6.86 TB/s on the 0000 band, bench.py --band-alloc)."""
    torch = _torch()
    dtype = dtype or torch.float32
    per = int(nchan) * int(nif) * int(ntime)
    slab = torch.empty(int(nbank) * per, dtype=dtype, device=device or "cuda")
    return [slab[b * per:(b + 1) * per].view(int(ntime), int(nif), int(nchan)).permute(2, 1, 0)
            for b in range(int(nbank))]


def fb_from_numpy(a: np.ndarray, device=None):
    """Host (nchan, nif, ntime) array -> device tensor with the same layout."""
    torch = _torch()
    a = np.asfortranarray(np.asarray(a, dtype=np.float32))
    if a.ndim != 3:
        raise ValueError("filterbank arrays are 3-D (nchan, nif, ntime)")
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0)))
    return t.to(device or "cuda").permute(2, 1, 0)


_d2h_streams: dict = {}


def device_to_host(c, stats=None) -> np.ndarray:
    """A contiguous device tensor into a new ordinary (pageable) numpy array
    of the same shape through the library's pinned slot ring
    (bldp_device_to_host: slot-sized DMAs overlapped with the slots' copy-out
    by the reader threads).  Ordered after the work queued on torch's current
    stream of the tensor's device.  No pinned memory is allocated or held: the
    result is the caller's ordinary memory (what torch's pinned caching
    allocator would have kept page-locked, rounded up to a power of two, for as
    long as the array lives and after)."""
    torch = _torch()
    if not c.is_contiguous():
        raise ValueError("device_to_host needs a contiguous tensor")
    h = np.empty(tuple(c.shape), dtype=np.dtype(str(c.dtype).replace("torch.", "")))
    if h.nbytes == 0:
        return h
    dev = c.device
    with torch.cuda.device(dev):
        cs = _d2h_streams.get(dev.index)
        if cs is None:
            cs = _d2h_streams[dev.index] = torch.cuda.Stream(dev, priority=-1)
        st = (ctypes.c_double * 4)()
        rc = _lib.lib().bldp_device_to_host(c.data_ptr(), h.ctypes.data, h.nbytes, cs.cuda_stream,
                                            _lib.stream_ptr(), st)
    _lib.check(rc, "bldp_device_to_host")
    if stats is not None:
        stats.update(first_dma_ms=st[0], total_ms=st[1], slots=int(st[2]), threads=int(st[3]))
    return h


def fb_to_numpy(t, pinned=False) -> np.ndarray:
    """Device tensor (Julia order) -> Fortran-ordered numpy array.  With
    ``pinned`` the copy goes through the library's pinned slot ring
    (device_to_host: DMA at PCIe speed instead of torch's staged copy into
    pageable memory, ~7 GB/s) into ordinary memory the array owns.  A 4-D plane
    tensor (``quantiles``) goes through ``planes_to_numpy``."""
    if t.dim() == 4:
        return planes_to_numpy(t)
    torch = _torch()
    c = t.permute(2, 1, 0).contiguous() if t.dim() == 3 else t.t().contiguous()
    if pinned and c.is_cuda:
        h = device_to_host(c)
    else:
        h = c.cpu().numpy()
    return np.asfortranarray(h.transpose(2, 1, 0) if t.dim() == 3 else h.T)


def peer_access(dev, peer) -> bool:
    """bldp_peer_access: may kernels on ``dev`` store straight into memory of
    ``peer`` (same device, or xGMI peer access, enabled here)?"""
    d = ctypes.c_int()
    _lib.check(_lib.lib().bldp_peer_access(int(dev), int(peer), ctypes.byref(d)), "bldp_peer_access")
    return bool(d.value)


def _abi_dims(t, allow_typed=False):
    """Map a channel-fastest tensor to (ptr, nchan, nif, ntime) of an array
    that contains it, so that its logical index (c, i, t) is element
    c + nchan*(i + nif*t) of the ABI array.

    Float32 only unless ``allow_typed``: every caller but the typed entry
    points (reduce / kurtosis, which branch to bldp_reduce_strided and
    bldp_kurtosis) hands the pointer to an ``_f32`` function."""
    code = _dtype_code(t.dtype)
    if code is None or (code != 0 and not allow_typed):
        raise TypeError(f"unsupported filterbank element type {t.dtype} (Float32 expected)")
    if not t.is_cuda:
        raise TypeError("device tensor expected (use getdata/reduce_host for host arrays)")
    if t.dim() != 3:
        raise ValueError("filterbank tensors are 3-D (nchan, nif, ntime)")
    n0, n1, n2 = t.shape
    s0, s1, s2 = t.stride()
    if n0 > 1 and s0 != 1:
        raise ValueError("channel axis must be the fastest (stride 1); use fb_empty layout")
    if n1 > 1 and n2 > 1:
        if s1 < n0 or s2 % s1 or s2 // s1 < n1:
            raise ValueError(f"unsupported strides {t.stride()} for shape {tuple(t.shape)}")
        nchan, nif = s1, s2 // s1
    elif n1 > 1:
        if s1 < n0:
            raise ValueError(f"unsupported strides {t.stride()}")
        nchan, nif = s1, n1
    else:
        nchan = s2 if (n2 > 1 and s2 >= n0) else n0
        if n2 > 1 and s2 < n0:
            raise ValueError(f"unsupported strides {t.stride()}")
        nif = 1
    return t.data_ptr(), int(nchan), int(nif), int(n2)


# bldp_dtype codes (include/bldp.h) by numpy element type
DTYPE_CODES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint8): 2,
               np.dtype(np.uint16): 3, np.dtype(np.uint32): 4, np.dtype(np.uint64): 5,
               np.dtype(np.int8): 6, np.dtype(np.int16): 7, np.dtype(np.int32): 8,
               np.dtype(np.int64): 9}
DTYPE_OF_CODE = {v: k for k, v in DTYPE_CODES.items()}


_dtype_codes: dict = {}  # _dtype_code's answers by dtype object: every call asks, for the same few


def _dtype_code(dt):
    """bldp_dtype of a numpy dtype or torch dtype (None if unsupported)."""
    try:
        return _dtype_codes[dt]
    except (KeyError, TypeError):  # (TypeError: not hashable, so not remembered either)
        pass
    key = dt
    if not isinstance(dt, np.dtype):
        try:
            dt = np.dtype(str(dt).replace("torch.", ""))
        except TypeError:
            return None
    code = DTYPE_CODES.get(np.dtype(dt))
    try:
        _dtype_codes[key] = code
    except TypeError:
        pass
    return code


def _quantile_kind(op):
    """"quantile" / "quantiles" for those function tuples (their p's checked:
    ValueError), else None."""
    if isinstance(op, str):  # (the common case, and never a tuple)
        return None
    if _lib.quantile_of(op) is not None:
        return "quantile"
    return "quantiles" if _lib.quantiles_of(op) is not None else None


def _no_quantile(op, what) -> None:
    if _quantile_kind(op):
        raise TypeError(f"{what} takes the ops of enum bldp_op; a quantile goes through "
                        f"engine.quantile / band_quantile")


def _route_quantile(op, form, data, n, axis, *rest):
    """An ``op`` that is ``("quantile", p)`` or ``("quantiles", ps)`` goes to that
    family's ``form`` ("", "_plan", "band_", "_host") with blocks of ``n`` on
    ``axis``; None for every other op."""
    kind = _quantile_kind(op)
    if kind is None:
        return None
    name = "band_" + kind if form == "band_" else kind + form
    return globals()[name](data, n, op[1], axis, *rest)


def _check_stat(op: str, tavby, dtype=None) -> None:
    """var / std / median / mad: no time integration, Float32 on the GPU (TypeError,
    as Julia's MethodError for an fqavfunc the call does not fit)."""
    if not _lib.stat_op(op):
        return
    if int(tavby) > 1:
        raise TypeError(f"fqavfunc {op!r} has no time integration: tavby={tavby} needs "
                        f"sum/mean/max/min")
    if dtype is not None and _dtype_code(dtype) != 0:
        raise TypeError(f"fqavfunc {op!r} runs on the GPU for Float32 data only, not {dtype}")


def out_dtype(dtype, op: str) -> np.dtype:
    """fqav's result element type for input `dtype` (Julia's; bldp_reduce_out_dtype):
    sum widens integers to (U)Int64, mean is Float64, max / min keep the type;
    var / std / median / mad are Float32 of Float32 and Float64 of anything else."""
    code = _dtype_code(dtype)
    if code is None:
        raise TypeError(f"unsupported element type {dtype}")
    if _quantile_kind(op):
        op = "median"  # (no op of the ABI: the median's types)
    rc = _lib.lib().bldp_reduce_out_dtype(code, _lib.OPS[op])
    _lib.check(min(rc, 0), "bldp_reduce_out_dtype")
    return DTYPE_OF_CODE[rc]


def _torch_dtype(dt: np.dtype):
    torch = _torch()
    return getattr(torch, np.dtype(dt).name)


def _check_bounds(win, shape):
    if win is None:
        return
    for ax in range(3):
        st, ct, sp = win[3 * ax: 3 * ax + 3]
        if ct > 0:
            last = st + (ct - 1) * sp
            if min(st, last) < 0 or max(st, last) >= shape[ax]:
                raise _lib.BoundsError(
                    _lib.BLDP_EBOUNDS,
                    f"BoundsError: window {st + 1}:{sp}:{last + 1} outside axis {ax + 1} of "
                    f"size {shape[ax]}")


def _full_win(win, shape):
    return list(win) if win is not None else [0, shape[0], 1, 0, shape[1], 1, 0, shape[2], 1]


def out_shape(shape, win, fqavby, tavby):
    nc, ni, nt = window_shape(win, shape)
    F, T = max(int(fqavby), 1), max(int(tavby), 1)
    if nc % F:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: fqavby={F} does not divide nchan={nc}")
    if nt % T:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: tavby={T} does not divide ntime={nt}")
    return nc // F, ni, nt // T


# The block operations (reduce, tstat, quantile(s), outliers, argext, masked
# reduce, histogram, hits, fold, unfold, dedoppler) come in four forms: the device call, its
# plan, the band and the host call.  The helpers below state once what the forms
# share; each public function applies its family's own checks between them, in
# its own order (tests/test_engine_front_errors.py pins that order).
def _window(x, win):
    """(shape, window shape) of a tensor or host array, the window inside it
    (BoundsError)."""
    shape = tuple(x.shape)
    if win is None:
        return shape, shape
    _check_bounds(win, shape)
    return shape, window_shape(win, shape)


def _win_ptr(win, shape):
    """(keep-alive, window pointer) of the ABI's nine int64 (a band passes it after
    its banks' pointers)."""
    return _lib.win_arg(_full_win(win, shape))


def _win_args(x, win, allow_typed=False):
    """What the ABI takes for a window of a device tensor: ((pointer, nchan, nif,
    ntime, window pointer), keep-alive).  The window has passed ``_window``."""
    dims = _abi_dims(x, allow_typed)
    keep, wp = _lib.win_arg(_full_win(win, x.shape))
    return (*dims, wp), keep


def _host_args(device, a, win):
    """``_win_args`` of a host array staged on ``device``: ((device, pointer,
    nchan, nif, ntime, window pointer), keep-alive)."""
    keep, wp = _lib.win_arg(_full_win(win, a.shape))
    return (int(device), _np_ptr(a), *a.shape, wp), keep


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _np_ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _host_fb(a, what=None, fn=None):
    """A host filterbank: a Fortran-ordered float32 (nchan, nif, ntime) array.
    ``what``: the caller's name in the TypeError of another element type (``fn``
    names the operation); None for the forms that only give the general one."""
    a = np.asarray(a)
    if what and a.dtype != np.float32:
        _need_f32(what, a.dtype, fn)
    if a.dtype != np.float32 or not a.flags.f_contiguous or a.ndim != 3:
        raise TypeError("host filterbank must be a Fortran-ordered float32 (nchan, nif, ntime)")
    return a


def _host_out(dims, dtype=np.float32):
    """Fortran-ordered host output of ``dims``.  int32: the ABI writes uint32
    offsets and counts, all below 2^31."""
    return np.empty(dims, dtype=dtype, order="F")


def _banks(banks, what=None, fn=None, agree=True, devices=False):
    """The banks of a band on one GPU: (banks, nbank, their pointers as the ABI's
    void*, (nchan, nif, ntime) every bank shares).  ``what`` / ``fn``: the banks
    must be Float32, named so in the TypeError; ``agree=False`` stops there
    (geometry None); ``devices``: the banks must share a device too."""
    banks = list(banks)
    if not banks:
        raise ValueError("no banks")
    if what:
        f32 = _torch().float32
        for b in banks:
            if b.dtype != f32:
                _need_f32(what, b.dtype, fn)
    geo = None
    if agree:
        shape = tuple(banks[0].shape)
        for b in banks:
            g = _abi_dims(b)[1:] if tuple(b.shape) == shape else None
            if geo is None and g is not None:
                geo = g
            if g != geo or (devices and b.device != banks[0].device):
                raise ValueError("all banks of a band must have the same shape"
                                 + (", layout and device" if devices else " and layout"))
    ptrs = (ctypes.c_void_p * len(banks))(*[b.data_ptr() for b in banks])
    return banks, len(banks), ctypes.cast(ptrs, ctypes.c_void_p), geo


def _axis_factors(n, axis):
    """(fqavby, tavby) of blocks of ``n`` along ``axis`` (0: channels, 2: spectra)."""
    return (n, 1) if axis == 0 else (1, n)


def _out_layout(t, dims, device, dtype, name="out", dtname=None, planes=None, loose=False):
    """A caller's output tensor, checked before any launch: a ``dtype`` tensor of
    shape ``dims`` (``(*dims, planes)`` with planes) on ``device`` with the
    channels fastest and rows that do not overlap; returns (pointer, ld_i, ld_t),
    with planes also ld_q (``_plane_ld``).  ``loose``: unfold's rule, which leaves
    the rows to the library."""
    torch = _torch()
    nc, ni, nt = dims
    full = tuple(dims) if planes is None else (*dims, planes)
    if loose:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError(f"{name} must be a {dtname} device tensor, not "
                            f"{getattr(t, 'dtype', type(t).__name__)}")
    else:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a device tensor")
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {dtname or dtype}, not {t.dtype}")
    if tuple(t.shape) != full:
        raise ValueError(f"{name} is {tuple(t.shape)}, expected {full}")
    if t.device != torch.device(device):
        raise ValueError(f"{name} is on {t.device}, the data on {device}")
    s0, s1, s2 = t.stride()[:3]
    ld_i = s1 if ni > 1 else nc
    ld_t = s2 if nt > 1 else max(ni - 1, 0) * ld_i + nc
    if loose:
        if nc > 1 and s0 != 1:
            raise ValueError(f"{name} strides {t.stride()}: the channels must be the fastest axis")
    elif (nc > 1 and s0 != 1) or ld_i < nc or ld_t < (ni - 1) * ld_i + nc:
        raise ValueError(f"{name} strides {t.stride()} are not a Julia-order (channel-fastest) "
                         f"layout of {(nc, ni, nt)}" + ("" if planes is None else " planes"))
    if planes is None:
        return _ptr(t), ld_i, ld_t
    return _ptr(t), ld_i, ld_t, _plane_ld(t, dims, planes, ld_i, ld_t)


def _plane_ld(t, dims, K, ld_i, ld_t):
    """out_ld_q of a 4-D output of K planes: they may not overlap."""
    nc, ni, nt = dims
    extent = max(nt - 1, 0) * ld_t + max(ni - 1, 0) * ld_i + nc
    ld_q = t.stride(3) if K > 1 else extent
    if ld_q < extent:
        raise ValueError(f"out strides {t.stride()}: the planes overlap")
    return ld_q


# The keys of the plans: the reduce's (blocks of channels, axis 0) and the
# tstat's (blocks of spectra, axis 2), which the quantile, quantiles and outliers
# plans extend, and the argext's, which the masked reduce extends.
REDUCE_PLAN_KEYS = ("path", "lanes_per_group", "time_split_waves", "float4_per_lane",
                    "time_chunks", "workgroups", "workspace_bytes", "vec_out")
TSTAT_PLAN_KEYS = ("path", "channels_per_lane", "time_split_lanes", "passes", "workgroups",
                   "workspace_bytes", "blocks", "channel_lanes")
ARGEXT_PLAN_KEYS = ("path", "lanes_per_block", "time_slices", "float4_per_lane", "workgroups",
                    "workspace_bytes", "outputs", "vector_loads")


def _plan_dict(fn, args, n, keys, **enums):
    """The dict of a plan entry point: ``fn(*args, info)`` fills ``n`` int64, named
    by ``keys``; ``enums`` maps a key's code to its name ("copy" for a code with
    none: the copy of a block of one)."""
    info = (ctypes.c_int64 * n)()
    _lib.check(getattr(_lib.lib(), fn)(*args, info), fn)
    d = dict(zip(keys, info[:]))
    for k, names in enums.items():
        d[k] = names.get(d[k], "copy")
    return d


def _axis_plan(fn, args, n, axis, extra=(), rank=False):
    """``_plan_dict`` with the reduce's keys (axis 0) or the tstat's (axis 2) and
    ``extra``; ``rank``: the rank stands where the workspace bytes do."""
    keys, paths = (REDUCE_PLAN_KEYS, _lib.PATHS) if axis == 0 else \
        (TSTAT_PLAN_KEYS, _lib.TSTAT_PATHS)
    if rank:
        keys = tuple("rank" if k == "workspace_bytes" else k for k in keys)
    return _plan_dict(fn, args, n, keys + tuple(extra), path=paths)


def reduce(x, fqavby=1, tavby=1, op="sum", win=None, out=None, stream=None):
    """fqav on the channel axis fused with time integration, on the GPU.

    x: device filterbank tensor; win: 9-int window (see idxs.to_window) or
    None; returns a Julia-order (nc/F, ni, nt/T) device tensor."""
    _check_stat(op, tavby, x.dtype)
    r = _route_quantile(op, "", x, fqavby, 0, win, out, stream)
    if r is not None:
        return r
    L = _lib.lib()
    shape, _ = _window(x, win)
    nco, ni, nto = out_shape(shape, win, fqavby, tavby)
    torch = _torch()
    typed = x.dtype != torch.float32
    odt = _torch_dtype(out_dtype(x.dtype, op)) if typed else torch.float32
    if out is None:
        out = fb_empty(nco, ni, nto, device=x.device, dtype=odt)
    elif tuple(out.shape) != (nco, ni, nto) or out.dtype != odt:
        raise ValueError(f"out is {out.dtype} {tuple(out.shape)}, expected {odt} {(nco, ni, nto)}")
    optr, onc, oni, _ = _abi_dims(out, allow_typed=True) if out.numel() else (0, nco, ni, nto)
    w, keep = _win_args(x, win, allow_typed=True)
    if typed:  # fqav's Julia result types for integer / Float64 data (bldp_reduce_strided)
        rc = L.bldp_reduce_strided(_dtype_code(x.dtype), *w, int(fqavby), int(tavby),
                                   _lib.OPS[op], optr, onc, onc * oni, _lib.stream_ptr(stream))
        _lib.check(rc, "bldp_reduce_strided")
        return out
    rc = L.bldp_reduce_strided_f32(*w, int(fqavby), int(tavby), _lib.OPS[op], optr, onc,
                                   onc * oni, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_reduce_strided_f32")
    return out


class _Prepared:
    """A bldp_reduce_op_t handle: ``launch`` is one ctypes call that queues
    the kernel(s), ``launch_timed`` the same with two timing HipEvents,
    ``close`` releases it.  Keeps its tensors alive."""

    def _bind(self, L, h, keep):
        self._L, self._h, self._keep = L, h, keep
        self._fn, self._timed = L.bldp_reduce_launch, L.bldp_reduce_launch_timed

    def launch(self, stream=None) -> None:
        sp = stream if isinstance(stream, int) else _lib.stream_ptr(stream)
        rc = self._fn(self._h, sp)
        if rc:
            _lib.check(rc, "bldp_reduce_launch")

    def launch_timed(self, stream, ev_start, ev_stop) -> None:
        sp = stream if isinstance(stream, int) else _lib.stream_ptr(stream)
        rc = self._timed(self._h, sp, ev_start.ev, ev_stop.ev)
        if rc:
            _lib.check(rc, "bldp_reduce_launch_timed")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.bldp_reduce_release(self._h)
            self._h = None

    def __del__(self):
        self.close()


class PreparedReduce(_Prepared):
    """``reduce`` prepared once for fixed buffers, any element type
    (bldp_reduce_prepare): the per-file worker call of
    src/gbtworkerfunctions.jl:171-177 re-run on resident buffers costs one
    ctypes call and the kernel launch.  ``out`` as ``reduce`` makes it."""

    def __init__(self, x, fqavby=1, tavby=1, op="sum", win=None, out=None):
        _check_stat(op, tavby, x.dtype)
        _no_quantile(op, "PreparedReduce")
        torch = _torch()
        L = _lib.lib()
        shape = tuple(x.shape)
        _check_bounds(win, shape)
        nco, ni, nto = out_shape(shape, win, fqavby, tavby)
        odt = _torch_dtype(out_dtype(x.dtype, op)) if x.dtype != torch.float32 else torch.float32
        if out is None:
            out = fb_empty(nco, ni, nto, device=x.device, dtype=odt)
        elif tuple(out.shape) != (nco, ni, nto) or out.dtype != odt:
            raise ValueError(f"out is {out.dtype} {tuple(out.shape)}, expected {odt} "
                             f"{(nco, ni, nto)}")
        optr, onc, oni, _ = _abi_dims(out, allow_typed=True) if out.numel() else (0, nco, ni, nto)
        ptr, nchan, nif, ntime = _abi_dims(x, allow_typed=True)
        keep, wp = _win_ptr(win, shape)
        h = ctypes.c_void_p()
        with torch.cuda.device(x.device):
            rc = L.bldp_reduce_prepare(_dtype_code(x.dtype), ptr, nchan, nif, ntime, wp,
                                       int(fqavby), int(tavby), _lib.OPS[op], optr, onc,
                                       onc * oni, ctypes.byref(h))
        _lib.check(rc, "bldp_reduce_prepare")
        self._bind(L, h, (x, keep))
        self.out = out


class PreparedKurtosis(_Prepared):
    """``kurtosis`` prepared once for fixed buffers, any element type
    (bldp_kurtosis_prepare): getkurtosis (src/gbtworkerfunctions.jl:197-202)
    re-run on a resident window for one ctypes call and the kernel launch."""

    def __init__(self, x, win=None, out=None):
        torch = _torch()
        L = _lib.lib()
        shape = tuple(x.shape)
        _check_bounds(win, shape)
        nc, ni, _ = window_shape(win, shape)
        if out is None:
            out = torch.empty((ni, nc), dtype=torch.float64, device=x.device).t()
        ptr, nchan, nif, ntime = _abi_dims(x, allow_typed=True)
        keep, wp = _win_ptr(win, shape)
        h = ctypes.c_void_p()
        with torch.cuda.device(x.device):
            rc = L.bldp_kurtosis_prepare(_dtype_code(x.dtype), ptr, nchan, nif, ntime, wp,
                                         out.data_ptr() if out.numel() else None,
                                         ctypes.byref(h))
        _lib.check(rc, "bldp_kurtosis_prepare")
        self._bind(L, h, (x, keep))
        self.out = out


def plan(x, fqavby=1, tavby=1, op="sum", win=None) -> dict:
    """Launch plan the library picks for this call (path, lanes/group, ...)."""
    if _quantile_kind(op):
        _check_stat(op, tavby)
        return _route_quantile(op, "_plan", x, fqavby, 0, win)
    _window(x, win)
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_reduce_plan_f32", (*w, int(fqavby), int(tavby), _lib.OPS[op], None),
                      8, REDUCE_PLAN_KEYS, path=_lib.PATHS)


def _band_args(banks, fqavby, tavby, win, out):
    """Checks of a one-GPU band reduce; (banks, geometry, out, the banks' pointers
    as the ABI's void*, window keepalive)."""
    banks, nb, ptrs, geo = _banks(banks)
    shape, _ = _window(banks[0], win)
    nco, ni, nto = out_shape(shape, win, fqavby, tavby)
    if out is None:
        out = fb_empty(nb * nco, ni, nto, device=banks[0].device)
    if _dtype_code(out.dtype) != 0:
        raise TypeError(f"out must be Float32, not {out.dtype}")
    if tuple(out.shape) != (nb * nco, ni, nto) or (
            out.numel() and out.stride() != (1, nb * nco, nb * nco * ni) and ni * nto > 1):
        raise ValueError("out must be a dense Julia-order (nbank*nco, ni, nto) tensor")
    return banks, geo, out, ptrs, _win_ptr(win, shape)


def _band_out_device(out, banks):
    if out.device != banks[0].device:
        raise ValueError(f"out is on {out.device}, the banks on {banks[0].device}")


def band_reduce(banks, fqavby=1, tavby=1, op="sum", win=None, out=None, stream=None):
    """Reduce every bank of a band resident on ONE GPU and stitch them in bank
    order (reduce(vcat, ...), src/gbt.jl:103) in a single launch."""
    _check_stat(op, tavby)
    r = _route_quantile(op, "band_", banks, fqavby, 0, win, out, stream)
    if r is not None:
        return r
    banks, geo, out, ptrs, (keep, wp) = _band_args(banks, fqavby, tavby, win, out)
    rc = _lib.lib().bldp_band_reduce_f32(len(banks), ptrs, *geo, wp, int(fqavby), int(tavby),
                                         _lib.OPS[op], _ptr(out), _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_reduce_f32")
    return out


class PreparedBandReduce:
    """band_reduce prepared once for fixed buffers (bldp_band_reduce_prepare_f32):
    checks, plan and kernel arguments are computed here, and ``launch`` only
    queues the kernel — one ctypes call, no Python-side work.  Results are
    those of ``band_reduce`` with the same arguments.  The banks and ``out``
    are kept alive by the object; ``close`` releases the handle."""

    def __init__(self, banks, fqavby=1, tavby=1, op="sum", win=None, out=None):
        _check_stat(op, tavby)
        _no_quantile(op, "PreparedBandReduce")
        L = _lib.lib()
        banks, geo, out, ptrs, (keep, wp) = _band_args(banks, fqavby, tavby, win, out)
        h = ctypes.c_void_p()
        with _torch().cuda.device(banks[0].device):
            rc = L.bldp_band_reduce_prepare_f32(len(banks), ptrs,
                                                *geo, wp, int(fqavby), int(tavby), _lib.OPS[op],
                                                out.data_ptr() if out.numel() else None,
                                                ctypes.byref(h))
        _lib.check(rc, "bldp_band_reduce_prepare_f32")
        self._L, self._h = L, h
        self._fn = L.bldp_reduce_launch
        self._timed = L.bldp_reduce_launch_timed
        self.banks, self.out = banks, out

    def launch(self, stream=None) -> None:
        """Queue the reduce on ``stream`` (a torch stream, a raw hipStream_t
        int, or None for torch's current stream)."""
        sp = stream if isinstance(stream, int) else _lib.stream_ptr(stream)
        rc = self._fn(self._h, sp)
        if rc:
            _lib.check(rc, "bldp_reduce_launch")

    def launch_timed(self, stream, ev_start, ev_stop) -> None:
        """``launch`` with the reduce's own dispatches carrying two timing
        ``_lib.HipEvent`` s (bldp_reduce_launch_timed): nothing is queued
        between this launch and the next."""
        sp = stream if isinstance(stream, int) else _lib.stream_ptr(stream)
        rc = self._timed(self._h, sp, ev_start.ev, ev_stop.ev)
        if rc:
            _lib.check(rc, "bldp_reduce_launch_timed")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.bldp_reduce_release(self._h)
            self._h = None

    def __del__(self):
        self.close()


def band_reduce_multi(banks, fqavby=1, tavby=1, op="sum", win=None, root=0, out=None,
                      staged=False, peer_store=False):
    """One process, banks on several GPUs (bldp_band_reduce_multi_f32): each
    GPU reduces its banks (one launch per device for contiguous shards) into
    their vcat slots of the stitched product on `root` (into ``out`` when
    given: a dense Julia-order (nbank*nco, ni, nto) Float32 tensor there); a
    device other than the root reduces into staging and one peer copy moves
    its slots.  ``staged``: every bank takes the staged branch
    (BLDP_BAND_STAGED), the root's included; ``peer_store``: devices with peer
    access store their slots over xGMI from the kernels (BLDP_BAND_PEER_STORE,
    opt-in until a multi-GPU node has run it) -- per-call arguments, not
    process state.  sum / mean / max / min only: var / std / median run on one
    device (GBT.getband then goes bank by bank)."""
    if _lib.stat_op(op):
        raise TypeError(f"band_reduce_multi takes sum/mean/max/min, not {op!r}: reduce each "
                        f"device's banks with band_reduce")
    torch = _torch()
    L = _lib.lib()
    banks = list(banks)
    shape = tuple(banks[0].shape)
    geo = _abi_dims(banks[0])[1:]
    for b in banks[1:]:
        if tuple(b.shape) != shape or _abi_dims(b)[1:] != geo:
            raise ValueError("all banks of a band must have the same shape and layout")
    _check_bounds(win, shape)
    nco, ni, nto = out_shape(shape, win, fqavby, tavby)
    if out is None:
        out = fb_empty(len(banks) * nco, ni, nto, device=torch.device("cuda", root))
    elif (_dtype_code(out.dtype) != 0 or tuple(out.shape) != (len(banks) * nco, ni, nto)
          or out.device != torch.device("cuda", root)
          or (out.numel() and ni * nto > 1 and out.stride() != (1, len(banks) * nco,
                                                                 len(banks) * nco * ni))):
        raise ValueError("out must be a dense Julia-order (nbank*nco, ni, nto) Float32 tensor "
                         "on the root device")
    devs = (ctypes.c_int * len(banks))(*[b.device.index for b in banks])
    ptrs = (ctypes.c_void_p * len(banks))(*[b.data_ptr() for b in banks])
    keep, wp = _win_ptr(win, shape)
    for d in {b.device.index for b in banks}:
        torch.cuda.synchronize(d)  # inputs written on torch streams are complete
    rc = L.bldp_band_reduce_multi_f32(len(banks), ctypes.cast(devs, ctypes.c_void_p),
                                      ctypes.cast(ptrs, ctypes.c_void_p), *geo, wp,
                                      int(fqavby), int(tavby), _lib.OPS[op], int(root),
                                      out.data_ptr() if out.numel() else None,
                                      (_lib.BLDP_BAND_STAGED if staged else 0)
                                      | (_lib.BLDP_BAND_PEER_STORE if peer_store else 0))
    _lib.check(rc, "bldp_band_reduce_multi_f32")
    return out


def reduce_host(a: np.ndarray, fqavby=1, tavby=1, op="sum", win=None, device=0) -> np.ndarray:
    """Host array in, host array out (bldp_reduce_host_f32): the window is
    streamed through the GPU and reduced there."""
    _check_stat(op, tavby)
    r = _route_quantile(op, "_host", a, fqavby, 0, win, device)
    if r is not None:
        return r
    a = _host_fb(a)
    shape, _ = _window(a, win)
    out = _host_out(out_shape(shape, win, fqavby, tavby))
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_reduce_host_f32(*h, int(fqavby), int(tavby), _lib.OPS[op], _np_ptr(out))
    _lib.check(rc, "bldp_reduce_host_f32")
    return out


def _tstat_op(op) -> int:
    if not isinstance(op, str) or op not in _lib.STAT_OPS:
        raise _lib.ArgumentError(
            _lib.BLDP_EINVAL, f"tstat takes var/std/median/mad or a quantile, not {op!r} "
                              f"(sum/mean/max/min over time: reduce with tavby)")
    return _lib.OPS[op]


def _tstat_out(out, dims, device):
    """A caller's ``out`` of a tstat, checked before any launch: a Float32
    (nc, ni, nb) tensor on ``device`` with the channels fastest and rows that
    do not overlap; returns (pointer, out_ld_i, out_ld_b)."""
    return _out_layout(out, dims, device, _torch().float32, dtname="Float32")


def tstat(x, tavby, op, win=None, out=None, stream=None):
    """var / std / median / mad of every block of ``tavby`` selected spectra of
    every (channel, IF) column, on the GPU (bldp_tstat_f32): fqav's rule on the
    time axis with Julia's Statistics (mad: StatsBase's normalised one).  x: a Float32 device filterbank tensor;
    returns a Julia-order (nc, ni, nt/tavby) Float32 device tensor (``out``
    when given: e.g. a bank's slot of a stitched product).  tavby <= 1 copies
    the window.  ``op`` may be ``("quantile", p)``: ``quantile`` on axis 2."""
    r = _route_quantile(op, "", x, tavby, 2, win, out, stream)
    if r is not None:
        return r
    code = _tstat_op(op)
    shape, _ = _window(x, win)
    dims = out_shape(shape, win, 1, tavby)
    w, keep = _win_args(x, win)
    if out is None:
        out = fb_empty(*dims, device=x.device)
    o = _tstat_out(out, dims, x.device)
    rc = _lib.lib().bldp_tstat_f32(*w, int(tavby), code, *o, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_tstat_f32")
    return out


def tstat_plan(x, tavby, op, win=None) -> dict:
    """Launch plan of ``tstat(x, tavby, op, win)`` (bldp_tstat_plan_f32): the
    path (_lib.TSTAT_PATHS, "copy" for tavby <= 1), channels per lane, the time
    slices of a workgroup splitting a block (1: the register form), passes over
    the block, workgroups, workspace bytes, blocks and the lanes along the
    channels of a split workgroup."""
    r = _route_quantile(op, "_plan", x, tavby, 2, win)
    if r is not None:
        return r
    code = _tstat_op(op)
    _window(x, win)
    w, keep = _win_args(x, win)
    return _axis_plan("bldp_tstat_plan_f32", (*w, int(tavby), code, None), 8, 2)


def band_tstat(banks, tavby, op, win=None, out=None, stream=None):
    """``tstat`` of every bank of a band resident on ONE GPU, stitched in bank
    order (the vcat of the per-bank results) in one launch
    (bldp_band_tstat_f32): a dense (nbank*nc, ni, nt/tavby) Float32 tensor."""
    r = _route_quantile(op, "band_", banks, tavby, 2, win, out, stream)
    if r is not None:
        return r
    code = _tstat_op(op)
    banks, geo, out, ptrs, (keep, wp) = _band_args(banks, 1, tavby, win, out)
    _band_out_device(out, banks)
    rc = _lib.lib().bldp_band_tstat_f32(len(banks), ptrs, *geo, wp, int(tavby), code, _ptr(out),
                                        _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_tstat_f32")
    return out


def tstat_host(a: np.ndarray, tavby, op, win=None, device=0) -> np.ndarray:
    """Host Fortran-ordered Float32 array in, (nc, ni, nt/tavby) Float32 host
    array out (bldp_tstat_host_f32: the window's rows staged on ``device``)."""
    r = _route_quantile(op, "_host", a, tavby, 2, win, device)
    if r is not None:
        return r
    code = _tstat_op(op)
    a = _host_fb(a)
    shape, _ = _window(a, win)
    out = _host_out(out_shape(shape, win, 1, tavby))
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_tstat_host_f32(*h, int(tavby), code, _np_ptr(out))
    _lib.check(rc, "bldp_tstat_host_f32")
    return out


def _quantile_args(p, axis):
    """(p, axis) of a quantile call, checked before any GPU work."""
    p = _lib.quantile_p(p)
    if axis not in (0, 2):
        raise ValueError(f"quantile: axis {axis!r} is not 0 (blocks of channels) or 2 (blocks "
                         f"of spectra)")
    return p, int(axis)


def quantile(x, n, p, axis=0, win=None, out=None, stream=None):
    """Statistics.quantile(block, p) (type 7) of every block of ``n`` channels
    (axis 0, the blocks of ``reduce``) or of ``n`` selected spectra (axis 2, the
    blocks of ``tstat``) of a Float32 device filterbank tensor, on the GPU
    (bldp_quantile_f32): the median's kernels selecting ranks j - 1 and j.  A
    block holding a NaN gives NaN; n <= 1 copies the window.  Returns a
    Julia-order (nc/n, ni, nt) or (nc, ni, nt/n) Float32 device tensor (``out``
    when given, laid out as ``tstat`` takes it)."""
    p, axis = _quantile_args(p, axis)
    shape, _ = _window(x, win)
    dims = out_shape(shape, win, *_axis_factors(n, axis))
    w, keep = _win_args(x, win)
    if out is None:
        out = fb_empty(*dims, device=x.device)
    o = _tstat_out(out, dims, x.device)
    rc = _lib.lib().bldp_quantile_f32(*w, axis, int(n), p, *o, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_quantile_f32")
    return out


def quantile_plan(x, n, p, axis=0, win=None) -> dict:
    """Launch plan of ``quantile(x, n, p, axis, win)`` (bldp_quantile_plan_f32):
    the median's plan of that axis and shape (the keys of ``plan`` on axis 0, of
    ``tstat_plan`` on axis 2) with ``rank``, the 0-based lower rank j - 1 (-1 for
    the copy of n <= 1), in place of the workspace bytes."""
    p, axis = _quantile_args(p, axis)
    _window(x, win)
    w, keep = _win_args(x, win)
    return _axis_plan("bldp_quantile_plan_f32", (*w, axis, int(n), p, None), 8, axis, rank=True)


def band_quantile(banks, n, p, axis=0, win=None, out=None, stream=None):
    """``quantile`` of every bank of a band resident on ONE GPU, stitched in bank
    order in one launch (bldp_band_quantile_f32): a dense Float32 tensor laid out
    as ``band_reduce``'s (axis 0) or ``band_tstat``'s (axis 2)."""
    p, axis = _quantile_args(p, axis)
    banks, geo, out, ptrs, (keep, wp) = _band_args(banks, *_axis_factors(n, axis), win, out)
    _band_out_device(out, banks)
    rc = _lib.lib().bldp_band_quantile_f32(len(banks), ptrs, *geo, wp, axis, int(n), p, _ptr(out),
                                           _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_quantile_f32")
    return out


def quantile_host(a: np.ndarray, n, p, axis=0, win=None, device=0) -> np.ndarray:
    """Host Fortran-ordered Float32 array in, dense Float32 host array out
    (bldp_quantile_host_f32: the window's rows staged on ``device``)."""
    p, axis = _quantile_args(p, axis)
    a = _host_fb(a)
    shape, _ = _window(a, win)
    out = _host_out(out_shape(shape, win, *_axis_factors(n, axis)))
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_quantile_host_f32(*h, axis, int(n), p, _np_ptr(out))
    _lib.check(rc, "bldp_quantile_host_f32")
    return out


def planes_empty(nchan, nif, ntime, nplanes, device=None):
    """Uninitialised (nchan, nif, ntime, nplanes) Float32 tensor on the GPU whose
    every ``r[..., k]`` is laid out as ``fb_empty`` makes a product: the planes
    lie one after the other (the layout of ``quantiles``)."""
    torch = _torch()
    return torch.empty((int(nplanes), int(ntime), int(nif), int(nchan)), dtype=torch.float32,
                       device=device or "cuda").permute(3, 2, 1, 0)


def planes_to_numpy(t) -> np.ndarray:
    """A 4-D plane tensor (``planes_empty``'s axes) -> Fortran-ordered numpy array."""
    h = t.permute(3, 2, 1, 0).contiguous().cpu().numpy()
    return np.asfortranarray(h.transpose(3, 2, 1, 0))


def _quantiles_args(ps, axis):
    """(ps, axis) of a quantiles call, checked before any GPU work."""
    ps = _lib.quantiles(ps)[1]
    return ps, _quantile_args(0.0, axis)[1]


def _p_batches(ps):
    """ps in launches of <= _lib.MAX_QUANTILES: (first plane, ctypes double array)."""
    m = _lib.MAX_QUANTILES
    return [(k, (ctypes.c_double * len(ps[k:k + m]))(*ps[k:k + m])) for k in range(0, len(ps), m)]


def _planes_out(out, dims, K, device):
    """A caller's 4-D ``out`` of a quantiles call, checked before any launch: a
    Float32 (\\*dims, K) tensor on ``device`` whose planes are laid out as
    ``_tstat_out`` takes a product and do not overlap; returns (pointer, out_ld_i,
    out_ld_t, out_ld_q)."""
    if not isinstance(out, _torch().Tensor):
        raise TypeError("out must be a device tensor")
    if out.dim() != 4 or tuple(out.shape) != (*dims, K):
        raise ValueError(f"out is {tuple(out.shape)}, expected {(*dims, K)}")
    optr, ld_i, ld_t = _tstat_out(out[..., 0], dims, device)
    return optr, ld_i, ld_t, _plane_ld(out, dims, K, ld_i, ld_t)


def quantiles(x, n, ps, axis=0, win=None, out=None, stream=None):
    """``quantile`` for several probabilities at once (bldp_quantiles_f32): every
    block is read and its ranks selected once, and plane ``r[..., k]`` is bit for
    bit ``quantile(x, n, ps[k], axis, win)``.  ``ps``: any non-empty sequence,
    unsorted and repeats allowed; more than ``_lib.MAX_QUANTILES`` of them go in
    several launches into the one output.  Returns a (nc/n, ni, nt, K) or (nc,
    ni, nt/n, K) Float32 device tensor laid out plane after plane
    (``planes_empty``; ``out`` when given)."""
    ps, axis = _quantiles_args(ps, axis)
    shape, _ = _window(x, win)
    dims = out_shape(shape, win, *_axis_factors(n, axis))
    w, keep = _win_args(x, win)
    if out is None:
        out = planes_empty(*dims, len(ps), device=x.device)
    optr, ld_i, ld_t, ld_q = _planes_out(out, dims, len(ps), x.device)
    for k0, arr in _p_batches(ps):
        rc = _lib.lib().bldp_quantiles_f32(*w, axis, int(n), len(arr), arr,
                                           optr + 4 * k0 * ld_q if optr else None, ld_i, ld_t,
                                           ld_q, _lib.stream_ptr(stream))
        _lib.check(rc, "bldp_quantiles_f32")
    return out


def quantiles_plan(x, n, ps, axis=0, win=None) -> dict:
    """Launch plan of ``quantiles(x, n, ps, axis, win)`` (bldp_quantiles_plan_f32)
    for at most ``_lib.MAX_QUANTILES`` probabilities (one launch): the median's
    plan of that axis and shape (the keys of ``plan`` on axis 0, of ``tstat_plan``
    on axis 2, where the split form reports its own passes, workgroups and
    channel lanes) plus ``ranks``, the count of distinct ranks selected (0 for the
    copy of n <= 1), and ``reads``, how often the block is read."""
    ps, axis = _quantiles_args(ps, axis)
    _window(x, win)
    w, keep = _win_args(x, win)
    arr = (ctypes.c_double * len(ps))(*ps)
    return _axis_plan("bldp_quantiles_plan_f32", (*w, axis, int(n), len(ps), arr, None), 10, axis,
                      ("ranks", "reads"))


def band_quantiles(banks, n, ps, axis=0, win=None, out=None, stream=None):
    """``quantiles`` of every bank of a band resident on ONE GPU, stitched in bank
    order (bldp_band_quantiles_f32, one launch per <= ``_lib.MAX_QUANTILES``
    probabilities): a dense (nbank*nc', ni, nt', K) Float32 tensor whose plane k
    is ``band_quantile(banks, n, ps[k], axis, win)``."""
    ps, axis = _quantiles_args(ps, axis)
    K = len(ps)
    banks = _banks(banks, agree=False)[0]
    fq, tv = _axis_factors(n, axis)
    if out is None:
        shape, _ = _window(banks[0], win)
        nco, ni, nto = out_shape(shape, win, fq, tv)
        out = planes_empty(len(banks) * nco, ni, nto, K, device=banks[0].device)
    elif out.dim() != 4 or out.shape[3] != K:
        raise ValueError(f"out is {tuple(out.shape)}, expected {K} planes on a fourth axis")
    # (plane 0 is checked as band_quantile's out is)
    banks, geo, first, ptrs, (keep, wp) = _band_args(banks, fq, tv, win, out[..., 0])
    plane = first.numel()
    if K > 1 and plane and out.stride(3) != plane:
        raise ValueError("out must be dense: plane k at k * nbank*nco*ni*nto elements")
    _band_out_device(out, banks)
    for k0, arr in _p_batches(ps):
        rc = _lib.lib().bldp_band_quantiles_f32(len(banks), ptrs, *geo, wp, axis, int(n), len(arr),
                                                arr,
                                                out.data_ptr() + 4 * k0 * plane if plane else None,
                                                _lib.stream_ptr(stream))
        _lib.check(rc, "bldp_band_quantiles_f32")
    return out


def quantiles_host(a: np.ndarray, n, ps, axis=0, win=None, device=0) -> np.ndarray:
    """Host Fortran-ordered Float32 array in, Fortran-ordered (…, K) Float32 host
    array out (bldp_quantiles_host_f32: the window's rows staged on ``device``,
    once per <= ``_lib.MAX_QUANTILES`` probabilities)."""
    ps, axis = _quantiles_args(ps, axis)
    a = _host_fb(a)
    shape, _ = _window(a, win)
    dims = out_shape(shape, win, *_axis_factors(n, axis))
    out = _host_out((*dims, len(ps)))
    h, keep = _host_args(device, a, win)
    plane = dims[0] * dims[1] * dims[2]
    for k0, arr in _p_batches(ps):
        rc = _lib.lib().bldp_quantiles_host_f32(*h, axis, int(n), len(arr), arr,
                                                out.ctypes.data + 4 * k0 * plane if out.size
                                                else None)
        _lib.check(rc, "bldp_quantiles_host_f32")
    return out


# The outputs of an outliers call, in the ABI's order; ``mask`` is asked for by
# its own argument.
OUTLIER_PLANES = ("median", "mad", "count")


def _outliers_args(axis, nsigma, which):
    """(axis, nsigma, flags of OUTLIER_PLANES) of an outliers call, checked before
    any GPU work (ValueError)."""
    if axis not in (0, 2):
        raise ValueError(f"outliers: axis={axis!r} is not 0 (blocks of n channels) or 2 (blocks "
                         f"of n spectra)")
    try:
        ns = float(nsigma)
    except (TypeError, ValueError):
        raise ValueError(f"outliers: nsigma={nsigma!r} is not a number") from None
    if not (ns >= 0.0) or ns == float("inf"):
        raise ValueError(f"outliers: nsigma={nsigma!r} is not a finite number >= 0")
    if isinstance(which, str):
        which = (which,)
    which = tuple(which)
    for w in which:
        if w not in OUTLIER_PLANES:
            raise ValueError(f"outliers: unknown output {w!r}; which takes names from "
                             f"{OUTLIER_PLANES} (the mask: mask=True)")
    return int(axis), ns, tuple(w in which for w in OUTLIER_PLANES)


def _outliers_n(n, axis, nc, nt):
    """The block length: ``None`` on axis 2 is the whole selected time range."""
    if n is None:
        if axis != 2:
            raise ValueError("outliers: n=None (the whole selected time range) is for axis 2")
        n = nt
    n = int(n)
    if n < 2:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"outliers: n={n}: a block of fewer than 2 values has no scale")
    return n


def _outliers_outs(want, mask, dims, mdims, empty):
    """The outputs of an outliers call from ``empty(dims, dtype name)``: (the dict
    to return, the four in the ABI's order with None for those not asked for)."""
    outs = [empty(dims, dt) if w else None for w, dt in zip(want, ("float32", "float32", "int32"))]
    outs.append(empty(mdims, "uint8") if mask else None)
    res = {k: o for k, o in zip(OUTLIER_PLANES + ("mask",), outs) if o is not None}
    if not res:
        raise ValueError("outliers: no output asked for (which is empty and mask is False)")
    return res, outs


def _dev_empty(device):
    torch = _torch()
    return lambda dims, dt: fb_empty(*dims, device=device, dtype=getattr(torch, dt))


def outliers(x, n, axis=2, nsigma=5.0, win=None, mask=False, which=OUTLIER_PLANES, stream=None):
    """Median, mad, outlier count and outlier flags of every block of ``n``
    selected channels (``axis=0``) or spectra (``axis=2``; ``n=None``: the whole
    selected time range) from one launch (bldp_outliers_f32).  A sample is flagged
    when ``|x - median| > Float32(nsigma * mad)``, strictly, with ``mad`` the
    scaled median absolute deviation ``"mad"`` returns; a block whose median or
    mad is NaN flags nothing (the rule of include/bldp.h).  Returns a dict of
    device tensors: ``"median"`` and ``"mad"`` (Float32, bit for bit what the
    ``"median"`` and ``"mad"`` statistics give), ``"count"`` (int32) for the names
    in ``which``, each (nc/n, ni, nt) or (nc, ni, nt/n), and with ``mask=True``
    ``"mask"``, the uint8 (nc, ni, nt) flags of the window.  Float32 tensors only."""
    axis, ns, want = _outliers_args(axis, nsigma, which)
    if x.dtype != _torch().float32:
        _need_f32("outliers", x.dtype, "outliers")
    shape, (nc, ni, nt) = _window(x, win)
    n = _outliers_n(n, axis, nc, nt)
    dims = out_shape(shape, win, *_axis_factors(n, axis))
    w, keep = _win_args(x, win)
    res, outs = _outliers_outs(want, mask, dims, (nc, ni, nt), _dev_empty(x.device))
    rc = _lib.lib().bldp_outliers_f32(*w, axis, n, ns, *map(_ptr, outs), dims[0],
                                      dims[0] * dims[1], _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_outliers_f32")
    return res


def outliers_plan(x, n, axis=2, win=None, mask=False) -> dict:
    """Launch plan of ``outliers(x, n, axis, win=win, mask=mask)``
    (bldp_outliers_plan_f32): mad's plan of that axis and shape (the keys of
    ``plan`` on axis 0, of ``tstat_plan`` on axis 2) plus ``reads``, how often the
    block is read, and ``mask`` (1 when one is written)."""
    axis, _, _ = _outliers_args(axis, 0.0, ())
    _, (nc, ni, nt) = _window(x, win)
    n = _outliers_n(n, axis, nc, nt)
    w, keep = _win_args(x, win)
    return _axis_plan("bldp_outliers_plan_f32", (*w, axis, n, 1 if mask else 0), 10, axis,
                      ("reads", "mask"))


def band_outliers(banks, n, axis=2, nsigma=5.0, win=None, mask=False, which=OUTLIER_PLANES,
                  stream=None):
    """``outliers`` of every bank of a band resident on ONE GPU, stitched in bank
    order in one launch (bldp_band_outliers_f32): the dict of ``outliers`` with
    dense (nbank*nc', ni, nt') planes and a (nbank*nc, ni, nt) mask, the vcat of
    the banks' results."""
    axis, ns, want = _outliers_args(axis, nsigma, which)
    banks = _banks(banks, "band_outliers", "outliers", agree=False)[0]
    _, (nc, ni, nt) = _window(banks[0], win)
    n = _outliers_n(n, axis, nc, nt)
    banks, geo, first, ptrs, (keep, wp) = _band_args(banks, *_axis_factors(n, axis), win, None)
    nb = len(banks)
    res, outs = _outliers_outs(want, mask, tuple(first.shape), (nb * nc, ni, nt),
                               _dev_empty(first.device))
    rc = _lib.lib().bldp_band_outliers_f32(nb, ptrs, *geo, wp, axis, n, ns, *map(_ptr, outs),
                                           _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_outliers_f32")
    return res


def outliers_host(a: np.ndarray, n, axis=2, nsigma=5.0, win=None, mask=False,
                  which=OUTLIER_PLANES, device=0) -> dict:
    """Host Fortran-ordered Float32 array in, the dict of ``outliers`` as
    Fortran-ordered host arrays out (bldp_outliers_host_f32: the window's rows
    staged on ``device`` once).  Float32 arrays only."""
    axis, ns, want = _outliers_args(axis, nsigma, which)
    a = _host_fb(a, "outliers_host", "outliers")
    shape, (nc, ni, nt) = _window(a, win)
    n = _outliers_n(n, axis, nc, nt)
    dims = out_shape(shape, win, *_axis_factors(n, axis))
    res, outs = _outliers_outs(want, mask, dims, (nc, ni, nt), _host_out)
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_outliers_host_f32(*h, axis, n, ns, *map(_np_ptr, outs))
    _lib.check(rc, "bldp_outliers_host_f32")
    return res


def _argext_op(op) -> int:
    if op not in _lib.ARG_OPS:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"argext takes {sorted(_lib.ARG_OPS)}, not {op!r}")
    return _lib.ARG_OPS[op]


def _argext_out(out, dims, device, values):
    """The outputs of an argext, checked before any launch: ``out`` is None
    (new dense tensors), the int32 index tensor, or with ``values`` the pair
    (idx, val) with val Float32; each a (nco, ni, nto) tensor on ``device``
    with the channels fastest and rows that do not overlap, both of one layout
    (the ABI takes one pair of strides).  Returns (idx, val or None, idx
    pointer, val pointer, out_ld_i, out_ld_t)."""
    torch = _torch()
    if out is None:
        idx = fb_empty(*dims, device=device, dtype=torch.int32)
        val = fb_empty(*dims, device=device) if values else None
    elif values:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be the pair (idx, val) when values=True")
        idx, val = out
    else:
        idx, val = out, None
    iptr, *ld = _out_layout(idx, dims, device, torch.int32, "idx")
    vptr = None
    if val is not None:
        vptr, *vld = _out_layout(val, dims, device, torch.float32, "val")
        if vld != ld:
            raise ValueError(f"idx and val must share one layout, not strides {idx.stride()} and "
                             f"{val.stride()}")
    return idx, val, iptr, vptr, ld[0], ld[1]


def argext(x, fqavby, tavby, op, win=None, values=False, out=None, stream=None):
    """"argmax" / "argmin" of every fqavby x tavby block of the window, on the
    GPU (bldp_argext_f32): where in its block the extreme lies, as the 0-based
    offset ``k + fqavby * tt`` (k along the block's channels, tt along its
    spectra: Julia's column-major order), Julia's rule: the first of the
    isless-greatest (least) elements, and the first NaN when the block holds
    one.  x: a Float32 device filterbank tensor; returns a Julia-order
    (nc/F, ni, nt/T) int32 device tensor, or with ``values`` the pair
    (idx, val), val holding the winners' bits (Float32).  ``out``: the idx
    tensor (the pair with ``values``) to write, e.g. a bank's slot of a
    stitched product."""
    code = _argext_op(op)
    shape, _ = _window(x, win)
    dims = out_shape(shape, win, fqavby, tavby)
    w, keep = _win_args(x, win)
    idx, val, iptr, vptr, ld_i, ld_t = _argext_out(out, dims, x.device, values)
    rc = _lib.lib().bldp_argext_f32(*w, int(fqavby), int(tavby), code, iptr, vptr, ld_i, ld_t,
                                    _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_argext_f32")
    return (idx, val) if values else idx


def argext_plan(x, fqavby, tavby, op, win=None) -> dict:
    """Launch plan of ``argext(x, fqavby, tavby, op, win)``
    (bldp_argext_plan_f32): the path (_lib.ARGEXT_PATHS), the lanes sharing a
    block (256: a workgroup), the time slices of a workgroup splitting a
    block's rows, float4 loads per lane per row, workgroups, workspace bytes,
    outputs and whether the loads are float4."""
    code = _argext_op(op)
    _window(x, win)
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_argext_plan_f32", (*w, int(fqavby), int(tavby), code, None), 8,
                      ARGEXT_PLAN_KEYS, path=_lib.ARGEXT_PATHS)


def band_argext(banks, fqavby, tavby, op, win=None, values=False, stream=None):
    """``argext`` of every bank of a band resident on ONE GPU in one launch
    (bldp_band_argext_f32): dense (nbank*nco, ni, nto) tensors, the vcat of the
    per-bank results (offsets are relative to each block, so stitching is
    concatenation)."""
    code = _argext_op(op)
    torch = _torch()
    banks, nb, ptrs, geo = _banks(banks, devices=True)
    shape, _ = _window(banks[0], win)
    nco, ni, nto = out_shape(shape, win, fqavby, tavby)
    idx = fb_empty(nb * nco, ni, nto, device=banks[0].device, dtype=torch.int32)
    val = fb_empty(nb * nco, ni, nto, device=banks[0].device) if values else None
    keep, wp = _win_ptr(win, shape)
    rc = _lib.lib().bldp_band_argext_f32(nb, ptrs, *geo, wp, int(fqavby), int(tavby), code,
                                         _ptr(idx), _ptr(val), _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_argext_f32")
    return (idx, val) if values else idx


def argext_host(a: np.ndarray, fqavby, tavby, op, win=None, values=False, device=0):
    """Host Fortran-ordered Float32 array in, (nco, ni, nto) int32 host array of
    offsets out, with ``values`` the pair (idx, val)
    (bldp_argext_host_f32: the window's rows staged on ``device``)."""
    code = _argext_op(op)
    a = _host_fb(a)
    shape, _ = _window(a, win)
    dims = out_shape(shape, win, fqavby, tavby)
    idx = _host_out(dims, np.int32)
    val = _host_out(dims) if values else None
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_argext_host_f32(*h, int(fqavby), int(tavby), code, _np_ptr(idx),
                                         _np_ptr(val))
    _lib.check(rc, "bldp_argext_host_f32")
    return (idx, val) if values else idx


MASKED_OPS = ("sum", "mean")


def _masked_op(op) -> int:
    if op not in MASKED_OPS:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"masked reduce takes {MASKED_OPS}, not {op!r}")
    return _lib.OPS[op]


def _mask_strides(shape, strides, wshape, what):
    """mask_ld of a 3-D mask over a ``wshape`` window: an axis of length 1 is a
    broadcast (stride 0); any other length must be the window's (ValueError)."""
    if len(shape) != 3:
        raise ValueError(f"{what}: the mask is {len(shape)}-D, expected the 3-D window "
                         f"{tuple(wshape)} (an axis may be 1: a broadcast)")
    ld = []
    for ax in range(3):
        if shape[ax] == 1:
            ld.append(0)
        elif shape[ax] == wshape[ax]:
            ld.append(int(strides[ax]))
        else:
            raise ValueError(f"{what}: mask shape {tuple(shape)} does not broadcast to the window "
                             f"{tuple(wshape)}")
    return ld


def _mask_arg(mask, wshape, device, what):
    """(pointer, mask_ld array) of a device mask, checked before any GPU work:
    a uint8 or bool tensor (TypeError) that broadcasts to ``wshape`` (ValueError).
    A strided view passes its strides."""
    torch = _torch()
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"{what}: the mask must be a uint8 or bool device tensor, not "
                        f"{getattr(mask, 'dtype', type(mask).__name__)}")
    ld = _mask_strides(tuple(mask.shape), mask.stride(), wshape, what)
    if not mask.is_cuda:
        raise TypeError(f"{what}: the mask must be a device tensor (masked_reduce_host takes "
                        f"host arrays)")
    if mask.device != torch.device(device):
        raise ValueError(f"{what}: the mask is on {mask.device}, the data on {device}")
    return _ptr(mask), (ctypes.c_int64 * 3)(*ld)


def _host_mask(mask, what):
    """A host mask: a uint8 or bool array (TypeError); one with a negative stride
    is copied to Fortran order.  ``_host_mask_arg`` gives what the ABI takes."""
    m = np.asarray(mask)
    if m.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError(f"{what}: the mask must be a uint8 or bool array, not {m.dtype}")
    if m.ndim == 3 and any(s < 0 for s in m.strides):
        m = np.asfortranarray(m)
    return m


def _host_mask_arg(m, wshape, what):
    """(pointer, mask_ld array) of a ``_host_mask`` that broadcasts to ``wshape``."""
    return _np_ptr(m), (ctypes.c_int64 * 3)(*_mask_strides(m.shape, m.strides, wshape, what))


def _data_kept(dims, device, data=None):
    """The result of a masked reduce or a fold: Float32 ``"data"`` and the int32
    weights ``"kept"``, Julia-order device tensors of ``dims``."""
    return {"data": fb_empty(*dims, device=device) if data is None else data,
            "kept": fb_empty(*dims, device=device, dtype=_torch().int32)}


def masked_reduce(x, mask, fqavby=1, tavby=1, op="sum", win=None, stream=None):
    """``"sum"`` or ``"mean"`` of the unflagged samples of every fqavby x tavby
    block of the window, and how many there were, from one read of the window and
    one of the mask (bldp_masked_reduce_f32; the rule of include/bldp.h).  x: a
    Float32 device filterbank tensor; ``mask``: a uint8 or bool device tensor of
    the window's shape (nc, ni, nt), any axis of which may be 1 (a broadcast: a
    bad-channel list is (nc, 1, 1)); a byte of 0 keeps the sample, any other
    value drops it.  ``engine.outliers(..., mask=True)["mask"]`` goes in as it
    is; a strided view passes its strides.  Returns a dict of Julia-order
    (nc/F, ni, nt/T) device tensors: ``"data"`` (Float32; 0.0 for the sum and NaN
    for the mean of a block with nothing kept) and ``"kept"`` (int32), the weight
    of each product."""
    code = _masked_op(op)
    if x.dtype != _torch().float32:
        _need_f32("masked_reduce", x.dtype, "masked_reduce")
    shape, wshape = _window(x, win)
    mptr, ld = _mask_arg(mask, wshape, x.device, "masked_reduce")
    dims = out_shape(shape, win, fqavby, tavby)
    w, keep = _win_args(x, win)
    res = _data_kept(dims, x.device)
    rc = _lib.lib().bldp_masked_reduce_f32(*w, int(fqavby), int(tavby), code, mptr, ld,
                                           _ptr(res["data"]), _ptr(res["kept"]), dims[0],
                                           dims[0] * dims[1], _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_masked_reduce_f32")
    return res


def masked_reduce_plan(x, mask, fqavby=1, tavby=1, win=None) -> dict:
    """Launch plan of ``masked_reduce(x, mask, fqavby, tavby, win=win)``
    (bldp_masked_reduce_plan_f32): the keys of ``argext_plan`` (the walk is
    argext's) and ``mask_loads``, how the flags are read (_lib.MASK_LOADS:
    "byte" per element, one "dword" per float4, one byte per "row")."""
    _, wshape = _window(x, win)
    mptr, ld = _mask_arg(mask, wshape, x.device, "masked_reduce_plan")
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_masked_reduce_plan_f32", (*w, int(fqavby), int(tavby), mptr, ld), 10,
                      ARGEXT_PLAN_KEYS + ("mask_loads",), path=_lib.ARGEXT_PATHS,
                      mask_loads=_lib.MASK_LOADS)


def band_masked_reduce(banks, mask, fqavby=1, tavby=1, op="sum", win=None, stream=None):
    """``masked_reduce`` of every bank of a band resident on ONE GPU in one
    launch (bldp_band_masked_reduce_f32): the dict of ``masked_reduce`` with dense
    (nbank*nco, ni, nto) tensors, the vcat of the per-bank results.  ``mask``
    covers the stitched window, (nbank*nc, ni, nt) with any axis allowed to be 1:
    bank b's channel c is its channel b*nc + c (``band_outliers``' mask as it
    is)."""
    code = _masked_op(op)
    banks, nb, _, _ = _banks(banks, "band_masked_reduce", "masked_reduce", agree=False)
    _, (nc, ni, nt) = _window(banks[0], win)
    mptr, ld = _mask_arg(mask, (nb * nc, ni, nt), banks[0].device, "band_masked_reduce")
    banks, geo, data, ptrs, (keep, wp) = _band_args(banks, fqavby, tavby, win, None)
    res = _data_kept(tuple(data.shape), data.device, data)
    rc = _lib.lib().bldp_band_masked_reduce_f32(nb, ptrs, *geo, wp, int(fqavby), int(tavby), code,
                                                mptr, ld, _ptr(data), _ptr(res["kept"]),
                                                _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_masked_reduce_f32")
    return res


def masked_reduce_host(a: np.ndarray, mask: np.ndarray, fqavby=1, tavby=1, op="sum", win=None,
                       device=0) -> dict:
    """Host Fortran-ordered Float32 array and host uint8 / bool mask in (the
    window's shape, any axis allowed to be 1), the dict of ``masked_reduce`` as
    Fortran-ordered host arrays out (bldp_masked_reduce_host_f32: the window's
    rows and the mask staged on ``device`` once)."""
    code = _masked_op(op)
    a = _host_fb(a, "masked_reduce_host", "masked_reduce")
    m = _host_mask(mask, "masked_reduce_host")
    shape, wshape = _window(a, win)
    mptr, ld = _host_mask_arg(m, wshape, "masked_reduce_host")
    dims = out_shape(shape, win, fqavby, tavby)
    res = {"data": _host_out(dims), "kept": _host_out(dims, np.int32)}
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_masked_reduce_host_f32(*h, int(fqavby), int(tavby), code, mptr, ld,
                                                _np_ptr(res["data"]), _np_ptr(res["kept"]))
    _lib.check(rc, "bldp_masked_reduce_host_f32")
    return res


def _hits_cap(maxhits):
    """``maxhits`` as the ABI's cap: None stays None (all), else an int >= 0
    (TypeError for anything that is no integer, ValueError below 0)."""
    if maxhits is None:
        return None
    if isinstance(maxhits, bool) or not isinstance(maxhits, (int, np.integer)):
        raise TypeError(f"hits: maxhits must be an integer or None, not {type(maxhits).__name__}")
    if maxhits < 0:
        raise ValueError(f"hits: maxhits={maxhits} is negative")
    return int(maxhits)


def _hits_stream(stream, device):
    """The torch stream a hits call queues its launches on: ``stream`` (a raw
    hipStream_t is wrapped), or torch's current stream."""
    torch = _torch()
    if stream is None:
        return torch.cuda.current_stream()
    if isinstance(stream, int):
        return torch.cuda.ExternalStream(stream, device=device)
    return stream


def _hits_lists(fn, head, cap, device, stream):
    """The dict of ``hits`` from ``fn(*head, cap, idx, val, total, stream)``, the
    library call made with those device tensors (None: a null pointer) on
    ``stream``.  ``total`` and the lists are made under that stream, and the
    stream is synchronised before every read of ``total``: torch streams do not
    wait for one another, so a read on any other stream could come before the
    scan's store."""
    torch = _torch()
    s = _hits_stream(stream, device)
    outer = torch.cuda.current_stream()

    def call(c, idx, val, total):
        rc = getattr(_lib.lib(), fn)(*head, c, _ptr(idx), _ptr(val), total.data_ptr(),
                                     _lib.stream_ptr(stream))
        _lib.check(rc, fn)

    with torch.cuda.stream(s):
        total = torch.empty(1, dtype=torch.int64, device=device)
        if cap is None:  # count, then list exactly
            call(0, None, None, total)
            s.synchronize()
            cap = int(total.item())
        idx = torch.empty(cap, dtype=torch.int64, device=device)
        val = torch.empty(cap, dtype=torch.float32, device=device)
        call(cap, idx, val, total)
        s.synchronize()
        n = int(total.item())
    if outer != s:  # the caller goes on using the lists on its own stream
        idx.record_stream(outer)
        val.record_stream(outer)
    return {"total": n, "index": idx[:min(n, cap)], "value": val[:min(n, cap)]}


def hits(x, mask, maxhits=None, win=None, stream=None):
    """The flagged samples of the window as an ordered list, Julia's
    ``findall(!iszero, mask)`` and ``A[mask]`` on the device (bldp_hits_f32; the
    rule of include/bldp.h).  x: a Float32 device filterbank tensor; ``mask``: a
    uint8 or bool device tensor of the window's shape (nc, ni, nt), any axis of
    which may be 1 (a broadcast), as ``masked_reduce`` takes it; a byte that is
    not 0 flags the sample.  Returns a dict: ``"total"`` (a Python int), the
    number of flagged samples, always exact; ``"index"`` (int64, 0-based), their
    linear window indices k = c + nc*(i + ni*t) in ascending order
    (``hits_unravel`` gives channel, IF and time); ``"value"`` (float32), those
    samples, bits untouched.  With a number, ``maxhits`` needs one call: the
    lists are allocated at ``maxhits`` and returned cut to min(total, maxhits),
    the first in that order.  ``maxhits=None`` means all: a count-only call, a
    read of ``total``, an exact allocation and a second call, so the mask is
    counted twice.  Either way ``total`` is read back: the call synchronises
    ``stream`` (default: torch's current stream), on which the launches are
    queued and under which the lists are allocated."""
    cap = _hits_cap(maxhits)
    if x.dtype != _torch().float32:
        _need_f32("hits", x.dtype, "hits")
    _, wshape = _window(x, win)
    mptr, ld = _mask_arg(mask, wshape, x.device, "hits")
    w, keep = _win_args(x, win)
    return _hits_lists("bldp_hits_f32", (*w, mptr, ld), cap, x.device, stream)


HITS_PLAN_KEYS = ("mask_loads", "tile_elems", "tiles", "workspace_bytes", "scan_chunks",
                  "flags_per_load", "launches")


def hits_plan(x, mask, maxhits=None, win=None) -> dict:
    """Launch plan of ``hits(x, mask, maxhits, win=win)`` (bldp_hits_plan_f32):
    ``mask_loads`` (_lib.HITS_LOADS: "byte" per element, "wide" loads of
    ``flags_per_load`` = 4 or 16 flags a lane, one byte per "row"), ``tile_elems``
    and ``tiles`` (one workgroup each), ``workspace_bytes``, ``scan_chunks`` (the
    passes of the one scan workgroup) and ``launches`` (2 for ``maxhits=0``, the
    count-only call, else 3)."""
    cap = _hits_cap(maxhits)
    _, wshape = _window(x, win)
    mptr, ld = _mask_arg(mask, wshape, x.device, "hits_plan")
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_hits_plan_f32", (*w, mptr, ld, 1 if cap is None else cap), 10,
                      HITS_PLAN_KEYS, mask_loads=_lib.HITS_LOADS)


def band_hits(banks, mask, maxhits=None, win=None, stream=None):
    """``hits`` of a band resident on ONE GPU (bldp_band_hits_f32): the window is
    the vcat (nbank*nc, ni, nt) of the banks' windows and ``mask`` covers it, any
    axis allowed to be 1: bank b's channel c is channel b*nc + c of the mask and
    of the linear index (``band_outliers``' mask as it is), so within one (IF,
    time) row all of bank 0 comes before bank 1."""
    cap = _hits_cap(maxhits)
    banks, nb, _, _ = _banks(banks, "band_hits", "hits", agree=False)
    shape, (nc, ni, nt) = _window(banks[0], win)
    mptr, ld = _mask_arg(mask, (nb * nc, ni, nt), banks[0].device, "band_hits")
    _, _, ptrs, geo = _banks(banks)
    keep, wp = _win_ptr(win, shape)
    return _hits_lists("bldp_band_hits_f32", (nb, ptrs, *geo, wp, mptr, ld), cap,
                       banks[0].device, stream)


def hits_host(a: np.ndarray, mask: np.ndarray, maxhits=None, win=None, device=0) -> dict:
    """Host Fortran-ordered Float32 array and host uint8 / bool mask in (the
    window's shape, any axis allowed to be 1), the dict of ``hits`` with host
    arrays out (bldp_hits_host_f32: the window's rows and the mask staged on
    ``device`` once; the mask is counted twice there)."""
    cap = _hits_cap(maxhits)
    a = _host_fb(a, "hits_host", "hits")
    m = _host_mask(mask, "hits_host")
    _, wshape = _window(a, win)
    mptr, ld = _host_mask_arg(m, wshape, "hits_host")
    h, keep = _host_args(device, a, win)
    total = ctypes.c_uint64(0)

    def call(c, idx, val):
        rc = _lib.lib().bldp_hits_host_f32(*h, mptr, ld, c, _np_ptr(idx), _np_ptr(val),
                                           ctypes.byref(total))
        _lib.check(rc, "bldp_hits_host_f32")

    if cap is None:
        call(0, None, None)
        cap = int(total.value)
    idx = np.empty(cap, dtype=np.int64)
    val = np.empty(cap, dtype=np.float32)
    call(cap, idx, val)
    n = min(int(total.value), cap)
    return {"total": int(total.value), "index": idx[:n], "value": val[:n]}


def hits_unravel(index, wshape):
    """(channel, if, time), 0-based, of the linear window indices of ``hits`` over
    a window of shape ``wshape`` = (nc, ni, nt): k = c + nc*(i + ni*t).  Works on
    NumPy arrays and device tensors alike."""
    nc, ni, _ = (int(v) for v in wshape)
    if nc <= 0 or ni <= 0:
        raise ValueError(f"hits_unravel: empty window shape {tuple(wshape)}")
    q = index // nc
    return index - q * nc, q - (q // ni) * ni, q // ni


def hits_snr(value, median, mad):
    """The signed robust SNR of listed samples: (Float64(value) - Float64(median))
    / Float64(mad), with ``median`` and ``mad`` those of each sample's block."""
    if isinstance(value, np.ndarray):
        with np.errstate(invalid="ignore", divide="ignore"):
            return (value.astype(np.float64) - median.astype(np.float64)) / mad.astype(np.float64)
    return (value.double() - median.double()) / mad.double()


def _hist_args(nbins, lo, hi):
    """(nbins, lo, hi) of a histogram call, checked before any GPU work: the
    parameter conditions of include/bldp.h, each an ArgumentError (BLDP_EINVAL,
    as the library itself answers)."""
    try:
        B = int(nbins)
        ok = B == nbins
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise TypeError(f"histogram: nbins must be an integer, not {nbins!r}")
    if not 1 <= B <= _lib.MAX_HIST_BINS:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"histogram: nbins={B} outside 1..{_lib.MAX_HIST_BINS}")
    lo, hi = float(lo), float(hi)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lo32, hi32 = np.float32(lo), np.float32(hi)
        if not (np.isfinite(lo32) and np.isfinite(hi32) and lo32 < hi32):
            raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                     f"histogram: Float32(lo)={lo32} and Float32(hi)={hi32} must be "
                                     f"finite with lo < hi")
        w = np.float32(hi32 - lo32)
        s = np.float32(np.float32(B) / w)
    if not np.isfinite(w) or not np.isfinite(s) or not s > 0:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"histogram: hi - lo = {w} or the bin scale nbins / (hi - lo) = {s} "
                                 f"is not a finite positive Float32")
    return B, lo, hi


def hist_edges(nbins, lo, hi) -> np.ndarray:
    """The nbins + 1 Float64 bin edges ``lo32 + k * (hi32 - lo32) / nbins`` of a
    histogram: a reading aid only, the rule of include/bldp.h decides where a
    sample goes."""
    B, lo, hi = _hist_args(nbins, lo, hi)
    lo32, hi32 = float(np.float32(lo)), float(np.float32(hi))
    return lo32 + np.arange(B + 1, dtype=np.float64) * (hi32 - lo32) / B


def _hist_factors(shape, win, fqavby, tavby):
    """fqavby / tavby with None meaning the whole selected range of that axis."""
    nc, _, nt = window_shape(win, shape)
    return (max(nc, 1) if fqavby is None else fqavby), (max(nt, 1) if tavby is None else tavby)


def _hist_out(out, dims, K, device):
    """A caller's 4-D ``out`` of a histogram, checked before any launch: an int32
    (\\*dims, K) tensor on ``device`` whose planes are laid out as ``planes_empty``
    lays them (channels fastest) and do not overlap; returns (pointer, out_ld_i,
    out_ld_t, out_ld_q) (``_planes_out`` for counts)."""
    return _out_layout(out, dims, device, _torch().int32, dtname="int32", planes=K)


def hist_empty(nchan, nif, ntime, nplanes, device=None):
    """``planes_empty`` for counts: an uninitialised int32 (nchan, nif, ntime,
    nplanes) device tensor, plane after plane."""
    torch = _torch()
    return torch.empty((int(nplanes), int(ntime), int(nif), int(nchan)), dtype=torch.int32,
                       device=device or "cuda").permute(3, 2, 1, 0)


def histogram(x, nbins, lo, hi, fqavby=1, tavby=None, win=None, out=None, stream=None):
    """Sample counts per bin of every fqavby x tavby block of the window
    (bldp_histogram_f32; the rule of include/bldp.h).  x: a Float32 device
    filterbank tensor; ``tavby=None``: the whole selected time range,
    ``fqavby=None``: the whole selected channel range.  Returns an int32
    (nc/F, ni, nt/T, nbins + 3) device tensor laid out plane after plane
    (``hist_empty``; ``out`` when given, whatever it held): planes 0 .. nbins-1
    are the bins of [lo, hi), plane nbins counts the samples below lo, nbins + 1
    those at or above hi, nbins + 2 the NaNs.  The planes of a block add up to
    F * T; counts are exact, so two calls give identical bits."""
    torch = _torch()
    B, lo, hi = _hist_args(nbins, lo, hi)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        _need_f32("histogram", getattr(x, "dtype", type(x).__name__), "histogram")
    shape, _ = _window(x, win)
    fqavby, tavby = _hist_factors(shape, win, fqavby, tavby)
    dims = out_shape(shape, win, fqavby, tavby)
    w, keep = _win_args(x, win)
    if out is None:
        out = hist_empty(*dims, B + 3, device=x.device)
    o = _hist_out(out, dims, B + 3, x.device)
    rc = _lib.lib().bldp_histogram_f32(*w, int(fqavby), int(tavby), B, lo, hi, *o,
                                       _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_histogram_f32")
    return out


HIST_PLAN_KEYS = ("path", "workgroups", "chunks_per_block", "blocks_per_workgroup", "lds_bytes",
                  "replicas", "workspace_bytes", "vector_loads", "channel_lanes",
                  "rows_per_chunk")


def histogram_plan(x, nbins, lo, hi, fqavby=1, tavby=None, win=None) -> dict:
    """Launch plan of ``histogram(x, nbins, lo, hi, fqavby, tavby, win=win)``
    (bldp_histogram_plan_f32; launches nothing): ``path`` (_lib.HIST_PATHS),
    ``workgroups`` per bank, ``chunks_per_block`` (the workgroups that share a
    block), ``blocks_per_workgroup``, ``lds_bytes``, ``replicas`` of a block's
    counters in LDS, ``workspace_bytes`` (0), ``vector_loads`` (1: float4),
    ``channel_lanes`` and ``rows_per_chunk``."""
    B, lo, hi = _hist_args(nbins, lo, hi)
    shape, _ = _window(x, win)
    fqavby, tavby = _hist_factors(shape, win, fqavby, tavby)
    out_shape(shape, win, fqavby, tavby)
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_histogram_plan_f32", (*w, int(fqavby), int(tavby), B, lo, hi), 10,
                      HIST_PLAN_KEYS, path=_lib.HIST_PATHS)


def band_histogram(banks, nbins, lo, hi, fqavby=1, tavby=None, win=None, out=None, stream=None):
    """``histogram`` of every bank of a band resident on ONE GPU in one launch
    (bldp_band_histogram_f32): a dense int32 (nbank*nco, ni, nto, nbins + 3)
    tensor, the vcat of the per-bank results."""
    B, lo, hi = _hist_args(nbins, lo, hi)
    banks = _banks(banks, "band_histogram", "histogram", agree=False)[0]
    shape, _ = _window(banks[0], win)
    fqavby, tavby = _hist_factors(shape, win, fqavby, tavby)
    banks, geo, first, ptrs, (keep, wp) = _band_args(banks, fqavby, tavby, win, None)
    dims = tuple(first.shape)
    if out is None:
        out = hist_empty(*dims, B + 3, device=banks[0].device)
    optr, ld_i, ld_t, ld_q = _hist_out(out, dims, B + 3, banks[0].device)
    plane = dims[0] * dims[1] * dims[2]
    if plane and (ld_i, ld_t, ld_q) != (dims[0], dims[0] * dims[1], plane):
        raise ValueError("out must be dense: plane q at q * nbank*nco*ni*nto elements")
    rc = _lib.lib().bldp_band_histogram_f32(len(banks), ptrs, *geo, wp, int(fqavby), int(tavby), B,
                                            lo, hi, optr, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_histogram_f32")
    return out


def histogram_host(a: np.ndarray, nbins, lo, hi, fqavby=1, tavby=None, win=None,
                   device=0) -> np.ndarray:
    """Host Fortran-ordered Float32 array in, Fortran-ordered int32 (nc/F, ni,
    nt/T, nbins + 3) host array out (bldp_histogram_host_f32: the window's rows
    staged on ``device`` once)."""
    B, lo, hi = _hist_args(nbins, lo, hi)
    a = _host_fb(a, "histogram_host", "histogram")
    shape, _ = _window(a, win)
    fqavby, tavby = _hist_factors(shape, win, fqavby, tavby)
    out = _host_out((*out_shape(shape, win, fqavby, tavby), B + 3), np.int32)
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_histogram_host_f32(*h, int(fqavby), int(tavby), B, lo, hi, _np_ptr(out))
    _lib.check(rc, "bldp_histogram_host_f32")
    return out


FOLD_PLAN_KEYS = ("path", "channel_lanes", "chunks_per_block", "workgroups", "workspace_bytes",
                  "launches", "mask_loads", "vector_loads", "outputs", "units_per_chunk")
UNFOLD_PLAN_KEYS = ("vector_loads", "workgroups", "elements_per_lane")


def _fold_factors(shape, win, nfpc, tavby):
    """(nfpc, T, (nfpc, ni, nto)) of a fold; ``tavby=None``: the whole selected time
    range.  nfpc < 1 is an ArgumentError, a factor that does not divide the window
    a DimensionMismatch, both before any GPU work."""
    nc, ni, nt = window_shape(win, shape)
    if nfpc is None or int(nfpc) < 1:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL, f"fold: nfpc={nfpc!r} is less than 1")
    nfpc = int(nfpc)
    T = max(nt, 1) if tavby is None else max(int(tavby), 1)
    if nc % nfpc:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: nfpc={nfpc} does not divide nchan={nc}")
    if nt % T:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: tavby={T} does not divide ntime={nt}")
    return nfpc, T, ((nfpc if nc else 0), ni, nt // T)


def _unfold_op(how) -> int:
    if how not in _lib.UNFOLD_OPS:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"unfold takes {tuple(_lib.UNFOLD_OPS)}, not {how!r}")
    return _lib.UNFOLD_OPS[how]


def _fold_mask(mask, wshape, device, what):
    """_mask_arg, with None for no mask: (None, None)."""
    if mask is None:
        return None, None
    return _mask_arg(mask, wshape, device, what)


def fold(x, nfpc, tavby=None, op="mean", mask=None, win=None, stream=None):
    """The profile of the window over its coarse channels (bldp_fold_f32; the rule
    of include/bldp.h): selected channel c has fine index c mod nfpc, and output
    (k, i, t') is the ``"sum"`` or ``"mean"`` of the samples of fine index k of
    every coarse channel and of the ``tavby`` spectra of time block t'
    (``tavby=None``: the whole selected time range), summed in Float64 and rounded
    once.  x: a Float32 device filterbank tensor.  ``mask``: None, or a uint8 / bool
    device tensor as ``masked_reduce`` takes it (the window's shape, any axis may be
    1; a byte of 0 keeps the sample).  Returns a dict of Julia-order (nfpc, ni, nto)
    device tensors: ``"data"`` (Float32; 0.0 for the sum and NaN for the mean where
    nothing is kept) and ``"kept"`` (int32).  Two calls give identical bits."""
    torch = _torch()
    code = _masked_op(op)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        _need_f32("fold", getattr(x, "dtype", type(x).__name__), "fold")
    shape, wshape = _window(x, win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    mptr, ld = _fold_mask(mask, wshape, x.device, "fold")
    w, keep = _win_args(x, win)
    res = _data_kept(dims, x.device)
    rc = _lib.lib().bldp_fold_f32(*w, nfpc, T, code, mptr, ld, _ptr(res["data"]),
                                  _ptr(res["kept"]), dims[0], dims[0] * dims[1],
                                  _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_fold_f32")
    return res


def fold_plan(x, nfpc, tavby=None, mask=None, win=None) -> dict:
    """Launch plan of ``fold(x, nfpc, tavby, mask=mask, win=win)``
    (bldp_fold_plan_f32; launches nothing): ``path`` (_lib.FOLD_PATHS),
    ``channel_lanes`` of a workgroup, ``chunks_per_block`` (the workgroups that
    share a block), ``workgroups``, ``workspace_bytes``, ``launches`` (2 with the
    merge), ``mask_loads`` (_lib.FOLD_MASK_LOADS), ``vector_loads`` (1: float4),
    ``outputs`` and ``units_per_chunk``."""
    shape, wshape = _window(x, win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    mptr, ld = _fold_mask(mask, wshape, x.device, "fold_plan")
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_fold_plan_f32", (*w, nfpc, T, mptr, ld), 10, FOLD_PLAN_KEYS,
                      path=_lib.FOLD_PATHS, mask_loads=_lib.FOLD_MASK_LOADS)


def band_fold(banks, nfpc, tavby=None, op="mean", mask=None, win=None, stream=None):
    """``fold`` of a band resident on ONE GPU (bldp_band_fold_f32): ONE (nfpc, ni,
    nto) profile over the coarse channels of every bank, not a vcat.  ``mask``
    covers the stitched window, (nbank*nc, ni, nt) with any axis allowed to be 1:
    bank b's channel c is its channel b*nc + c."""
    code = _masked_op(op)
    banks, nb, _, _ = _banks(banks, "band_fold", "fold", agree=False)
    shape, (nc, ni, nt) = _window(banks[0], win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    mptr, ld = _fold_mask(mask, (nb * nc, ni, nt), banks[0].device, "band_fold")
    _, _, ptrs, geo = _banks(banks)
    keep, wp = _win_ptr(win, shape)
    res = _data_kept(dims, banks[0].device)
    rc = _lib.lib().bldp_band_fold_f32(nb, ptrs, *geo, wp, nfpc, T, code, mptr, ld,
                                       _ptr(res["data"]), _ptr(res["kept"]),
                                       _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_fold_f32")
    return res


def fold_host(a: np.ndarray, nfpc, tavby=None, op="mean", mask=None, win=None, device=0) -> dict:
    """Host Fortran-ordered Float32 array and (or None) host uint8 / bool mask in,
    the dict of ``fold`` as Fortran-ordered host arrays out (bldp_fold_host_f32:
    the window's rows and the mask staged on ``device`` once)."""
    code = _masked_op(op)
    a = _host_fb(a, "fold_host", "fold")
    shape, wshape = _window(a, win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    mptr = ld = None
    if mask is not None:
        mptr, ld = _host_mask_arg(_host_mask(mask, "fold_host"), wshape, "fold_host")
    res = {"data": _host_out(dims), "kept": _host_out(dims, np.int32)}
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_fold_host_f32(*h, nfpc, T, code, mptr, ld, _np_ptr(res["data"]),
                                       _np_ptr(res["kept"]))
    _lib.check(rc, "bldp_fold_host_f32")
    return res


def _unfold_prof(prof, dims, device, what):
    """(pointer, prof_ld_i, prof_ld_t) of a Float32 device profile of shape ``dims``
    with the fine channels fastest; a strided view passes its strides."""
    torch = _torch()
    if not isinstance(prof, torch.Tensor) or prof.dtype != torch.float32:
        raise TypeError(f"{what}: the profile must be a Float32 device tensor, not "
                        f"{getattr(prof, 'dtype', type(prof).__name__)}")
    if tuple(prof.shape) != tuple(dims):
        raise ValueError(f"{what}: the profile is {tuple(prof.shape)}, expected {tuple(dims)}")
    if not prof.is_cuda:
        raise TypeError(f"{what}: the profile must be a device tensor (unfold_host takes host "
                        f"arrays)")
    if prof.device != torch.device(device):
        raise ValueError(f"{what}: the profile is on {prof.device}, the data on {device}")
    s0, s1, s2 = prof.stride()
    if (dims[0] > 1 and s0 != 1) or min(s1, s2) < 0:
        raise ValueError(f"{what}: profile strides {prof.stride()}: the fine channels must be "
                         f"the fastest axis")
    return _ptr(prof), (s1 if dims[1] > 1 else 0), (s2 if dims[2] > 1 else 0)


def _unfold_out(out, dims, device):
    """(pointer, out_ld_i, out_ld_t) of a caller's Float32 ``out`` of shape ``dims``,
    channels fastest; a strided view (a bank's slot of a stitched band) passes its
    strides."""
    return _out_layout(out, tuple(dims), device, _torch().float32, dtname="Float32", loose=True)


def unfold(x, prof, nfpc, tavby=None, how="divide", win=None, out=None, stream=None):
    """The window with a profile taken out (bldp_unfold_f32): element (c, i, t) is
    ``x[c, i, t] / prof[c mod nfpc, i, t div tavby]`` (``how="divide"``, one correctly
    rounded Float32 division) or the difference (``"subtract"``); bit for bit
    NumPy's Float32 ``/`` and ``-``.  ``prof``: a Float32 (nfpc, ni, nto) device
    tensor, ``fold``'s ``"data"`` as it is.  Returns a Float32 (nc, ni, nt) device
    tensor (``out`` when given: any channel-fastest view, such as a bank's slot of a
    stitched band; it may not overlap ``x``)."""
    torch = _torch()
    code = _unfold_op(how)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        _need_f32("unfold", getattr(x, "dtype", type(x).__name__), "unfold")
    shape, wshape = _window(x, win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    p = _unfold_prof(prof, dims, x.device, "unfold")
    w, keep = _win_args(x, win)
    if out is None:
        out = fb_empty(*wshape, device=x.device)
    o = _unfold_out(out, wshape, x.device)
    rc = _lib.lib().bldp_unfold_f32(*w, nfpc, T, code, *p, *o, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_unfold_f32")
    return out


def unfold_plan(x, nfpc, tavby=None, win=None, prof=None, out=None) -> dict:
    """Launch plan of ``unfold`` (bldp_unfold_plan_f32; launches nothing):
    ``vector_loads`` (1: float4), ``workgroups`` per bank, ``elements_per_lane``.
    Without ``prof`` / ``out`` dense, aligned ones are assumed."""
    shape, wshape = _window(x, win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    p = (None, dims[0], dims[0] * dims[1]) if prof is None else \
        _unfold_prof(prof, dims, x.device, "unfold_plan")
    o = (None, wshape[0], wshape[0] * wshape[1]) if out is None else \
        _unfold_out(out, wshape, x.device)
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_unfold_plan_f32", (*w, nfpc, T, *p, *o), 4, UNFOLD_PLAN_KEYS)


def band_unfold(banks, prof, nfpc, tavby=None, how="divide", win=None, stream=None):
    """``unfold`` of every bank of a band resident on ONE GPU in one launch
    (bldp_band_unfold_f32) with ONE profile (``band_fold``'s): the dense vcat
    (nbank*nc, ni, nt)."""
    code = _unfold_op(how)
    banks = _banks(banks, "band_unfold", "unfold", agree=False)[0]
    shape, _ = _window(banks[0], win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    p = _unfold_prof(prof, dims, banks[0].device, "band_unfold")
    banks, geo, out, ptrs, (keep, wp) = _band_args(banks, 1, 1, win, None)
    rc = _lib.lib().bldp_band_unfold_f32(len(banks), ptrs, *geo, wp, nfpc, T, code, *p, _ptr(out),
                                         _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_unfold_f32")
    return out


def unfold_host(a: np.ndarray, prof: np.ndarray, nfpc, tavby=None, how="divide", win=None,
                device=0) -> np.ndarray:
    """Host Fortran-ordered Float32 array and host Float32 (nfpc, ni, nto) profile
    in, the Fortran-ordered (nc, ni, nt) result out (bldp_unfold_host_f32: the
    window's rows and the profile staged on ``device`` once)."""
    code = _unfold_op(how)
    a = _host_fb(a, "unfold_host", "unfold")
    shape, wshape = _window(a, win)
    nfpc, T, dims = _fold_factors(shape, win, nfpc, tavby)
    p = np.asarray(prof)
    if p.dtype != np.float32:
        raise TypeError(f"unfold_host: the profile must be float32, not {p.dtype}")
    if p.shape != tuple(dims):
        raise ValueError(f"unfold_host: the profile is {p.shape}, expected {tuple(dims)}")
    p = np.asfortranarray(p)
    out = _host_out(wshape)
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_unfold_host_f32(*h, nfpc, T, code, _np_ptr(p), _np_ptr(out))
    _lib.check(rc, "bldp_unfold_host_f32")
    return out


DEDOPPLER_PLAN_KEYS = ("path", "tile_channels", "halo", "rows_per_chunk", "drifts_per_group",
                       "groups", "lds_bytes", "workgroups", "vector_loads", "workspace_bytes")
MAX_TAVBY_DEDOPPLER = 1 << 20


def drift_offsets(maxdrift, T) -> np.ndarray:
    """The paths of a dedoppler: the (2*maxdrift + 1, T) Int64 table off(d_k, t) =
    sign(d) * floor((2|d|t + (T-1)) / (2(T-1))), d_k = k - maxdrift: the straight
    line from 0 to d over the T spectra of a block, rounded to the nearest channel,
    halves away from zero."""
    D, T = int(maxdrift), int(T)
    if D < 0 or T < 2:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"drift_offsets: maxdrift={maxdrift!r} < 0 or T={T!r} < 2")
    d = np.arange(-D, D + 1, dtype=np.int64)[:, None]
    t = np.arange(T, dtype=np.int64)[None, :]
    return np.sign(d) * ((2 * np.abs(d) * t + (T - 1)) // (2 * (T - 1)))


def drift_rates(maxdrift, T, foff, tsamp) -> np.ndarray:
    """The drift rates, in Hz/s, of the 2*maxdrift + 1 drifts of a dedoppler over
    blocks of T spectra: d * foff * 1e6 / ((T - 1) * tsamp), with ``foff`` the
    channel width in MHz (its sign is the band's direction) and ``tsamp`` the
    spectrum spacing in seconds."""
    D, T = int(maxdrift), int(T)
    if D < 0 or T < 2:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"drift_rates: maxdrift={maxdrift!r} < 0 or T={T!r} < 2")
    d = np.arange(-D, D + 1, dtype=np.float64)
    return d * (float(foff) * 1e6) / ((T - 1) * float(tsamp))


def _dedop_args(shape, win, maxdrift, tavby, seg):
    """(D, T, seg, (nc, ni, nb)) of a dedoppler, with the library's refusals raised
    before any GPU work; ``tavby=None``: the whole selected time range, ``seg``
    None or 0: the whole window is one segment."""
    nc, ni, nt = window_shape(win, shape)
    if isinstance(maxdrift, bool) or int(maxdrift) != maxdrift or \
            not 0 <= int(maxdrift) <= _lib.MAX_DRIFT:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"dedoppler: maxdrift={maxdrift!r} outside 0..{_lib.MAX_DRIFT}")
    T = nt if tavby is None else int(tavby)
    if T < 2 or T > MAX_TAVBY_DEDOPPLER:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL,
                                 f"dedoppler: tavby={T} outside 2..2^20 (a block needs two spectra)")
    seg = 0 if seg is None else int(seg)
    if seg < 0:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL, f"dedoppler: seg={seg} is negative")
    if nt % T:
        raise _lib.DimensionMismatch(_lib.BLDP_EDIM,
                                     f"DimensionMismatch: tavby={T} does not divide ntime={nt}")
    return int(maxdrift), T, seg, (nc, ni, nt // T)


def _dedop_outs(dims, K, device, sums):
    """The outputs of a dedoppler and what the ABI takes for them: (result dict,
    best pointer, drift pointer, sums pointer, ld_i, ld_t, ld_q)."""
    torch = _torch()
    res = {"best": fb_empty(*dims, device=device),
           "drift": fb_empty(*dims, device=device, dtype=torch.int32)}
    _, ld_i, ld_t = _out_layout(res["best"], dims, device, torch.float32, name="best")
    sptr, ld_q = None, max(dims[0] * dims[1] * dims[2], 1)
    if sums:
        res["sums"] = planes_empty(*dims, K, device=device)
        sptr, _, _, ld_q = _out_layout(res["sums"], dims, device, torch.float32, name="sums",
                                       planes=K)
    return res, _ptr(res["best"]), _ptr(res["drift"]), sptr, ld_i, ld_t, ld_q


def dedoppler(x, maxdrift, tavby=None, seg=None, win=None, sums=False, stream=None):
    """The drift-rate sums of every channel of the window (bldp_dedoppler_f32; the
    rule of include/bldp.h): ``tavby`` spectra make a block (None: the whole
    selected time range), drift d in -maxdrift .. maxdrift moves ``drift_offsets``'
    off(d, t) selected channels at spectrum t of a block, and S[c, i, b, d] is the
    Float32 sum of the block's samples along that path, added in time order; a
    path takes no sample outside the segment of c (``seg`` channels each: the
    coarse channels; None: the whole window).  x: a Float32 device filterbank
    tensor.  Returns a dict of Julia-order device tensors: ``"best"`` (Float32,
    (nc, ni, nb)), the greatest sum of every channel, ``"drift"`` (int32), the d
    it belongs to (ties and a flat window give the drift nearest 0, the negative
    one first), and with ``sums`` also ``"sums"`` ((nc, ni, nb, 2*maxdrift + 1),
    plane d + maxdrift; laid out as ``planes_empty``).  ``sums`` is for zoom
    windows: it is (2*maxdrift + 1) / tavby times the input.  Two calls give
    identical bits."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        _need_f32("dedoppler", getattr(x, "dtype", type(x).__name__), "dedoppler")
    shape, _ = _window(x, win)
    D, T, seg, dims = _dedop_args(shape, win, maxdrift, tavby, seg)
    w, keep = _win_args(x, win)
    res, bptr, dptr, sptr, ld_i, ld_t, ld_q = _dedop_outs(dims, 2 * D + 1, x.device, sums)
    rc = _lib.lib().bldp_dedoppler_f32(*w, T, D, seg, bptr, dptr, sptr, ld_i, ld_t, ld_q,
                                       _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_dedoppler_f32")
    return res


def dedoppler_plan(x, maxdrift, tavby=None, seg=None, win=None) -> dict:
    """Launch plan of ``dedoppler(x, maxdrift, tavby, seg, win)``
    (bldp_dedoppler_plan_f32; launches nothing): ``path`` (_lib.DEDOPPLER_PATHS),
    ``tile_channels`` (the lanes of a workgroup), ``halo`` channels staged on each
    side, ``rows_per_chunk`` in LDS (resident: tavby), ``drifts_per_group`` a lane
    sums at a time, ``groups``, ``lds_bytes``, ``workgroups`` per bank,
    ``vector_loads`` (1: float4) and ``workspace_bytes`` (0)."""
    shape, _ = _window(x, win)
    D, T, seg, _ = _dedop_args(shape, win, maxdrift, tavby, seg)
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_dedoppler_plan_f32", (*w, T, D, seg), 10, DEDOPPLER_PLAN_KEYS,
                      path=_lib.DEDOPPLER_PATHS)


def band_dedoppler(banks, maxdrift, tavby=None, seg=None, win=None, sums=False, stream=None):
    """``dedoppler`` of every bank of a band resident on ONE GPU in one launch
    (bldp_band_dedoppler_f32): dense (nbank*nc, ni, nb[, K]) tensors, the vcat of
    the per-bank results.  Segments are counted from each bank's first selected
    channel, so no path crosses from one bank into the next."""
    banks, nb, ptrs, geo = _banks(banks, "band_dedoppler", "dedoppler", devices=True)
    shape, _ = _window(banks[0], win)
    D, T, seg, (nc, ni, nblk) = _dedop_args(shape, win, maxdrift, tavby, seg)
    keep, wp = _win_ptr(win, shape)
    res, bptr, dptr, sptr, _, _, _ = _dedop_outs((nb * nc, ni, nblk), 2 * D + 1, banks[0].device,
                                                 sums)
    rc = _lib.lib().bldp_band_dedoppler_f32(nb, ptrs, *geo, wp, T, D, seg, bptr, dptr, sptr,
                                            _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_dedoppler_f32")
    return res


def dedoppler_host(a: np.ndarray, maxdrift, tavby=None, seg=None, win=None, sums=False,
                   device=0) -> dict:
    """Host Fortran-ordered Float32 array in, the dict of ``dedoppler`` as
    Fortran-ordered host arrays out (bldp_dedoppler_host_f32: the window's rows
    staged on ``device`` once)."""
    a = _host_fb(a, "dedoppler_host", "dedoppler")
    shape, _ = _window(a, win)
    D, T, seg, dims = _dedop_args(shape, win, maxdrift, tavby, seg)
    res = {"best": _host_out(dims), "drift": _host_out(dims, np.int32)}
    if sums:
        res["sums"] = _host_out((*dims, 2 * D + 1))
    h, keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_dedoppler_host_f32(*h, T, D, seg, _np_ptr(res["best"]),
                                            _np_ptr(res["drift"]), _np_ptr(res.get("sums")))
    _lib.check(rc, "bldp_dedoppler_host_f32")
    return res


def stitch(gathered, nbank, out=None, stream=None):
    """gathered: nbank dense (nc, ni, nt) blocks back to back (1-D or a
    [nbank, nt, ni, nc] contiguous tensor); returns vcat (nbank*nc, ni, nt)."""
    L = _lib.lib()
    g = gathered
    if g.dim() == 4:
        nb, nt, ni, nc = g.shape
    else:
        raise ValueError("gathered must be a contiguous [nbank, ntime, nif, nc] tensor")
    if nb != nbank or not g.is_contiguous():
        raise ValueError("gathered must be a contiguous [nbank, ntime, nif, nc] tensor")
    if out is None:
        out = fb_empty(nbank * nc, ni, nt, device=g.device)
    rc = L.bldp_stitch_f32(nbank, g.data_ptr(), nc, ni, nt, out.data_ptr(),
                           _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_stitch_f32")
    return out


def despike(x, nfpc, stream=None):
    """In place: every coarse channel's DC bin takes its left neighbour's
    value (src/gbt.jl:101-102,111).  Returns x."""
    L = _lib.lib()
    ptr, nchan, nif, ntime = _abi_dims(x)
    if nchan != x.shape[0] or (x.shape[1] > 1 and nif != x.shape[1]):
        raise ValueError("despike needs a dense Julia-order tensor")
    rc = L.bldp_despike_f32(ptr, x.shape[0], x.shape[1], x.shape[2], int(nfpc),
                            _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_despike_f32")
    return x


def _check_tblock(tblock, nt) -> int:
    """Blocks of ``tblock`` selected spectra: the count nt / tblock, with the
    library's own errors (bldp_kurtosis_blocks_shape) raised before any launch."""
    if isinstance(tblock, bool) or int(tblock) != tblock:
        raise TypeError(f"tblock must be an integer, not {tblock!r}")
    M = int(tblock)
    if M < 1:
        raise _lib.ArgumentError(_lib.BLDP_EINVAL, f"tblock={M} must be >= 1")
    if nt % M:
        raise _lib.DimensionMismatch(
            _lib.BLDP_EDIM, f"DimensionMismatch: tblock={M} does not divide ntime={nt}")
    return nt // M


def _block_win(win, shape, M, b):
    """The window of block b: spectra [b*M, (b+1)*M) of the selected ones."""
    w = _full_win(win, shape)
    w[6] += b * M * w[8]
    w[7] = M
    return w


def _skew_tblock(tblock, nt) -> int:
    """The ABI's tblock of a skewness call: 0 = the whole window (``None``),
    else the checked block length (the errors of ``_check_tblock``)."""
    if tblock is None:
        return 0
    _check_tblock(tblock, nt)
    return int(tblock)


def _need_f32(what, dtype, fn="skewness"):
    raise TypeError(f"{what}: element type {dtype} is not supported; {fn} takes Float32 "
                    "(float32) data only")


# The time-moment family (kurtosis over blocks, skewness, moments) shares one
# helper per kind of call.  ``fn`` names the ABI function, ``want`` flags the
# planes to allocate (one for kurtosis and skewness, four for moments); each
# returns the planes in ``want``'s order, ``None`` where it is false.  The
# callers check ``which`` and the element type first, in that order.
def _moment_call(fn, x, win, tblock, stream, want=(True,)):
    """Device call: (nc, ni, nt/tblock) float64 tensors, (nc, ni) ones for the
    whole window (``tblock=None``)."""
    torch = _torch()
    _, (nc, ni, nt) = _window(x, win)
    M = _skew_tblock(tblock, nt)
    nb = nt // M if M else 1
    outs = [torch.empty((nb, ni, nc), dtype=torch.float64, device=x.device).permute(2, 1, 0)
            if w else None for w in want]
    w, keep = _win_args(x, win)
    rc = getattr(_lib.lib(), fn)(*w, M, *map(_ptr, outs), nc, nc * ni, _lib.stream_ptr(stream))
    _lib.check(rc, fn)
    return [o if o is None or M else o[:, :, 0] for o in outs]


def _moment_plan(fn, x, win, tblock, check=_skew_tblock) -> dict:
    """Plan call: the path ("regs", "mid", "leaf", "twopass"), fused, the block
    count and the workspace bytes."""
    _, wshape = _window(x, win)
    check(tblock, wshape[2])
    w, keep = _win_args(x, win)
    return _plan_dict(fn, (*w, int(tblock or 0)), 4,
                      ("path", "fused", "blocks", "workspace_bytes"), path=_lib.KURT_PATHS)


def _band_moment_call(fn, banks, win, tblock, stream, want=(True,)):
    """Band call: per bank the list of its planes, views of one buffer per
    plane."""
    torch = _torch()
    shape, (nc, ni, nt) = _window(banks[0], win)
    M = _skew_tblock(tblock, nt)
    nb = nt // M if M else 1
    banks, nbank, ptrs, geo = _banks(banks)
    keep, wp = _win_ptr(win, shape)
    bufs = [torch.empty((nbank, nb, ni, nc), dtype=torch.float64, device=banks[0].device)
            if w else None for w in want]
    rc = getattr(_lib.lib(), fn)(nbank, ptrs, *geo, wp, M, *map(_ptr, bufs),
                                 _lib.stream_ptr(stream))
    _lib.check(rc, fn)

    def view(buf, k):
        if buf is None:
            return None
        return buf[k].permute(2, 1, 0) if M else buf[k, 0].t()
    return [[view(buf, k) for buf in bufs] for k in range(nbank)]


def _moment_host(fn, a, win, device, tblock, want=(True,), what=None, takes="skewness"):
    """Host call: Fortran-ordered (nc, ni, nt/tblock) float64 arrays, (nc, ni)
    ones for the whole window.  ``what``: the caller's name in the TypeError of
    an element type other than Float32 (``takes`` names the statistic)."""
    a = _host_fb(a, what, takes)
    _, (nc, ni, nt) = _window(a, win)
    M = _skew_tblock(tblock, nt)
    outs = [np.empty((nc, ni, nt // M) if M else (nc, ni), dtype=np.float64, order="F")
            if w else None for w in want]
    h, keep = _host_args(device, a, win)
    # (bldp_kurtosis_host_f32, the whole-window kurtosis, takes no tblock)
    rc = getattr(_lib.lib(), fn)(*h, *(() if fn == "bldp_kurtosis_host_f32" else (M,)),
                                 *map(_np_ptr, outs))
    _lib.check(rc, fn)
    return outs


def kurtosis(x, win=None, tblock=None, stream=None):
    """Excess kurtosis over time per (channel, IF): (nc, ni) float64 tensor.

    ``tblock=M``: the kurtosis of every block of M selected spectra, a
    Julia-order (nc, ni, nt/M) float64 tensor (bldp_kurtosis_blocks_f32: one
    call; M must divide nt).  Element types other than Float32 go block by
    block through the typed kurtosis."""
    torch = _torch()
    if tblock is not None and x.dtype == torch.float32:
        return _moment_call("bldp_kurtosis_blocks_f32", x, win, tblock, stream)[0]
    L = _lib.lib()
    shape, (nc, ni, nt) = _window(x, win)
    if tblock is not None:
        nb = _check_tblock(tblock, nt)
        out = torch.empty((nb, ni, nc), dtype=torch.float64, device=x.device).permute(2, 1, 0)
        for b in range(nb):
            out[:, :, b] = kurtosis(x, _block_win(win, shape, int(tblock), b), stream=stream)
        return out
    out = torch.empty((ni, nc), dtype=torch.float64, device=x.device).t()
    w, keep = _win_args(x, win, allow_typed=True)
    if x.dtype != torch.float32:  # StatsBase in Float64 for integer / Float64 rows
        rc = L.bldp_kurtosis(_dtype_code(x.dtype), *w, _ptr(out), _lib.stream_ptr(stream))
        _lib.check(rc, "bldp_kurtosis")
        return out
    rc = L.bldp_kurtosis_f32(*w, _ptr(out), None, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_kurtosis_f32")
    return out


def kurtosis_plan(x, win=None) -> dict:
    """Kurtosis plan for this tensor and window: path ("regs", "mid", "leaf",
    "twopass"), K (level of the pairwise-sum blocks), leaf slots, workspace."""
    _window(x, win)
    w, keep = _win_args(x, win)
    return _plan_dict("bldp_kurtosis_plan_f32", w, 4, ("path", "K", "leaf_slots", "workspace_bytes"),
                      path=_lib.KURT_PATHS)


def kurtosis_blocks_plan(x, tblock, win=None) -> dict:
    """Plan of ``kurtosis(x, win, tblock)``: the path of the blocks ("regs",
    "mid", "leaf", "twopass": the class of the results), fused (1 = the
    one-launch kernel, 0 = block by block through the whole-window paths),
    the block count and the workspace bytes."""
    return _moment_plan("bldp_kurtosis_blocks_plan_f32", x, win, tblock, check=_check_tblock)


def band_kurtosis(banks, win=None, tblock=None, stream=None):
    """Kurtosis of every bank of a band on one GPU in one set of launches;
    returns a list of (nc, ni) float64 tensors (views of one buffer), or with
    ``tblock`` of (nc, ni, nt/tblock) ones (bldp_band_kurtosis_blocks_f32)."""
    torch = _torch()
    banks, nb, ptrs, geo = _banks(banks)
    shape, (nc, ni, nt) = _window(banks[0], win)
    if tblock is not None:
        return [v[0] for v in _band_moment_call("bldp_band_kurtosis_blocks_f32", banks, win,
                                                tblock, stream)]
    keep, wp = _win_ptr(win, shape)
    buf = torch.empty((nb, ni, nc), dtype=torch.float64, device=banks[0].device)
    rc = _lib.lib().bldp_band_kurtosis_f32(nb, ptrs, *geo, wp, _ptr(buf), _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_band_kurtosis_f32")
    return [buf[k].t() for k in range(nb)]


def kurtosis_host(a: np.ndarray, win=None, device=0, tblock=None) -> np.ndarray:
    """Host array in, (nc, ni) float64 host array out (bldp_kurtosis_host_f32);
    with ``tblock`` the (nc, ni, nt/tblock) kurtosis of every block of tblock
    selected spectra (bldp_kurtosis_blocks_host_f32)."""
    fn = "bldp_kurtosis_host_f32" if tblock is None else "bldp_kurtosis_blocks_host_f32"
    return _moment_host(fn, a, win, device, tblock)[0]


def skewness(x, win=None, tblock=None, stream=None):
    """Skewness over time per (channel, IF), StatsBase.skewness with Julia's
    Float32 mean (bldp_skewness_f32): an (nc, ni) float64 tensor, or with
    ``tblock=M`` the Julia-order (nc, ni, nt/M) skewness of every block of M
    selected spectra (M must divide nt).  Float32 tensors only."""
    if x.dtype != _torch().float32:
        _need_f32("skewness", x.dtype)
    return _moment_call("bldp_skewness_f32", x, win, tblock, stream)[0]


def skewness_plan(x, win=None, tblock=None) -> dict:
    """Plan of ``skewness(x, win, tblock)``: the path ("regs", "mid", "leaf",
    "twopass": the class of the results), fused (1 = one set of launches, 0 =
    block by block), the block count and the workspace bytes."""
    return _moment_plan("bldp_skewness_plan_f32", x, win, tblock)


def band_skewness(banks, win=None, tblock=None, stream=None):
    """Skewness of every bank of a band on one GPU in one set of launches
    (bldp_band_skewness_f32): a list of (nc, ni) float64 tensors (views of one
    buffer), or with ``tblock`` of (nc, ni, nt/tblock) ones."""
    banks = _banks(banks, "band_skewness", "skewness", agree=False)[0]
    return [v[0] for v in _band_moment_call("bldp_band_skewness_f32", banks, win, tblock, stream)]


def skewness_host(a: np.ndarray, win=None, device=0, tblock=None) -> np.ndarray:
    """Host array in, (nc, ni) float64 host array out (bldp_skewness_host_f32);
    with ``tblock`` the (nc, ni, nt/tblock) skewness of every block of tblock
    selected spectra.  Float32 arrays only."""
    return _moment_host("bldp_skewness_host_f32", a, win, device, tblock, what="skewness_host")[0]


# The planes of a moments call, in the ABI's order.  ``var`` is cm2 / n, the
# uncorrected variance both StatsBase recipes divide by (not Julia's var).
MOMENTS = ("mean", "var", "skewness", "kurtosis")
Moments = collections.namedtuple("Moments", MOMENTS)


def _which_planes(which) -> tuple:
    """The requested planes as four flags in ``MOMENTS`` order."""
    if isinstance(which, str):
        which = (which,)
    which = tuple(which)
    for w in which:
        if w not in MOMENTS:
            raise ValueError(f"moments: unknown plane {w!r}; which takes names from {MOMENTS}")
    if not which:
        raise ValueError(f"moments: which is empty; it takes names from {MOMENTS}")
    return tuple(name in which for name in MOMENTS)


def moments(x, win=None, tblock=None, stream=None, which=MOMENTS):
    """Mean, variance, skewness and kurtosis over time per (channel, IF) from
    one read of the window (bldp_moments_f32): a ``Moments`` named tuple of
    (nc, ni) float64 tensors, or with ``tblock=M`` of Julia-order (nc, ni,
    nt/M) ones, one value per block of M selected spectra (M must divide nt).
    ``skewness`` and ``kurtosis`` are what ``skewness()`` and ``kurtosis()``
    return, ``mean`` is Julia's Float32 mean widened, and ``var`` is cm2 / n,
    the UNCORRECTED variance those two divide by (not Julia's ``var``).  A
    plane not named in ``which`` is ``None`` and is not computed into memory.
    Float32 tensors only."""
    want = _which_planes(which)
    if x.dtype != _torch().float32:
        _need_f32("moments", x.dtype, "moments")
    return Moments(*_moment_call("bldp_moments_f32", x, win, tblock, stream, want))


def moments_plan(x, win=None, tblock=None) -> dict:
    """Plan of ``moments(x, win, tblock)``: the path ("regs", "mid", "leaf",
    "twopass": the class of the results), fused (1 = one set of launches, 0 =
    block by block), the block count and the workspace bytes."""
    return _moment_plan("bldp_moments_plan_f32", x, win, tblock)


def band_moments(banks, win=None, tblock=None, stream=None, which=MOMENTS):
    """The moments of every bank of a band on one GPU in one set of launches
    (bldp_band_moments_f32): a list of ``Moments`` (views of one buffer per
    plane), shaped as ``moments`` shapes them."""
    want = _which_planes(which)
    banks = _banks(banks, "band_moments", "moments", agree=False)[0]
    return [Moments(*v) for v in _band_moment_call("bldp_band_moments_f32", banks, win, tblock,
                                                    stream, want)]


def moments_host(a: np.ndarray, win=None, device=0, tblock=None, which=MOMENTS):
    """Host array in, a ``Moments`` of (nc, ni) float64 host arrays out
    (bldp_moments_host_f32), (nc, ni, nt/tblock) with ``tblock``; the window is
    staged on the device once.  Float32 arrays only."""
    want = _which_planes(which)
    return Moments(*_moment_host("bldp_moments_host_f32", a, win, device, tblock, want,
                                 "moments_host", "moments"))


def synth(nchan, nif, ntime, nfpc=1024, seed=0, kind=0, device=None, stream=None, out=None):
    """Synthetic BL-like filterbank generated on the GPU (bldp_synth_f32),
    into ``out`` (a dense Julia-order tensor, e.g. a band_empty view) if given."""
    L = _lib.lib()
    if out is None:
        out = fb_empty(nchan, nif, ntime, device=device)
    elif tuple(out.shape) != (nchan, nif, ntime) or (
            out.numel() and out.stride() != (1, nchan, nchan * nif)):
        raise ValueError("out must be a dense Julia-order (nchan, nif, ntime) tensor")
    rc = L.bldp_synth_f32(out.data_ptr() if out.numel() else None, nchan, nif, ntime, nfpc,
                          seed, kind, _lib.stream_ptr(stream))
    _lib.check(rc, "bldp_synth_f32")
    return out


def reduce_host_typed(a: np.ndarray, fqavby=1, tavby=1, op="sum", win=None, device=0) -> np.ndarray:
    """Host array of any supported element type in, host array of fqav's
    Julia result type out (bldp_reduce_host): e.g. UInt8 SIGPROC data summed
    into UInt64, averaged into Float64, max / min kept as UInt8."""
    a = np.asarray(a)
    _check_stat(op, tavby, a.dtype)
    code = _dtype_code(a.dtype)
    if code is None or a.ndim != 3:
        raise TypeError(f"unsupported host filterbank {a.dtype} {a.shape}")
    a = np.asfortranarray(a)
    shape, _ = _window(a, win)
    out = _host_out(out_shape(shape, win, fqavby, tavby), out_dtype(a.dtype, op))
    (dev, *h), keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_reduce_host(dev, code, *h, int(fqavby), int(tavby), _lib.OPS[op],
                                     _np_ptr(out))
    _lib.check(rc, "bldp_reduce_host")
    return out


def kurtosis_host_typed(a: np.ndarray, win=None, device=0, tblock=None) -> np.ndarray:
    """Host array of any supported element type in, (nc, ni) float64 out
    (bldp_kurtosis_host; StatsBase's recipe in Float64 for non-Float32 rows,
    8- and 16-bit integer rows from exact integer power sums).  With ``tblock``:
    one such call per block of tblock selected spectra, (nc, ni, nt/tblock)."""
    a = np.asarray(a)
    code = _dtype_code(a.dtype)
    if code is None or a.ndim != 3:
        raise TypeError(f"unsupported host filterbank {a.dtype} {a.shape}")
    a = np.asfortranarray(a)
    _, (nc, ni, nt) = _window(a, win)
    if tblock is not None:
        nb = _check_tblock(tblock, nt)
        out = np.empty((nc, ni, nb), dtype=np.float64, order="F")
        for b in range(nb):
            out[:, :, b] = kurtosis_host_typed(a, _block_win(win, a.shape, int(tblock), b),
                                               device=device)
        return out
    out = _host_out((nc, ni), np.float64)
    (dev, *h), keep = _host_args(device, a, win)
    rc = _lib.lib().bldp_kurtosis_host(dev, code, *h, _np_ptr(out))
    _lib.check(rc, "bldp_kurtosis_host")
    return out
