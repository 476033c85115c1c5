"""GPU: fold and unfold (csrc/fold.hip) against the NumPy restatement of their rule
(fold_ref.py), on the cases of fold_cases.py: every path, mask load form, vector
and scalar loads, chunked and not.

Integer-valued data in 0 .. 255: every Float64 partial sum is exact in any order,
so ``data`` (sum and mean) equals the restatement bit for bit.  Gamma and signed
data: a block of n samples may differ by one Float32 rounding and by the Float64
reordering, |got - ref| <= ulp32(ref) + n 2^-52 sum|x|; how many elements differ at
all is printed.  ``kept`` is always exact.  NaN, +Inf and -Inf lie under every flag,
so each result also shows that a flagged sample never reaches the sum.

The mean differs from a Float32 rounding of ref by the same bound divided by kept."""
from __future__ import annotations

import numpy as np
import pytest

import fold_cases as fc
from fold_ref import fold_abs, fold_ref, unfold_ref
from mad_ref import window
from outliers_ref import outliers_ref
from test_gpu_masked import dmask, gamma_data, int_data, masks, poison, put, same, spiky, view

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


def signed_data(shape, seed):
    return np.random.default_rng(seed).normal(0.0, 100.0, shape).astype(np.float32)


def case_mask(c, nbank=1, seed=0):
    """The host mask of a case over its (nbank * nc, ni, nt) window, or None."""
    if c.mask is None:
        return None
    shape = (nbank * c.nfpc * c.J, c.ni, c.nt)
    return masks(shape, c.nfpc, c.T or c.nt, 1000 + seed)[c.mask]


def bit_equal(got, want):
    """The same Float32 bits, every NaN alike."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return (got.dtype == want.dtype == np.float32 and got.shape == want.shape and
            np.array_equal(np.isnan(got), nan) and
            np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


def within(got, s, k, sabs, n, mean, what):
    """|got - ref| <= ulp32(ref) + n 2^-52 sum|x| (the mean: both over kept); prints
    how many elements differ from the rounded restatement at all."""
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = s / k if mean else s
        slack = n * 2.0 ** -52 * sabs / (k if mean else 1)
    ref32 = ref.astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    ulp = np.spacing(np.abs(ref32[~nan])).astype(np.float64)
    err = np.abs(got[~nan].astype(np.float64) - ref[~nan])
    differ = int((got[~nan] != ref32[~nan]).sum())
    print("%s: %d of %d elements differ from the restatement, max err / bound %.3g" %
          (what, differ, err.size, float((err / (ulp + slack[~nan])).max()) if err.size else 0.0))
    assert (err <= ulp + slack[~nan]).all(), what


def run_case(eng, c, a, exact, seed=0):
    """One case on the GPU against the restatement; returns the plan."""
    win, T = fc.window(c), c.T or c.nt
    m = case_mask(c, seed=seed)
    ap = poison(a, win, m) if m is not None else a
    x = put(eng, ap)
    md = None if m is None else dmask(m, c.mask == "odd_address")
    w = window(ap, win)
    s, k, s32, mean = fold_ref(w, c.nfpc, T, m)
    for op in ("sum", "mean"):
        r = eng.fold(x, c.nfpc, c.T, op, mask=md, win=win)
        data, kept = eng.fb_to_numpy(r["data"]), eng.fb_to_numpy(r["kept"])
        assert kept.dtype == np.int32 and np.array_equal(kept, k), (fc.case_id(c), op)
        assert data.dtype == np.float32 and data.shape == (c.nfpc, c.ni, c.nt // T)
        if op == "sum":
            assert np.isfinite(data).all(), fc.case_id(c)  # nothing flagged reached the sum
        else:
            assert np.array_equal(np.isnan(data), k == 0), fc.case_id(c)
        if exact:
            assert bit_equal(data, s32 if op == "sum" else mean), (fc.case_id(c), op)
        else:
            within(data, s, k, fold_abs(w, c.nfpc, T, m), c.J * T, op == "mean",
                   fc.case_id(c) + " " + op)
    return eng.fold_plan(x, c.nfpc, c.T, mask=md, win=win)


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_fold_cases(eng, c):
    shape = fc.array_shape(c)
    p = run_case(eng, c, int_data(shape, 7), True)
    assert (p["path"], p["vector_loads"], p["mask_loads"], p["chunks_per_block"] > 1) == c.plan
    assert p["launches"] == (2 if c.plan[3] else 1)
    run_case(eng, c, gamma_data(shape, 8), False, seed=1)
    run_case(eng, c, signed_data(shape, 9), False, seed=2)


@pytest.mark.parametrize("nfpc,J,ni,nt,T", [(8, 4, 2, 6, 3), (3, 5, 2, 4, 2), (1024, 2, 2, 4, 2),
                                            (8, 4, 1, 4099, 4099)])
def test_every_mask_form(eng, nfpc, J, ni, nt, T):
    shape = (nfpc * J, ni, nt)
    a = int_data(shape, nfpc + T)
    for name, m in masks(shape, nfpc, T, J + T).items():
        if name == "bad_ifs" and ni == 1:
            continue
        ap = poison(a, None, m)
        s, k, s32, mean = fold_ref(ap, nfpc, T, m)
        x, md = put(eng, ap), dmask(m, name == "odd_address")
        for op, want in (("sum", s32), ("mean", mean)):
            r = eng.fold(x, nfpc, T, op, mask=md)
            assert bit_equal(eng.fb_to_numpy(r["data"]), want), (name, op)
            assert np.array_equal(eng.fb_to_numpy(r["kept"]), k), (name, op)
        want = ("row" if name in ("bad_spectra", "bad_ifs") else
                "byte" if nfpc % 4 or name == "odd_address" else "dword")
        assert eng.fold_plan(x, nfpc, T, mask=md)["mask_loads"] == want, name
    # an all-zero mask and no mask at all: the same bits, every sample kept
    x = put(eng, a)
    r0 = eng.fold(x, nfpc, T, "sum")
    r1 = eng.fold(x, nfpc, T, "sum", mask=dmask(np.zeros((1, 1, 1), np.uint8)))
    assert bit_equal(eng.fb_to_numpy(r0["data"]), eng.fb_to_numpy(r1["data"]))
    assert (eng.fb_to_numpy(r0["kept"]) == J * T).all()
    # ... and the torch route on exact data
    want = x.permute(2, 1, 0).contiguous().view(nt // T, T, ni, J, nfpc).sum((1, 3)).permute(2, 1, 0)
    assert bit_equal(eng.fb_to_numpy(r0["data"]), eng.fb_to_numpy(want))


@pytest.mark.parametrize("nfpc,J,ni,nt,T", [(8, 4, 2, 6, 3), (5, 3, 1, 34, 17), (1024, 3, 2, 4, 2),
                                            (1024, 5, 1, 273, 273), (4, 1, 1, 20000, 20000)])
def test_kept_nan_propagates_to_its_own_output(eng, nfpc, J, ni, nt, T):
    a = int_data((nfpc * J, ni, nt), 3)
    k0, i0, t0 = nfpc // 2, ni - 1, nt - 1   # (the spike bin of the last coarse channel)
    a[(J - 1) * nfpc + k0, i0, t0] = np.nan
    x = put(eng, a)
    for op in ("sum", "mean"):
        d = eng.fb_to_numpy(eng.fold(x, nfpc, T, op)["data"])
        want = np.zeros(d.shape, bool)
        want[k0, i0, t0 // T] = True
        assert np.array_equal(np.isnan(d), want), op


def test_nothing_kept_gives_zero_and_nan(eng):
    a = int_data((32, 2, 8), 4)
    m = np.zeros((32, 1, 1), np.uint8)
    m[3::8] = 9      # fine bin 3 of every coarse channel
    x, md = put(eng, poison(a, None, m)), dmask(m)
    s = eng.fb_to_numpy(eng.fold(x, 8, 4, "sum", mask=md)["data"])
    mean = eng.fold(x, 8, 4, "mean", mask=md)
    assert (s[3] == 0).all() and not np.signbit(s[3]).any() and np.isfinite(s).all()
    assert np.isnan(eng.fb_to_numpy(mean["data"])[3]).all()
    assert (eng.fb_to_numpy(mean["kept"])[3] == 0).all()
    assert np.isfinite(np.delete(eng.fb_to_numpy(mean["data"]), 3, axis=0)).all()


@pytest.mark.parametrize("c", [c for c in fc.CASES if c.plan[3]][:4], ids=fc.case_id)
def test_two_calls_give_identical_bytes(eng, c):
    shape = fc.array_shape(c)
    x = put(eng, signed_data(shape, 11))
    m = case_mask(c)
    md = None if m is None else dmask(m, c.mask == "odd_address")
    r = [eng.fold(x, c.nfpc, c.T, "mean", mask=md, win=fc.window(c)) for _ in range(3)]
    assert eng.fold_plan(x, c.nfpc, c.T, mask=md, win=fc.window(c))["chunks_per_block"] > 1
    for q in r[1:]:
        assert eng.fb_to_numpy(q["data"]).tobytes() == eng.fb_to_numpy(r[0]["data"]).tobytes()
        assert eng.fb_to_numpy(q["kept"]).tobytes() == eng.fb_to_numpy(r[0]["kept"]).tobytes()


@pytest.mark.parametrize("axis,n", [(0, 16), (2, 8), (2, None)])
def test_outliers_mask_goes_straight_in(eng, axis, n):
    a = spiky((64, 2, 24), 40 + axis)
    x = put(eng, a)
    o = eng.outliers(x, n, axis=axis, nsigma=3.0, mask=True, which=("count",))
    m = eng.fb_to_numpy(o["mask"])
    assert m.any() and np.array_equal(m, outliers_ref(a, n or 24, 3.0, None, axis)[3])
    for nfpc, T in ((16, 8), (4, 1), (64, None), (1, 24)):
        s, k, s32, mean = fold_ref(a, nfpc, T, m)
        r = eng.fold(x, nfpc, T, "mean", mask=o["mask"])
        assert bit_equal(eng.fb_to_numpy(r["data"]), mean)
        assert np.array_equal(eng.fb_to_numpy(r["kept"]), k)
        assert int(r["kept"].sum()) + int(o["count"].sum()) == a.size


# ---- the band: one profile over every bank --------------------------------------------------
@pytest.mark.parametrize("c", fc.BAND_CASES, ids=fc.case_id)
def test_band_fold_is_the_fold_of_the_concatenation(eng, c):
    shape = fc.array_shape(c)
    nc = shape[0]
    m = case_mask(c, nbank=3)
    banks = [int_data(shape, 20 + b) for b in range(3)]
    if m is not None:
        banks = [poison(a, None, m[b * nc:(b + 1) * nc] if m.shape[0] > 1 else m)
                 for b, a in enumerate(banks)]
    cat = np.concatenate(banks)
    xs, xc = [put(eng, a) for a in banks], put(eng, cat)
    md = None if m is None else dmask(m)
    s, k, s32, mean = fold_ref(cat, c.nfpc, c.T, m)
    for op, want in (("sum", s32), ("mean", mean)):
        r = eng.band_fold(xs, c.nfpc, c.T, op, mask=md)
        one = eng.fold(xc, c.nfpc, c.T, op, mask=md)
        assert tuple(r["data"].shape) == (c.nfpc, c.ni, c.nt // (c.T or c.nt))
        assert bit_equal(eng.fb_to_numpy(r["data"]), want), op
        assert bit_equal(eng.fb_to_numpy(r["data"]), eng.fb_to_numpy(one["data"])), op
        assert np.array_equal(eng.fb_to_numpy(r["kept"]), k)
    # gamma data: the band and the concatenation within the bound of each other's reference
    g = [gamma_data(shape, 30 + b) for b in range(3)]
    r = eng.band_fold([put(eng, a) for a in g], c.nfpc, c.T, "sum")
    gc = np.concatenate(g)
    s, k, _, _ = fold_ref(gc, c.nfpc, c.T)
    within(eng.fb_to_numpy(r["data"]), s, k, fold_abs(gc, c.nfpc, c.T), 3 * c.J * (c.T or c.nt),
           False, "band " + fc.case_id(c))
    # band_unfold equals the concatenated unfold
    prof = eng.band_fold(xs, c.nfpc, c.T, "mean")["data"]
    for how in ("divide", "subtract"):
        got = eng.fb_to_numpy(eng.band_unfold(xs, prof, c.nfpc, c.T, how))
        assert bit_equal(got, eng.fb_to_numpy(eng.unfold(xc, prof, c.nfpc, c.T, how))), how
        if m is None:
            assert bit_equal(got, unfold_ref(cat, eng.fb_to_numpy(prof), c.nfpc, c.T, how)), how


# ---- unfold -----------------------------------------------------------------------------
@pytest.mark.parametrize("c,vec", fc.UNFOLD_CASES, ids=lambda v: fc.case_id(v) if isinstance(v, tuple) else str(v))
def test_unfold(eng, c, vec):
    shape, win, T = fc.array_shape(c), fc.window(c), c.T or c.nt
    rng = np.random.default_rng(5)
    for a in (gamma_data(shape, 41), signed_data(shape, 42)):
        w = window(a, win)
        prof = rng.gamma(2.0, 50.0, (c.nfpc, c.ni, c.nt // T)).astype(np.float32)
        special = [0.0, INF, NAN, -0.0][:min(4, prof.size)]  # IEEE results stand
        prof.ravel()[:len(special)] = special
        x, pd = put(eng, a), put(eng, prof)
        assert eng.unfold_plan(x, c.nfpc, c.T, win=win)["vector_loads"] == vec
        for how in ("divide", "subtract"):
            got = eng.fb_to_numpy(eng.unfold(x, pd, c.nfpc, c.T, how, win=win))
            assert bit_equal(got, unfold_ref(w, prof, c.nfpc, T, how)), (fc.case_id(c), how)
        # zeros, infinities and NaNs in the window as well
        b = a.copy()
        view(b, win)[0, 0, :4] = [0.0, INF, NAN, -INF][:min(4, c.nt)]
        got = eng.fb_to_numpy(eng.unfold(put(eng, b), pd, c.nfpc, c.T, "divide", win=win))
        assert bit_equal(got, unfold_ref(window(b, win), prof, c.nfpc, T, "divide"))


@pytest.mark.parametrize("nfpc,J", [(8, 4), (3, 5)])
def test_unfold_strided_out_and_profile(eng, nfpc, J):
    """A bank writes its slot of a stitched band; the profile is a view of a wider one."""
    nc, ni, nt, T = nfpc * J, 2, 6, 3
    a = gamma_data((nc, ni, nt), 51)
    wide = np.random.default_rng(52).gamma(2.0, 50.0, (nfpc + 4, ni, nt // T)).astype(np.float32)
    x, pw = put(eng, a), put(eng, wide)
    band = eng.fb_empty(3 * nc, ni, nt, device="cuda:0")
    band.fill_(-7.0)
    for off, pv in ((nc, pw[:nfpc]), (2 * nc, pw[4:4 + nfpc])):
        out = band[off:off + nc]
        p = eng.unfold_plan(x, nfpc, T, prof=pv, out=out)
        assert p["vector_loads"] == int(nfpc % 4 == 0)
        got = eng.unfold(x, pv, nfpc, T, "divide", out=out)
        assert got.data_ptr() == out.data_ptr()
    h = eng.fb_to_numpy(band)
    assert (h[:nc] == -7).all()
    assert bit_equal(h[nc:2 * nc], unfold_ref(a, wide[:nfpc], nfpc, T))
    assert bit_equal(h[2 * nc:], unfold_ref(a, wide[4:4 + nfpc], nfpc, T))
    # a profile one float off the float4 grid takes the scalar kernel, with the same bits
    pv = pw[1:1 + nfpc]
    assert eng.unfold_plan(x, nfpc, T, prof=pv)["vector_loads"] == 0
    assert bit_equal(eng.fb_to_numpy(eng.unfold(x, pv, nfpc, T, "subtract")),
                     unfold_ref(a, wide[1:1 + nfpc], nfpc, T, "subtract"))
    with pytest.raises(ValueError):  # not in place
        eng.unfold(x, pw[:nfpc], nfpc, T, out=x)


def test_strided_and_single_fold_outputs(eng, pkg):
    import torch

    nfpc, J, ni, nt, T = 8, 4, 2, 6, 3
    a = int_data((nfpc * J, ni, nt), 61)
    x = put(eng, a)
    s, k, s32, mean = fold_ref(a, nfpc, T)
    out = eng.fb_empty(3 * nfpc, ni, nt // T, device="cuda:0")
    kept = eng.fb_empty(3 * nfpc, ni, nt // T, device="cuda:0", dtype=torch.int32)
    out.fill_(-7.0)
    kept.fill_(-7)
    ptr, nchan, nif, ntime = eng._abi_dims(x)
    L = pkg._lib.lib()
    # the middle slot of a wider product; then out only, kept only
    pkg._lib.check(L.bldp_fold_f32(ptr, nchan, nif, ntime, None, nfpc, T, 0, None, None,
                                   out.data_ptr() + 4 * nfpc, kept.data_ptr() + 4 * nfpc, 3 * nfpc,
                                   3 * nfpc * ni, None), "bldp_fold_f32")
    pkg._lib.check(L.bldp_fold_f32(ptr, nchan, nif, ntime, None, nfpc, T, 1, None, None,
                                   out.data_ptr() + 8 * nfpc, None, 3 * nfpc, 3 * nfpc * ni, None),
                   "bldp_fold_f32")
    pkg._lib.check(L.bldp_fold_f32(ptr, nchan, nif, ntime, None, nfpc, T, 0, None, None, None,
                                   kept.data_ptr(), 3 * nfpc, 3 * nfpc * ni, None), "bldp_fold_f32")
    o, kk = eng.fb_to_numpy(out), eng.fb_to_numpy(kept)
    assert bit_equal(o[nfpc:2 * nfpc], s32) and bit_equal(o[2 * nfpc:], mean) and (o[:nfpc] == -7).all()
    assert np.array_equal(kk[:nfpc], k) and np.array_equal(kk[nfpc:2 * nfpc], k)
    assert (kk[2 * nfpc:] == -7).all()


# ---- the pipeline -------------------------------------------------------------------------
def test_getflattened_flattens_the_synthetic_passband(eng, pkg):
    nfpc, J, nt = 64, 8, 32
    x = eng.synth(nfpc * J, 1, nt, nfpc=nfpc, seed=3, kind=0, device="cuda:0")
    a = eng.fb_to_numpy(x)
    prof = eng.fb_to_numpy(eng.fold(x, nfpc)["data"])[:, 0, 0]
    # the scallop and the DC spike are in the raw profile ...
    assert prof[nfpc // 2] > 4 * np.median(prof) and prof.max() > 4 * prof.min()
    r = pkg.worker.getflattened(x, nfpc=nfpc)
    assert sorted(r) == ["data", "kept", "profile"] and tuple(r["data"].shape) == (nfpc * J, 1, nt)
    flat = eng.fb_to_numpy(r["data"])
    assert bit_equal(flat, unfold_ref(a, eng.fb_to_numpy(r["profile"]), nfpc))
    assert bit_equal(eng.fb_to_numpy(r["profile"]), fold_ref(a, nfpc)[3])
    assert (eng.fb_to_numpy(r["kept"]) == J * nt).all()
    # ... and the per-k mean of the flattened window is 1, the spike bin included: one
    # rounding of the profile, one of every quotient (positive data), and one of the
    # Float32 mean itself
    m64 = fold_ref(flat, nfpc)[0][:, 0, 0] / (J * nt)
    assert np.abs(m64 - 1).max() <= 2 * 2.0 ** -24 * (1 + 2.0 ** -20), np.abs(m64 - 1).max()
    m32 = eng.fb_to_numpy(eng.fold(r["data"], nfpc)["data"])[:, 0, 0]
    assert np.abs(m32.astype(np.float64) - 1).max() <= 3 * 2.0 ** -24 * (1 + 2.0 ** -20)
    # subtracting leaves a zero-mean window, within the same roundings of the profile's size
    sub = pkg.worker.getflattened(x, nfpc=nfpc, how="subtract")
    z = fold_ref(eng.fb_to_numpy(sub["data"]), nfpc)[0][:, 0, 0] / (J * nt)
    assert (np.abs(z) <= 2 * 2.0 ** -24 * a.reshape(J, nfpc, nt).max(axis=(0, 2))).all()
    # with nsigma the profile is folded over the unflagged samples alone
    b = a.copy()
    b[5 * nfpc + 7, 0, 3] = 1e14   # (the noise is a gamma of mean 1e9)
    r = pkg.worker.getflattened(put(eng, b), nfpc=nfpc, nsigma=5.0, n=nfpc, axis=0)
    _, _, _, m = outliers_ref(b, nfpc, 5.0, None, 0)
    assert m[5 * nfpc + 7, 0, 3] and bit_equal(eng.fb_to_numpy(r["profile"]),
                                                fold_ref(b, nfpc, None, m)[3])
    assert np.array_equal(eng.fb_to_numpy(r["kept"]), fold_ref(b, nfpc, None, m)[1])
    assert eng.fb_to_numpy(r["profile"])[7, 0, 0] < 1e10


def test_getbandpass_sources_and_gbt(eng, pkg, tmp_path):
    import torch

    W, J, C = pkg.worker, pkg.JRange, pkg.COLON
    data = spiky((64, 2, 40), 50)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    fil = str(tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil")
    raw = str(tmp_path / "raw.rawspec.0000.h5")
    pkg.readers.write_fil(fil, hdr, data)
    pkg.fbh5.write(raw, dict(foff=-1.0, nfpc=16), data)
    # the FBH5 header names nfpc = 16; the whole file, the whole time range
    got = W.getbandpass(raw)
    s, k, s32, mean = fold_ref(data, 16)
    assert bit_equal(got["data"], mean) and np.array_equal(got["kept"], k)
    assert got["kept"].dtype == np.int32
    idxs, win = (J(5, 36), C, J(40, -1, 9)), [4, 32, 1, 0, 2, 1, 39, 32, -1]
    m = masks((32, 2, 32), 8, 4, 51)["random"]
    bad = masks((32, 2, 32), 8, 4, 52)["bad_channels"]
    x = put(eng, data)
    for src in (data, x, fil, raw):
        dev = isinstance(src, torch.Tensor)
        host = (lambda r: {k: eng.fb_to_numpy(t) for k, t in r.items()}) if dev else (lambda r: r)
        for mk in (None, m, bad, m != 0, dmask(m)):
            for func in ("sum", "mean"):
                got = W.getbandpass(src, idxs, nfpc=8, tavby=4, func=func, mask=mk)
                assert all(isinstance(v, torch.Tensor if dev else np.ndarray) for v in got.values())
                mh = mk.cpu().numpy() if isinstance(mk, torch.Tensor) else mk
                s, k, s32, mean = fold_ref(window(data, win), 8, 4, mh)
                got = host(got)
                assert bit_equal(got["data"], s32 if func == "sum" else mean), func
                assert np.array_equal(got["kept"], k)
        got = host(W.getflattened(src, idxs, nfpc=8, tavby=4, how="subtract"))
        w = window(data, win)
        assert bit_equal(got["profile"], fold_ref(w, 8, 4)[3])
        assert bit_equal(got["data"], unfold_ref(w, got["profile"], 8, 4, "subtract"))
    # the fan-out: two banks, one profile, combined in Float64 before the division
    got = pkg.GBT.getbandpass([0, 0], [fil, raw], idxs, nfpc=8, tavby=4)
    s, k, _, _ = fold_ref(window(data, win), 8, 4)
    assert got["data"].dtype == np.float32 and np.array_equal(got["kept"], 2 * k)
    assert bit_equal(got["data"], (2 * s / (2 * k)).astype(np.float32))
    parts = pkg.GBT.getflattened([0, 0], [fil, raw], idxs, nfpc=8, tavby=4)
    assert len(parts) == 2
    for p in parts:
        assert bit_equal(p["data"], unfold_ref(window(data, win), fold_ref(window(data, win), 8, 4)[3],
                                               8, 4))


def test_host_entry_points_against_the_device_ones(eng):
    a = int_data((40, 2, 12), 60)
    win = [3, 32, 1, 0, 2, 1, 11, 12, -1]
    x = put(eng, a)
    for name, m in masks((32, 2, 12), 8, 4, 61).items():
        ap = np.asfortranarray(poison(a, win, m))
        s, k, s32, mean = fold_ref(window(ap, win), 8, 4, m)
        r = eng.fold_host(ap, 8, 4, "mean", mask=m, win=win)
        assert r["data"].flags.f_contiguous and r["kept"].dtype == np.int32
        assert bit_equal(r["data"], mean) and np.array_equal(r["kept"], k), name
        d = eng.fold(put(eng, ap), 8, 4, "mean", mask=dmask(m), win=win)
        assert bit_equal(r["data"], eng.fb_to_numpy(d["data"])), name
    r = eng.fold_host(np.asfortranarray(a), 8, None, "sum", win=win)   # no mask, T = nt
    d = eng.fold(x, 8, None, "sum", win=win)
    assert bit_equal(r["data"], eng.fb_to_numpy(d["data"])) and (r["kept"] == 4 * 12).all()
    g = np.asfortranarray(gamma_data((40, 2, 12), 62))
    prof = eng.fold_host(g, 8, 4, "mean", win=win)["data"]
    for how in ("divide", "subtract"):
        u = eng.unfold_host(g, prof, 8, 4, how, win=win)
        assert u.flags.f_contiguous and u.shape == (32, 2, 12)
        assert bit_equal(u, unfold_ref(window(g, win), prof, 8, 4, how)), how
        dv = eng.unfold(put(eng, g), put(eng, prof), 8, 4, how, win=win)
        assert bit_equal(u, eng.fb_to_numpy(dv)), how
