"""GPU: fqavfunc "median" / "var" / "std" of Float32 windows (csrc/stats.hip)
against Julia's Statistics restated in NumPy below.

median is compared bit for bit.  The restatement orders by the integer image
of the float (isless: -0.0 < 0.0; np.sort does not order the zeros), takes the
middle element of an odd block and a/2 + b/2 in Float32 of an even one, and
gives NaN for a block that holds a NaN.

var / std are compared with a Float64 two-pass oracle (ddof = 1) at
rtol = 1e-5, the project's Float32 bound: a sequential Float32 two-pass on
gamma(2, 5e8) data stays within 3.4e-6 of Float64 up to F = 4096, and the
kernels add in a tree, so the worst ordering has about 3x room."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu

RTOL = 1e-5
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def eng(pkg):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg._lib.lib()
    return pkg.engine


# ---------------------------------------------------------------------------
# Julia's rules in NumPy

def window(a, win):
    if win is None:
        return a
    return a[np.ix_(*[win[3 * k] + win[3 * k + 2] * np.arange(win[3 * k + 1]) for k in range(3)])]


def blocks(a, F, win=None):
    w = np.asfortranarray(window(a, win))
    assert w.shape[0] % F == 0
    return w.reshape((F, w.shape[0] // F) + w.shape[1:], order="F")


def key32(x):
    u = np.ascontiguousarray(x).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def median_ref(a, F, win=None):
    R = blocks(a, F, win)
    S = np.take_along_axis(R, np.argsort(key32(R), axis=0, kind="stable"), axis=0)
    with np.errstate(invalid="ignore"):
        r = S[F // 2] if F % 2 else S[F // 2 - 1] / np.float32(2) + S[F // 2] / np.float32(2)
    assert r.dtype == np.float32
    return np.asfortranarray(np.where(np.isnan(R).any(axis=0), np.float32(np.nan), r))


def var_ref(a, F, win=None, std=False):
    R = blocks(a, F, win).astype(np.float64)
    m = R.sum(axis=0) / F
    v = ((R - m) ** 2).sum(axis=0) / (F - 1)
    return np.asfortranarray(np.sqrt(v) if std else v)


def test_restatement_rules():
    a = np.array([3e38, 3e38, 0.0, -0.0, -0.0, 0.0, 1.0, np.nan], np.float32).reshape((8, 1, 1))
    m = median_ref(a, 2)[:, 0, 0]
    assert m[0] == np.float32(3e38) and np.isnan(m[3]) and m[1] == 0 and not np.signbit(m[1])
    z = np.array([0.0, -0.0, -0.0], np.float32).reshape((3, 1, 1))
    assert np.signbit(median_ref(z, 3)[0, 0, 0])  # sorted -0, -0, 0
    np.testing.assert_allclose(var_ref(np.array([1, 2, 4, 7], np.float32).reshape((4, 1, 1)), 4),
                               np.var([1, 2, 4, 7], ddof=1))


# ---------------------------------------------------------------------------
# data

def ties(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).integers(0, 8, shape).astype(np.float32))


def specials(shape, F, seed):
    """Signed normals with some zeros and subnormals everywhere, and whole
    blocks of: a floatmax pair in the middle (the a/2 + b/2 rule), +-0.0 only,
    +-Inf and subnormals, one value, one NaN."""
    rng = np.random.default_rng(seed)
    a = np.asfortranarray((rng.standard_normal(shape) * 1e3).astype(np.float32))
    small = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -2e-40], np.float32)
    hit = rng.random(shape) < 0.05
    a[hit] = rng.choice(small, int(hit.sum()))
    R = a.reshape((F, shape[0] // F) + tuple(shape[1:]), order="F")  # a view
    where = [(j, i, t) for t in range(shape[2]) for i in range(shape[1])
             for j in range(shape[0] // F)]
    lo = (F - 2) // 2  # values below the pair
    pair = np.concatenate([R[:lo, 0, 0, 0], np.float32([3e38, 3.3e38]),
                           np.full(F - 2 - lo, np.inf, np.float32)])
    fills = [rng.permutation(pair),
             rng.choice(np.float32([0.0, -0.0]), F),
             rng.choice(np.concatenate([small, np.float32([np.inf, -np.inf, FMAX, -FMAX])]), F),
             np.full(F, 1234.5, np.float32)]
    for blk, fill in zip(where[::-1], fills):
        R[(slice(None),) + blk] = fill
    if len(where) > len(fills):
        R[(int(rng.integers(F)),) + where[0]] = np.nan
    return a


def put(eng, a):
    return eng.fb_from_numpy(a, device="cuda:0")


# ---------------------------------------------------------------------------
# median, bit for bit

SORT_F = [2, 3, 4, 12, 32, 64]
SELECT_F = [65, 128, 1000, 1024, 4096]
# (nchan, nif, ntime) per F: several blocks a row, several workgroups
MEDIAN_SHAPES = {**{F: (768, 2, 3) for F in SORT_F},  # 768 = 4 lcm(2, 3, 4, 12, 32, 64)
                 65: (325, 2, 3), 128: (512, 2, 3), 1000: (3000, 2, 3), 1024: (2048, 2, 3),
                 4096: (8192, 2, 3), 65536: (65536, 1, 2)}
MEDIAN_PATH = {**{F: "median_sort" for F in SORT_F}, **{F: "median_select" for F in SELECT_F},
               65536: "median_stream"}


@pytest.mark.parametrize("F", SORT_F + SELECT_F + [65536])
def test_median_bits(eng, F):
    shape = MEDIAN_SHAPES[F]
    synth = eng.fb_to_numpy(eng.synth(*shape, nfpc=max(F, 4), seed=F, kind=0, device="cuda:0"))
    for name, a in (("ties", ties(shape, F)), ("synth", synth), ("specials", specials(shape, F, F))):
        x = put(eng, a)
        assert eng.plan(x, F, 1, "median")["path"] == MEDIAN_PATH[F], (F, name)
        got = eng.fb_to_numpy(eng.reduce(x, F, 1, "median"))
        want = median_ref(a, F)
        assert got.dtype == np.float32 and same_bits(got, want), (F, name)
        if name == "specials":
            assert np.isnan(want).sum() >= (shape[0] // F * shape[1] * shape[2] > 4)
            if F % 2 == 0:  # the floatmax pair sits in the middle of its block
                assert np.isin(np.float32(3e38) / 2 + np.float32(3.3e38) / 2, want)


def test_every_form_is_planned(eng):
    x = eng.fb_empty(65536, 1, 2, device="cuda:0")

    def plan(F, op):
        return eng.plan(x, F, 1, op, [0, F, 1, 0, 1, 1, 0, 2, 1])

    med = {plan(F, "median")["path"] for F in SORT_F + SELECT_F + [65536]}
    assert med == {"median_sort", "median_select", "median_stream"}
    lanes = {}
    for F in (2, 3, 64, 1024, 4096, 65536):
        p = plan(F, "var")
        assert p["path"] == "moments" and plan(F, "std") == p
        lanes[F] = (p["lanes_per_group"], p["float4_per_lane"])
    # lanes sharing a block (256 = a workgroup); float4 loads where 4 divides F
    assert lanes == {2: (2, 0), 3: (4, 0), 64: (16, 1), 1024: (64, 1), 4096: (256, 1),
                     65536: (256, 1)}
    assert plan(64, "sum")["path"] not in med | {"moments"}


# ---------------------------------------------------------------------------
# windows: c0 = 3 (off a 16-byte boundary), channel step 2, reversed channels,
# an IF pick, a time step

WIN_SHAPE = (4200, 3, 5)


def windows(F):
    nch, ni, nt = WIN_SHAPE

    def nc(c0, cs):  # two blocks where they fit, else one
        return 2 * F if 0 <= c0 + (2 * F - 1) * cs < nch else F
    return [[3, nc(3, 1), 1, 0, ni, 1, 0, nt, 1],
            [1, nc(1, 2), 2, 0, ni, 1, 0, nt, 1],
            [nch - 1, nc(nch - 1, -1), -1, 0, ni, 1, 0, nt, 1],
            [0, 2 * F, 1, 1, 1, 1, 0, nt, 1],
            [4, 2 * F, 1, 0, ni, 1, 1, 2, 2],
            [nch - 2, nc(nch - 2, -2), -2, 2, 1, 1, 4, 2, -3]]


@pytest.fixture(scope="module")
def win_data(eng):
    a = specials((4096, 3, 5), 64, 99)
    a = np.asfortranarray(np.concatenate([a, ties((104, 3, 5), 5)], axis=0))
    a[~np.isfinite(a)] = 7.0  # (var / std share it: finite, of moderate size)
    a[np.abs(a) > 1e6] = -3.0
    return a, put(eng, a)


@pytest.mark.parametrize("F", [3, 12, 64, 128, 2048])
def test_median_windows(eng, win_data, F):
    a, x = win_data
    for w in windows(F):
        got = eng.fb_to_numpy(eng.reduce(x, F, 1, "median", w))
        assert same_bits(got, median_ref(a, F, w)), (F, w)


@pytest.mark.parametrize("F", [3, 12, 64, 1024, 2048])
def test_moments_windows(eng, win_data, F):
    a, x = win_data
    for w in windows(F):
        for op in ("var", "std"):
            got = eng.fb_to_numpy(eng.reduce(x, F, 1, op, w))
            want = var_ref(a, F, w, std=op == "std")
            assert got.dtype == np.float32 and got.shape == want.shape
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=f"{F} {w} {op}")


# ---------------------------------------------------------------------------
# var / std

MOM_SHAPES = {2: (1536, 2, 3), 3: (1536, 2, 3), 64: (1536, 2, 3), 1024: (2048, 2, 3),
              4096: (8192, 2, 3)}


@pytest.mark.parametrize("F", sorted(MOM_SHAPES))
@pytest.mark.parametrize("kind", [0, 1])
def test_var_std(eng, F, kind):
    shape = MOM_SHAPES[F]
    x = eng.synth(*shape, nfpc=max(F, 4), seed=10 * F + kind, kind=kind, device="cuda:0")
    a = eng.fb_to_numpy(x)
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.reduce(x, F, 1, op))
        want = var_ref(a, F, std=op == "std")
        err = np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)
        print(f"F={F} kind={kind} {op}: max rel err {err.max():.3g}")
        assert got.dtype == np.float32 and not np.isnan(got).any() and (got >= 0).all()
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


@pytest.mark.parametrize("F", sorted(MOM_SHAPES) + [65536])
def test_constant_block_is_exactly_zero(eng, F):
    shape = MOM_SHAPES.get(F, (65536, 1, 2))
    a = np.full(shape, 1e9, dtype=np.float32, order="F")
    a[:F, 0, 0] = 3.0000001  # another constant, inexact in binary
    x = put(eng, a)
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.reduce(x, F, 1, op))
        assert (got == 0).all() and not np.signbit(got).any(), (F, op)


def test_two_pass_block(eng):
    """F = 65536: the block is read twice (the workgroup's registers hold 4096)."""
    x = eng.synth(65536, 1, 2, nfpc=65536, seed=3, kind=0, device="cuda:0")
    a = eng.fb_to_numpy(x)
    for op in ("var", "std"):
        got = eng.fb_to_numpy(eng.reduce(x, 65536, 1, op))
        np.testing.assert_allclose(got, var_ref(a, 65536, std=op == "std"), rtol=RTOL, atol=0)


def test_huge_finite_values_stay_finite_or_inf(eng):
    # sum(x - K) overflows in one direction only: the result is Inf, never NaN
    a = np.full((64, 1, 1), FMAX, dtype=np.float32, order="F")
    a[::2] = np.float32(3e38)
    got = eng.fb_to_numpy(eng.reduce(put(eng, a), 64, 1, "var"))
    assert not np.isnan(got).any() and (got >= 0).all()


# ---------------------------------------------------------------------------
# layers

def test_fqav_device_tensor(eng, pkg):
    import torch

    a = ties((256, 2, 3), 1)
    x = put(eng, a)
    r = pkg.fqav(x, 4, "median")
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.float32
    assert same_bits(eng.fb_to_numpy(r), median_ref(a, 4))
    assert same_bits(pkg.fqav(a, 4, "median"), median_ref(a, 4))  # host array: through the GPU
    # fqav(A, n <= 1) is A whatever f is; the ABI copies
    assert same_bits(eng.fb_to_numpy(eng.reduce(x, 1, 1, "var")), a)
    with pytest.raises(TypeError, match="tavby"):
        eng.reduce(x, 4, 2, "median")
    with pytest.raises(TypeError, match="tavby"):
        pkg.worker.getdata(x, fqavby=4, fqavfunc="median", tavby=2)
    with pytest.raises(TypeError, match="Float32"):
        eng.reduce(x.to(torch.int16), 4, 1, "median")
    with pytest.raises(TypeError):
        eng.band_reduce_multi([x, x], 4, 1, "median")
    rc = pkg._lib.lib().bldp_reduce_strided(7, None, 256, 2, 3, None, 4, 1, 6, None, 64, 128,
                                            None)
    assert rc == pkg._lib.BLDP_EINVAL and "Float32" in pkg._lib.last_error()


def test_band_reduce_is_the_concatenation(eng):
    banks = [specials((1024, 2, 3), 64, 20), specials((1024, 2, 3), 64, 21)]
    xs = [put(eng, b) for b in banks]
    for F, op in ((64, "median"), (256, "median"), (64, "var")):
        band = eng.fb_to_numpy(eng.band_reduce(xs, F, 1, op))
        parts = [eng.fb_to_numpy(eng.reduce(x, F, 1, op)) for x in xs]
        assert same_bits(band, np.concatenate(parts, axis=0)), (F, op)
        if op == "median":
            assert same_bits(parts[1], median_ref(banks[1], F))
    p = eng.PreparedBandReduce(xs, 64, 1, "median")
    p.launch()
    assert same_bits(eng.fb_to_numpy(p.out), eng.fb_to_numpy(eng.band_reduce(xs, 64, 1, "median")))
    p.close()


def test_prepared_reduce(eng, pkg):
    import torch

    x = eng.synth(2048, 2, 3, nfpc=64, seed=5, kind=0, device="cuda:0")
    want = eng.fb_to_numpy(eng.reduce(x, 64, 1, "var"))
    p = eng.PreparedReduce(x, 64, 1, "var")
    for _ in range(2):
        p.out.zero_()
        p.launch()
        assert same_bits(eng.fb_to_numpy(p.out), want)
    e0, e1 = pkg._lib.HipEvent(timing=True), pkg._lib.HipEvent(timing=True)
    p.out.zero_()
    p.launch_timed(None, e0, e1)  # the dispatch itself carries the events
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) >= 0 and same_bits(eng.fb_to_numpy(p.out), want)
    p.close()


def test_getdata_sigproc_file(eng, pkg, tmp_path):
    rd = pkg.readers
    data = specials((64, 2, 5), 8, 4)
    hdr = dict(telescope_id=6, machine_id=10, data_type=1, source_name="VOYAGER1",
               tstart=59000.5, tsamp=18.253611, fch1=8438.96484375, foff=-2.7939677238464355e-06,
               nchans=64, nifs=2, nbits=32)
    f = tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0000.fil"
    rd.write_fil(f, hdr, data)
    got = pkg.worker.getdata(str(f), fqavby=8, fqavfunc="median")
    assert got.dtype == np.float32 and same_bits(got, median_ref(data, 8))
    J, C = pkg.JRange, pkg.COLON
    noise = np.asfortranarray(np.random.default_rng(6).gamma(2.0, 5e8, (64, 2, 5))
                              .astype(np.float32))
    g = tmp_path / "guppi_59000_00001_VOYAGER1_0001.rawspec.0002.fil"
    rd.write_fil(g, hdr, noise)
    got = pkg.worker.getdata(str(g), (J(4, 35), C, J(2, 2, 4)), 16, "std")
    np.testing.assert_allclose(got, var_ref(noise, 16, [3, 32, 1, 0, 2, 1, 1, 2, 2], std=True),
                               rtol=RTOL, atol=0)
    band = pkg.GBT.getband([0, 0], [str(f), str(f)], fqavby=8, fqavfunc="median")
    assert same_bits(band, np.concatenate([median_ref(data, 8)] * 2, axis=0))


def test_reduce_host_matches_device(eng):
    a = np.asfortranarray(np.random.default_rng(8).gamma(2.0, 5e8, (4096, 2, 6)).astype(np.float32))
    x = put(eng, a)
    for F, op in ((64, "std"), (1024, "std"), (64, "median")):
        host = eng.reduce_host(a, F, 1, op)  # a pageable host array, not pinned
        assert host.dtype == np.float32
        assert same_bits(host, eng.fb_to_numpy(eng.reduce(x, F, 1, op))), (F, op)
    win = [5, 2048, 1, 1, 1, 1, 0, 3, 2]
    np.testing.assert_allclose(eng.reduce_host(a, 64, 1, "std", win),
                               var_ref(a, 64, win, std=True), rtol=RTOL, atol=0)
