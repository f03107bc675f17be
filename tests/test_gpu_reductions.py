"""The reductions and element-wise helpers the skimage facades rest on (`mi_sum`, `mi_min_max`, `mi_elementwise`,
`mi_scalar_op`) and the image metrics, against NumPy in float64.

Sums of the exactly summable arrays of tests/helpers/array_cases.py must EQUAL the reference (any summation order gives the
same float64); sums of general float64 values are held to the classical bound (n - 1) u sum|x_i| that holds for every
order (`ac.sum_bound`).  No tolerance in this module is measured."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import array_cases as ac
from test_gpu_skimage import _ssim_host

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
COMPUTE_DTYPES = tuple(d for d in ac.DTYPES if d != np.float16)           # float16 is a storage type: see the *_float16 tests


@pytest.fixture(scope="module")
def S(gpu):
    from cupyimg_amd.scipy.ndimage import _support
    return _support


@pytest.fixture(scope="module")
def metrics(gpu):
    from cupyimg_amd.skimage import metrics
    return metrics


def _mi_sum(op, a, b=None):
    """(return code, result) of mi_sum, called directly"""
    from cupyimg_amd import _lib
    out = ctypes.c_double(-12345.0)
    da = a._desc()
    if b is None:
        rc = _lib.load().mi_sum(op, ctypes.byref(da), None, ctypes.byref(out), None)
    else:
        db = b._desc()
        rc = _lib.load().mi_sum(op, ctypes.byref(da), ctypes.byref(db), ctypes.byref(out), None)
    return rc, out.value


# ---------------------------------------------------------------- mi_sum
def _sum_cases(gpu, dtype):
    """(name, device a, device b, host a, host b): the shapes at which sum_kernel takes another path"""
    def pair(shape, seed, cut=None):
        ha, hb = ac.exact_array(dtype, shape, seed), ac.exact_array(dtype, shape, seed + 1000)
        if shape == ():
            da, db = gpu.asarray(ha.reshape(1))[0], gpu.asarray(hb.reshape(1))[0]         # a 0-d device array
            assert da.shape == ()
        else:
            da, db = gpu.asarray(ha), gpu.asarray(hb)
        if cut is not None:
            ha, hb, da, db = ha[cut], hb[cut], da[cut], db[cut]
        return da, db, ha, hb

    inner = slice(1, -1)
    yield ("0-d",) + pair((), 1)
    for n in (1, 4095, 4096, 4097):
        yield ("({},)".format(n),) + pair((n,), n)
    yield ("(3, 4096)",) + pair((3, 4096), 11)                    # contiguous, n % 4096 == 0: rows of 4096
    yield ("(5, 4099)",) + pair((5, 4099), 12)                    # contiguous, n % 4096 != 0: walks its own rows
    yield ("(70, 70, 5) of (70, 70, 9)",) + pair((70, 70, 9), 13, (Ellipsis, slice(2, 7)))      # 4900 rows > 4096 blocks
    yield ("rank 4 crop",) + pair((9, 10, 11, 12), 14, (inner,) * 4)
    yield ("rank 5 crop",) + pair((6, 7, 8, 9, 10), 15, (inner,) * 5)
    # b strided differently from a
    ha = ac.exact_array(dtype, (64, 65), 16)
    hb = ac.exact_array(dtype, (65, 64), 17)
    yield "b transposed", gpu.asarray(ha), gpu.asarray(hb).T, ha, hb.T
    hb = ac.exact_array(dtype, (64, 130), 18)
    yield "b every second column", gpu.asarray(ha), gpu.asarray(hb)[:, ::2], ha, hb[:, ::2]
    yield "a reversed rows", gpu.asarray(ha)[::-1], gpu.asarray(hb)[:, 1::2], ha[::-1], hb[:, 1::2]


@pytest.mark.parametrize("dtype", COMPUTE_DTYPES, ids=str)
def test_sum_is_exact(gpu, dtype):
    for name, da, db, ha, hb in _sum_cases(gpu, dtype):
        assert ha.size <= ac.EXACT_MAX_FLOAT_TERMS
        for op in (0, 1, 2):
            want, _ = ac.sum_reference(op, ha, hb)
            rc, got = _mi_sum(op, da, db if op == 1 else None)
            assert rc == 0 and got == want, "mi_sum op {} on {} {}: got {!r}, exact {!r}".format(op, dtype, name, got, want)


def test_sum_many_rows_uint8(gpu):
    """4097 x 4096 contiguous uint8: 4097 rows of 4096 for 4096 workgroups, so the row loop strides"""
    rng = np.random.default_rng(21)
    ha = rng.integers(0, 256, size=(4097, 4096), dtype=np.uint8)
    hb = np.roll(ha, 12345).reshape(ha.shape)
    hb[-1, -1] ^= 0x80
    da, db = gpu.asarray(ha), gpu.asarray(hb)
    a64, b64 = ha.astype(np.int64), hb.astype(np.int64)
    for op, want in ((0, int(a64.sum())), (1, int(((a64 - b64) ** 2).sum())), (2, int((a64 * a64).sum()))):
        rc, got = _mi_sum(op, da, db if op == 1 else None)
        assert rc == 0 and got == float(want), (op, got, want)           # integers below 2**53: exact in any order


def test_sum_general_float64_within_the_summation_bound(gpu):
    for shape, cut in [((20011,), None), ((5, 4099), None), ((70, 70, 9), (Ellipsis, slice(2, 7))), ((4, 4096), None)]:
        n = int(np.prod(shape))
        ha = ac.general_f64(n, 31).reshape(shape)
        hb = ac.general_f64(n, 32).reshape(shape)
        da, db = gpu.asarray(ha), gpu.asarray(hb)
        if cut is not None:
            ha, hb, da, db = ha[cut], hb[cut], da[cut], db[cut]
        for op in (0, 1, 2):
            want, mag = ac.sum_reference(op, ha, hb)
            rc, got = _mi_sum(op, da, db if op == 1 else None)
            bound = ac.sum_bound(ha.size, mag)
            print("mi_sum op {} {}: error {:.3e}, bound {:.3e}".format(op, shape, abs(got - want), bound))
            assert rc == 0 and abs(got - want) <= bound, (op, shape, got, want, bound)


def test_sum_float16_is_refused_cleanly(gpu):
    """float16 is a storage type: mi_sum answers MI_ERR_INVALID_ARG and leaves 0.0, never a number read from half data"""
    from cupyimg_amd import _lib
    a = gpu.asarray(ac.exact_array(np.float16, (300,), 1))
    for op in (0, 1, 2):
        rc, got = _mi_sum(op, a, a if op == 1 else None)
        assert rc == _lib.MI_ERR_INVALID_ARG and got == 0.0, (op, rc, got)
        assert "float16" in _lib.last_error()
    rc, got = _mi_sum(0, gpu.empty((0,), np.float32))
    assert rc == 0 and got == 0.0
    rc, _ = _mi_sum(1, gpu.zeros((4,), np.float32), None)
    assert rc == _lib.MI_ERR_INVALID_ARG
    rc, _ = _mi_sum(1, gpu.zeros((4,), np.float32), gpu.zeros((4,), np.float64))
    assert rc == _lib.MI_ERR_INVALID_ARG


# ---------------------------------------------------------------- mi_min_max
_MM_BIG = 262144 + 77              # more than 1024 blocks of 256: the blocks stride


def _mid_values(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype.kind == "b":
        return np.zeros(n, bool), False, True
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        lo, hi = (info.min, info.max) if dtype.itemsize < 8 else (info.min + 1, info.max - 1)      # 64 bit: not a power of two
        mid = rng.integers(max(info.min // 2, -1000), min(info.max // 2, 1000), size=n).astype(dtype)
        return mid, lo, hi
    mid = rng.uniform(-1000, 1000, size=n).astype(dtype)
    return mid, dtype.type(-1e30), dtype.type(3e30)


@pytest.mark.parametrize("dtype", COMPUTE_DTYPES, ids=str)
def test_min_max_every_size_and_position(gpu, S, dtype):
    for n in (1, 255, 256, 257, _MM_BIG):
        mid, lo, hi = _mid_values(dtype, n, n)
        places = [(0, n - 1), (n - 1, 0)] + ([(262144, 262143), (5, 262144)] if n > 262144 else [])
        for at_lo, at_hi in places:
            x = mid.copy()
            x[at_hi] = hi
            if at_lo != at_hi:
                x[at_lo] = lo
            got = S.min_max(gpu.asarray(x))
            want = (float(x.min()), float(x.max()))              # float() of a 64-bit integer: the extremum rounded to double
            assert got == want and all(isinstance(g, float) for g in got), (dtype, n, at_lo, at_hi, got, want)
    # a non-contiguous view is compacted first
    x = _mid_values(dtype, 600, 3)[0].reshape(20, 30)
    got = S.min_max(gpu.asarray(x)[::2, ::-3])
    assert got == (float(x[::2, ::-3].min()), float(x[::2, ::-3].max()))


def test_min_max_64bit_extrema_round_to_double(gpu, S):
    x = np.array([5, 2 ** 63 - 2, -2 ** 63 + 1, 2 ** 53 + 1, -2 ** 53 - 1], np.int64)
    assert S.min_max(gpu.asarray(x)) == (-(2.0 ** 63), 2.0 ** 63)
    assert S.min_max(gpu.asarray(x[3:])) == (-(2.0 ** 53), 2.0 ** 53)
    y = np.array([2 ** 64 - 1, 2 ** 53 + 1, 2 ** 63 + 1], np.uint64)
    assert S.min_max(gpu.asarray(y)) == (2.0 ** 53, 2.0 ** 64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_min_max_skips_nans(gpu, S, dtype):
    rng = np.random.default_rng(4)
    x = rng.uniform(-5, 5, size=_MM_BIG).astype(dtype)
    x[rng.random(x.size) < 0.3] = np.nan
    x[0] = x[-1] = x[262144] = np.nan
    assert S.min_max(gpu.asarray(x)) == (float(np.nanmin(x)), float(np.nanmax(x)))
    x[1000], x[-2] = np.inf, -np.inf
    assert S.min_max(gpu.asarray(x)) == (-np.inf, np.inf)
    x[-2] = np.nan
    assert S.min_max(gpu.asarray(x)) == (float(np.nanmin(x)), np.inf)
    y = np.full(257, np.nan, dtype)
    y[256] = -0.5
    assert S.min_max(gpu.asarray(y)) == (-0.5, -0.5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_min_max_of_all_nans_is_nan(gpu, S, dtype):
    """the decision documented in S.min_max: no sample to report, so both answers are NaN (what np.min / np.max give)"""
    for n in (1, 257, 70000):
        lo, hi = S.min_max(gpu.asarray(np.full(n, np.nan, dtype)))
        assert math.isnan(lo) and math.isnan(hi), (n, lo, hi)
    assert "NaN" in S.min_max.__doc__


def test_min_max_refusals(gpu, S):
    with pytest.raises(RuntimeError, match="float16"):
        S.min_max(gpu.asarray(np.ones(5, np.float16)))
    with pytest.raises(RuntimeError, match="empty"):
        S.min_max(gpu.empty((0,), np.float32))


# ---------------------------------------------------------------- mi_elementwise
def _operands(dtype):
    lad = ac.ladder(dtype)
    a = np.repeat(lad, lad.size)
    b = np.tile(lad, lad.size)                                    # every pair of ladder values: wrap-around included
    return a, b


@pytest.mark.parametrize("dtype", COMPUTE_DTYPES, ids=str)
def test_elementwise_matches_numpy_ufuncs(gpu, S, dtype):
    a, b = _operands(dtype)
    if dtype.kind == "b":
        ufuncs = {"add": np.logical_or, "subtract": np.logical_xor, "multiply": np.logical_and}
    else:
        ufuncs = {"add": np.add, "subtract": np.subtract, "multiply": np.multiply}
    da, db = gpu.asarray(a), gpu.asarray(b)
    for op, uf in ufuncs.items():
        with np.errstate(all="ignore"):
            want = uf(a, b)
        assert want.dtype == dtype
        got = S.elementwise(op, da, db, gpu.empty(a.shape, dtype)).get()
        if not ac.same(got, want):
            bad = np.flatnonzero(~((got == want) | (np.isnan(got.astype(np.float64)) & np.isnan(want.astype(np.float64)))))
            i = int(bad[0]) if bad.size else 0
            raise AssertionError("{} on {}: {} differ, e.g. {!r} {!r} -> {!r}, NumPy {!r}".format(
                op, dtype, bad.size, a[i].item(), b[i].item(), got[i].item(), want[i].item()))
    # a strided `out` (the result goes through a contiguous temporary) keeps the rest of its array
    big_host = np.full((2 * a.size + 1,), 3, dtype)
    big = gpu.asarray(big_host)
    S.elementwise("add", da, db, big[1::2])
    with np.errstate(all="ignore"):
        big_host[1::2] = ufuncs["add"](a, b)
    assert ac.same(big.get(), big_host)


def test_elementwise_casts_operands_to_the_output_dtype(gpu, S):
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, size=(33, 17)).astype(np.uint8)
    b = rng.integers(-32768, 32768, size=(33, 17)).astype(np.int16)
    for out_dtype in (np.float32, np.int32, np.uint8, np.float64):
        for op, uf in (("add", np.add), ("subtract", np.subtract), ("multiply", np.multiply)):
            got = S.elementwise(op, gpu.asarray(a), gpu.asarray(b).T.copy().T, gpu.empty(a.shape, out_dtype)).get()
            want = uf(a.astype(out_dtype), b.astype(out_dtype))
            assert got.dtype == want.dtype and np.array_equal(got, want), (out_dtype, op)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_elementwise_sqrt(gpu, S, dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(8)
    kmax = 2 ** 12 if dtype == np.float32 else 2 ** 26              # k * k is exact in the type
    k = np.concatenate([np.arange(0, 1025), rng.integers(0, kmax, size=20000), [kmax - 1]]).astype(np.float64)
    sq = (k * k).astype(dtype)
    got = S.elementwise("sqrt", gpu.asarray(sq), None, gpu.empty(sq.shape, dtype)).get()
    assert np.array_equal(got, k.astype(dtype)) and np.array_equal(got, np.sqrt(sq))
    # general positive values: within one ulp of the output type of the correctly rounded root
    x = np.concatenate([rng.uniform(0, 4, size=50000), 10.0 ** rng.uniform(-30, 30, size=50000)]).astype(dtype)
    x = np.concatenate([x, np.array([np.finfo(dtype).tiny, np.finfo(dtype).max, np.finfo(dtype).smallest_subnormal], dtype)])
    want = np.sqrt(x)                                               # IEEE: correctly rounded
    got = S.elementwise("sqrt", gpu.asarray(x), None, gpu.empty(x.shape, dtype)).get()
    u = np.dtype("i{}".format(dtype.itemsize))
    ulps = np.abs(got.view(u).astype(np.int64) - want.view(u).astype(np.int64))        # positive floats: ordered like their bits
    print("sqrt {}: {} of {} general values differ from the correctly rounded root, worst {} ulp".format(
        dtype, int((ulps != 0).sum()), x.size, int(ulps.max())))
    assert ulps.max() <= 1, (dtype, int(ulps.max()))
    special = np.array([0.0, -0.0, np.inf, np.nan, -1.0], dtype)
    with np.errstate(invalid="ignore"):
        want = np.sqrt(special)
    assert ac.same(S.elementwise("sqrt", gpu.asarray(special), None, gpu.empty(special.shape, dtype)).get(), want)


def test_elementwise_float16_is_refused_cleanly(gpu):
    from cupyimg_amd import _lib
    a = gpu.asarray(np.ones(8, np.float16))
    out = gpu.asarray(np.full(8, 3, np.float16))
    da, dd = a._desc(), out._desc()
    rc = _lib.load().mi_elementwise(0, ctypes.byref(da), ctypes.byref(da), ctypes.byref(dd), None)
    assert rc == _lib.MI_ERR_INVALID_ARG and "float16" in _lib.last_error()
    assert (out.get() == 3).all()


# ---------------------------------------------------------------- mi_scalar_op
def _exact_affine(x, s, t, dtype):
    """x * s + t evaluated exactly and rounded once to float64 (a fused multiply-add), then to `dtype`"""
    s, t = Fraction(float(s)), Fraction(float(t))
    return np.array([float(Fraction(float(v)) * s + t) for v in x.ravel().tolist()], np.float64).astype(dtype).reshape(x.shape)


def _check_scale_shift(S, gpu, x, s, t, out_dtype, dev_dtype=None):
    """float64 arithmetic rounded once: the exact value of x * s + t rounded to float64 (the kernel's `a * s + t` in double
    is one fused multiply-add), then to the output dtype.  Where the product is exact anyway (t == 0, s a power of two)
    NumPy's product-and-sum is the same number."""
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore"):
        want = _exact_affine(x64, s, t, out_dtype)
        two_step = (x64 * float(s) + float(t)).astype(out_dtype)
    if t == 0.0 or math.frexp(s)[0] == 0.5:
        assert ac.same(two_step, want)
    got = S.scale_shift(gpu.asarray(x), s, t, dev_dtype).get()
    assert got.dtype == out_dtype
    if not ac.same(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("scale_shift {} -> {} s={!r} t={!r}: {} of {} differ, e.g. {!r} -> {!r}, want {!r}".format(
            x.dtype, np.dtype(out_dtype).name, s, t, bad.size, got.size, x.ravel()[bad[0]].item(), got.ravel()[bad[0]].item(),
            want.ravel()[bad[0]].item()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_scale_shift_floats(gpu, S, dtype):
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.standard_normal(3000) * 100, rng.uniform(0, 1, 1000), [0.0, -0.0, 1.0, -1.0, 255.0, 1e-30, 3e30]]).astype(dtype)
    for s, t in [(1.0 / 255, 0.0), (2.0, -1.0), (0.1, 0.7), (-3.3, 1e-3), (1.0, 0.0), (65535.0, 0.5)]:
        _check_scale_shift(S, gpu, x, s, t, dtype)
    special = np.array([np.nan, np.inf, -np.inf], dtype)
    got = S.scale_shift(gpu.asarray(special), 2.0, 1.0).get()
    assert ac.same(got, special * dtype(2.0) + dtype(1.0))


@pytest.mark.parametrize("src", [np.bool_, np.int8, np.uint8, np.int16, np.uint16], ids=lambda d: np.dtype(d).name)
def test_scale_shift_fused_integer_to_float(gpu, S, src):
    src = np.dtype(src)
    if src.kind == "b":
        x = np.array([False, True] * 50)
        scales = [(1.0, 0.0), (0.25, 0.5)]
    else:
        info = np.iinfo(src)
        x = np.arange(info.min, info.max + 1, max(1, (info.max - info.min) // 5003)).astype(src)
        x = np.concatenate([x, ac.ladder(src)])
        scales = [(1.0 / info.max, 0.0), (1.0 / (info.max - info.min), 0.5), (2.0 / 65535, -1.0), (1.0, 0.0)]
    for out_dtype in (np.float32, np.float64):
        for s, t in scales:
            _check_scale_shift(S, gpu, x.reshape(-1, 1), s, t, out_dtype, dev_dtype=out_dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_clip(gpu, S, dtype):
    rng = np.random.default_rng(10)
    x = np.concatenate([rng.standard_normal(5000) * 2, [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.25, -7.0, 7.0, np.nan]]).astype(dtype)
    d = gpu.asarray(x)
    for lo, hi in [(0.0, 1.0), (-1.5, 0.25), (-7.0, 7.0), (0.3, 0.3)]:
        got = S.clip(d, lo, hi).get()
        want = np.clip(x, dtype(lo), dtype(hi))
        assert np.array_equal(np.isnan(got), np.isnan(x)), "clip({}, {}) turned NaN into {!r}".format(lo, hi, got[np.isnan(x)][0].item())
        assert ac.same(got, want), (lo, hi)
    got = S.clip(d, 0.0, 1.0).get()
    assert got[-9] == 1.0 and got[-8] == 0.0                        # +-inf clip to the bounds
    assert got[-7] == 0 and np.signbit(got[-7]) and not np.signbit(got[-6])         # -0.0 is inside [0, 1] and stays -0.0
    # keep: samples equal to it stay, inside or outside [lo, hi]; everything else is clipped
    for keep in (-7.0, 7.0, 0.25, 100.0):
        got = S.clip(d, 0.0, 1.0, keep).get()
        want = np.where(x == dtype(keep), x, np.clip(x, dtype(0), dtype(1)))
        assert ac.same(got, want), keep
    assert ac.same(S.clip(d, 0.0, 1.0, None).get(), np.clip(x, dtype(0), dtype(1)))
    # a strided input is compacted first
    assert ac.same(S.clip(gpu.asarray(np.repeat(x, 2))[::2], -1.0, 1.0).get(), np.clip(x, dtype(-1), dtype(1)))


def test_resize_and_warp_keep_nans_when_clipping(gpu):
    from cupyimg_amd.skimage import transform
    rng = np.random.default_rng(12)
    img = rng.uniform(10, 20, size=(40, 48)).astype(np.float32)
    img[12:20, 30:41] = np.nan
    lo, hi = np.nanmin(img), np.nanmax(img)
    d = gpu.asarray(img)
    theta = 0.1
    H = np.array([[np.cos(theta), -np.sin(theta), 2.0], [np.sin(theta), np.cos(theta), -1.5], [0, 0, 1]])
    calls = {
        "resize": lambda clip: transform.resize(d, (70, 90), order=1, anti_aliasing=False, clip=clip),
        "warp": lambda clip: transform.warp(d, H, order=1, mode="edge", clip=clip),
        "warp constant": lambda clip: transform.warp(d, H, order=1, mode="constant", cval=-5.0, clip=clip),
    }
    for name, call in calls.items():
        free = call(False).get()
        clipped = call(True).get()
        nan = np.isnan(free)
        assert nan.any() and not nan.all(), name
        lost = nan & ~np.isnan(clipped)
        assert not lost.any(), "{}: {} NaN samples became {!r} under clip=True".format(name, int(lost.sum()), clipped[lost][0].item())
        want = np.clip(free, lo, hi)
        if name == "warp constant":
            want = np.where(free == np.float32(-5.0), free, want)                 # cval outside the range marks the outside and stays
        assert ac.same(clipped, want.astype(clipped.dtype)), name


# ---------------------------------------------------------------- metrics
def _metric_inputs():
    rng = np.random.default_rng(14)
    cases = []
    base = rng.uniform(0, 1, size=(70, 70, 9)).astype(np.float32)
    noisy = (base + 0.05 * rng.standard_normal(base.shape)).astype(np.float32)
    cases.append(("(70, 70, 5) views", base, noisy, (Ellipsis, slice(2, 7))))
    a = rng.uniform(-1, 1, size=(4097, 64)).astype(np.float32)
    cases.append(("(4097, 64) float32", a, (a + 0.01 * rng.standard_normal(a.shape)).astype(np.float32), None))
    u8 = rng.integers(0, 256, size=(61, 67)).astype(np.uint8)
    i16 = (u8.astype(np.int16) + rng.integers(-9, 10, size=u8.shape)).astype(np.int16)
    cases.append(("uint8 / int16", u8, i16, None))
    cases.append(("int16 / uint8", i16 - np.int16(300), u8, None))
    f32 = rng.uniform(0, 1, size=(50, 60)).astype(np.float32)
    cases.append(("float32 / float64", f32, f32.astype(np.float64) + 0.02 * rng.standard_normal(f32.shape), None))
    cases.append(("float64 / float32", f32.astype(np.float64) * 0.5 + 0.1, f32, None))
    return cases


def _rel(n):
    """relative error of sum / n, or of its square root, for any summation order of n non-negative terms, with room for
    the handful of roundings that follow (division, square root, quotient): (n - 1) u + 8 u"""
    return (n + 7) * U * (1 + 2.0 ** -30)


def test_simple_metrics_against_float64(gpu, metrics):
    for name, a, b, cut in _metric_inputs():
        da, db = gpu.asarray(a), gpu.asarray(b)
        if cut is not None:
            a, b, da, db = a[cut], b[cut], da[cut], db[cut]
        ft = np.result_type(a.dtype, b.dtype, np.float32)           # the facade converts both to one float type first
        a64, b64 = a.astype(ft).astype(np.float64), b.astype(ft).astype(np.float64)
        n = a.size
        sq, _ = ac.sum_reference(1, a64, b64)
        mse = sq / n
        got = metrics.mean_squared_error(da, db)
        print("{}: mse rel err {:.3e}, bound {:.3e}".format(name, abs(got - mse) / mse, _rel(n)))
        assert abs(got - mse) <= _rel(n) * mse, (name, got, mse)
        # NRMSE = sqrt(mse) / denominator: the relative errors of both add (halved under the root, so _rel covers them)
        s2, _ = ac.sum_reference(2, a64)
        s0, s0mag = ac.sum_reference(0, a64)
        denoms = {"euclidean": (math.sqrt(s2 / n), _rel(n)),
                  "min-max": (float(a64.max() - a64.min()), 2 * U),
                  "mean": (s0 / n, ac.sum_bound(n, s0mag) / abs(s0) + 2 * U)}
        for norm, (den, den_rel) in denoms.items():
            want = math.sqrt(mse) / den
            got = metrics.normalized_root_mse(da, db, normalization=norm)
            bound = (_rel(n) + den_rel) * abs(want)
            print("{}: nrmse {} rel err {:.3e}, bound {:.3e}".format(name, norm, abs(got - want) / abs(want), bound / abs(want)))
            assert abs(got - want) <= bound, (name, norm, got, want)
        # PSNR = 10 log10(R^2 / mse): d/d(mse) = 10 / (ln 10 mse), plus a few ulps of the result for log10 and the product
        if a.dtype.kind == "f":
            rng_ = 1.0 if a64.min() >= 0 else 2.0
        else:
            info = np.iinfo(a.dtype)
            rng_ = float(info.max - info.min) if a64.min() < 0 else float(info.max)
        want = 10 * math.log10(rng_ ** 2 / mse)
        with pytest.warns(UserWarning) if a.dtype != b.dtype else _no_warning():
            got = metrics.peak_signal_noise_ratio(da, db)
        bound = 10 / math.log(10) * _rel(n) + 8 * U * abs(want)
        print("{}: psnr err {:.3e}, bound {:.3e}".format(name, abs(got - want), bound))
        assert abs(got - want) <= bound, (name, got, want)
        got = metrics.peak_signal_noise_ratio(da, db, data_range=3.5)
        assert abs(got - 10 * math.log10(3.5 ** 2 / mse)) <= bound + 8 * U * abs(got), name
    with pytest.raises(ValueError):
        metrics.normalized_root_mse(da, db, normalization="foo")
    with pytest.raises(ValueError):
        metrics.mean_squared_error(da, da[1:])


class _no_warning:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_ssim_of_4d_and_5d_images(gpu, metrics):
    rng = np.random.default_rng(15)
    for shape in [(10, 10, 10, 10), (6, 7, 8, 9, 10)]:
        x = (rng.random(shape) * 255).astype(np.uint8)
        y = np.clip(x + rng.normal(0, 20, shape), 0, 255).astype(np.uint8)
        want, wmap = _ssim_host(x, y, win_size=3)
        got, gmap = metrics.structural_similarity(gpu.asarray(x), gpu.asarray(y), win_size=3, full=True)
        assert abs(got - want) <= 1e-10, (shape, got, want)
        np.testing.assert_allclose(gmap.get(), wmap, rtol=1e-9, atol=1e-11)
        assert metrics.structural_similarity(gpu.asarray(x), gpu.asarray(y), win_size=3) == got


def test_ssim_gradient_of_a_volume(gpu, metrics):
    rng = np.random.default_rng(16)
    shape = (20, 24, 28)
    x = (rng.random(shape) * 255).astype(np.uint8)
    y = np.clip(x + rng.normal(0, 20, shape), 0, 255).astype(np.uint8)
    for kw in ({}, {"win_size": 3}):
        want, wmap, wgrad = _ssim_host(x, y, gradient=True, **kw)
        got, ggrad, gmap = metrics.structural_similarity(gpu.asarray(x), gpu.asarray(y), gradient=True, full=True, **kw)
        assert abs(got - want) <= 1e-10, kw
        np.testing.assert_allclose(gmap.get(), wmap, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(ggrad.get(), wgrad, rtol=1e-8, atol=1e-14)
