"""The yardstick of the array-layer tests (tests/helpers/array_cases.py) held against NumPy on the host: the expectations
the GPU tests assert are NumPy's own results wherever NumPy defines one, the float64 -> float16 witnesses tell one rounding
from two, the exactly summable arrays are exact, and every generated view stays inside its base.  No GPU."""
import math
import warnings

import numpy as np
import pytest

from helpers import array_cases as ac


def _sources(dtype):
    return ac.f16_all() if dtype == np.float16 else ac.ladder(dtype)


@pytest.mark.parametrize("src", ac.DTYPES, ids=str)
def test_admitted_casts_are_numpys(src):
    vals = _sources(src)
    for dst in ac.DTYPES:
        v = vals[ac.admitted(vals, dst)]
        assert v.size, (src, dst)
        want = ac.expected_cast(v, dst)
        assert want.dtype == dst and want.shape == v.shape
        wraps = np.zeros(v.shape, bool)
        if src.kind == "f" and dst.kind == "u":
            wraps = np.trunc(v.astype(np.float64)) < 0              # the rule of csrc/copy.hip; NumPy defines only some of these
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            if dst in (np.float16, np.float32):                     # a finite value beyond the narrower type's range becomes inf
                warnings.filterwarnings("ignore", message="overflow encountered in cast", category=RuntimeWarning)
            got = v[~wraps].astype(dst)                              # any other warning fails the test
        assert ac.same(got, want[~wraps]), (src, dst)
        # negative into unsigned: compared wherever NumPy casts without a warning (one value at a time)
        agreed = 0
        for x, w in zip(v[wraps][:4096], want[wraps][:4096]):
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                try:
                    g = np.array([x]).astype(dst)[0]
                except RuntimeWarning:
                    continue
            assert g == w, (src, dst, x, g, w)
            agreed += 1
        if wraps.any() and dst.itemsize >= 4:
            assert agreed, (src, dst)                                # wide targets: the hardware conversion is defined there


def test_admission_rule_edges():
    f = np.array([255.9, 256.0, -0.9, -1.0, -2.0 ** 63, -2.0 ** 62, np.nan, np.inf, 2.0 ** 63, 2.0 ** 64])
    assert ac.admitted(f, np.uint8).tolist() == [True, False, True, True, False, True, False, False, False, False]
    assert ac.admitted(f, np.int8).tolist() == [False, False, True, True, False, False, False, False, False, False]
    assert ac.admitted(f, np.int64).tolist() == [True, True, True, True, True, True, False, False, False, False]
    assert ac.admitted(f, np.uint64).tolist() == [True, True, True, True, False, True, False, False, True, False]
    assert ac.admitted(f, np.bool_).all() and ac.admitted(f, np.float16).all()
    assert ac.expected_cast(np.array([-1.5, -32769.0, 255.9]), np.uint8).tolist() == [255, 255, 255]
    assert ac.expected_cast(np.array([-1.0]), np.uint64).tolist() == [2 ** 64 - 1]
    assert ac.expected_cast(np.array([-(2.0 ** 63)]), np.int64).tolist() == [-2 ** 63]


def test_ladders_hold_the_listed_edges():
    assert ac.ladder(np.int8).tolist() == [-128, -127, -1, 0, 1, 126, 127]
    assert set(ac.ladder(np.uint64).tolist()) >= {0, 255, 2 ** 24 + 1, 2 ** 53 + 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1}
    assert set(ac.ladder(np.int64).tolist()) >= {-2 ** 63, -2 ** 63 + 1, -32769, 2 ** 53 + 1, 2 ** 63 - 2, 2 ** 63 - 1}
    for dt in (np.float16, np.float32, np.float64):
        lad = ac.ladder(dt)
        info = np.finfo(dt)
        assert np.isnan(lad).sum() == 1 and np.isinf(lad).sum() == 2
        for v in (info.max, -info.max, info.tiny, info.smallest_subnormal, 0.5, -2.5, 128, -129):
            assert (lad == dt(v)).any(), (dt, v)
        assert (np.signbit(lad) & (lad == 0)).sum() == 1                       # one -0.0
    f32 = ac.ladder(np.float32)
    assert (f32 == 2.0 ** 24).any() and not (f32.astype(np.float64) == 2.0 ** 24 + 1).any()
    f64 = ac.ladder(np.float64)
    beyond = float(np.finfo(np.float32).max) + 2.0 ** 103
    with np.errstate(over="ignore"):
        assert (f64 == beyond).any() and np.isinf(np.float32(beyond)) and np.isfinite(np.float32(np.nextafter(beyond, 0)))
    assert (f64 == 2.0 ** -150).any() and np.float32(2.0 ** -150) == 0 and np.float32(np.nextafter(2.0 ** -150, 1)) > 0
    assert ac.f16_all().view(np.uint16).tolist() == list(range(65536))


def test_f16_witnesses_discriminate():
    w = ac.f16_witnesses()
    for name in ("up", "down", "neg_up", "neg_down"):
        x = w[name]
        assert x.shape == (4096,) and np.isfinite(x).all()
        once = x.astype(np.float16).view(np.uint16)
        twice = x.astype(np.float32).astype(np.float16).view(np.uint16)
        assert (once != twice).sum() >= 1000, (name, int((once != twice).sum()))
    sub = w["subnormal"]
    assert (np.abs(sub) < 2.0 ** -14).all()
    assert (sub.astype(np.float16).view(np.uint16) != sub.astype(np.float32).astype(np.float16).view(np.uint16)).sum() >= 500
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="overflow encountered in cast", category=RuntimeWarning)
        top = w["top"].astype(np.float16)
        through32 = np.float32(65519.999).astype(np.float16)
    assert top[0] == 65504 and np.isinf(top[3]) and top[1] == 65504                # 65519.999 stays finite, 65520 overflows
    assert np.isinf(through32)                                                     # through float32 it is 65520 first


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=str)
def test_exact_arrays_sum_exactly(dtype):
    n = ac.EXACT_MAX_FLOAT_TERMS if dtype.kind == "f" else 2 ** 16
    a, b = ac.exact_array(dtype, (n,), 1), ac.exact_array(dtype, (n,), 2)
    assert a.dtype == dtype and not np.array_equal(a, b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for terms in (a64, (a64 - b64) ** 2, a64 * a64):
        exact = math.fsum(terms.tolist())
        fwd, rev = float(np.sum(terms)), float(np.sum(terms[::-1]))
        seq = float(np.cumsum(terms)[-1])                                         # plain left-to-right order
        assert fwd == exact and rev == exact and seq == exact
    for op in (0, 1, 2):
        assert ac.sum_reference(op, a, b)[0] == math.fsum(((a64, (a64 - b64) ** 2, a64 * a64)[op]).tolist())


def test_general_array_is_not_exact():
    x = ac.general_f64(20011, 3)
    exact, mag = ac.sum_reference(0, x)
    assert float(np.cumsum(x)[-1]) != exact                                        # a real rounding error to bound ...
    assert abs(float(np.cumsum(x)[-1]) - exact) <= ac.sum_bound(x.size, mag)       # ... and the bound holds for this order
    assert abs(float(np.sum(x)) - exact) <= ac.sum_bound(x.size, mag)


@pytest.mark.parametrize("shape", ac.RANK_SHAPES, ids=lambda s: "rank{}".format(len(s)))
def test_views_stay_inside_their_base(shape):
    names = set()
    for base_shape, view in ac.layouts(shape):
        base = np.zeros(base_shape, np.float32)
        v = view(base)
        names.add(view.name.split("@")[0])
        if view.name.startswith("newaxis"):
            assert v.ndim == len(shape) + 1 and v.size == int(np.prod(shape)) and tuple(s for s in v.shape if s != 1) == tuple(
                s for s in shape if s != 1)
        else:
            assert v.shape == tuple(shape), (view, v.shape)
        assert v.ndim <= ac.MAX_NDIM
        lo, hi = ac.view_extent(v, base)
        assert 0 <= lo and hi <= base.nbytes, (view, lo, hi, base.nbytes)
        assert np.shares_memory(v, base)
    want = {"contiguous"}
    if len(shape) >= 1:
        want |= {"step2", "reverse", "inner"}
    if len(shape) >= 2:
        want |= {"transposed", "rolled"}
    if len(shape) < ac.MAX_NDIM:
        want.add("newaxis")
    assert names == want
    assert [len(s) for s in ac.RANK_SHAPES] == list(range(9))
