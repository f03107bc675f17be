"""skimage.filters thresholding and the ordering operators of core.ndarray on the device (csrc/threshold.hip) against the
host references of tests/helpers/threshold_ref.py: the known answers of tests/golden/threshold_kat.json through the public
functions; the histogram methods bit for bit; the window statistics bit for bit on integer images (three routes: fused, fused
with small tiles, generic) and inside derived bounds on floats; Li's iteration; the multi-Otsu search; the comparisons against
NumPy; and one case of each kernel on poisoned pool memory."""
import ctypes
import math

import numpy as np
import pytest
from scipy import ndimage as sndi

from helpers import threshold_ref as R
from helpers.dirty_pool import FILLS, pool_fill
from test_threshold_yardstick import (INT_DTYPES, KAT_CASES, KAT_IDS, TIE_CASES, WINDOW_CASES, WINDOW_IDS, same_bits, seeded, tie_image)

pytestmark = pytest.mark.gpu

# (small tiles, forced generic route)
SETTINGS = [(0, 0), (1, 0), (0, 1)]
SETTING_IDS = ["planner", "small", "generic"]


@pytest.fixture(scope="module")
def F(gpu):
    from cupyimg_amd.skimage import filters
    return filters


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_threshold
    fn.argtypes = [ctypes.c_int] * 2
    yield fn
    fn(0, 0)


def host(v):
    return v.get() if hasattr(v, "get") and hasattr(v, "ptr") else v


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("case", KAT_CASES, ids=KAT_IDS)
def test_known_answers(gpu, F, case):
    image = R.kat_image(case["image"])
    fn = getattr(F, case["function"])
    R.check_expectation(case["expect"], lambda: host(fn(gpu.asarray(image), **case["kwargs"])), image)


# ---------------------------------------------------------------- histogram methods
def _same_outcome(fn, ref):
    """both raise the same error, or both return the same bits"""
    try:
        want = ref()
    except (RuntimeError, IndexError) as exc:
        with pytest.raises(type(exc)):
            fn()
        return
    got = fn()
    assert same_bits(got, want), (got, want)


def _bimodal(shape, dtype, seed):
    """two seeded modes (signed and float dtypes: one of them negative), the kind of image a threshold is asked of"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(shape) < 0.4, rng.normal(60, 12, size=shape), rng.normal(170, 20, size=shape))
    if dtype == "uint8":
        return np.clip(v, 0, 255).astype(np.uint8)
    if dtype == "int16":
        return ((v - 100) * 9).astype(np.int16)
    return ((v - 100) / 64).astype(dtype)


@pytest.mark.parametrize("nbins", [16, 256])
@pytest.mark.parametrize("shape", [(37, 41), (11, 12, 13)], ids=["37x41", "11x12x13"])
@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32", "float64"])
def test_histogram_methods_match_host_bit_for_bit(gpu, F, dtype, shape, nbins):
    image = _bimodal(shape, dtype, 11)
    if dtype == "int16":
        assert image.min() < 0
    x = gpu.asarray(image)
    counts, centers = R.exposure_ref.histogram(image, nbins, "image")
    methods = [(F.threshold_otsu, R.otsu, {}), (F.threshold_yen, R.yen, {}), (F.threshold_isodata, R.isodata, {}),
               (F.threshold_isodata, R.isodata, dict(return_all=True)), (F.threshold_minimum, R.minimum, {})]
    for fn, ref, kw in methods:
        _same_outcome(lambda: fn(x, nbins=nbins, **kw), lambda: ref(image, nbins=nbins, **kw))
        for hist in (counts, (counts, centers), (gpu.asarray(counts), gpu.asarray(centers))):
            _same_outcome(lambda: fn(hist=hist, **kw), lambda: ref(hist=(counts, centers) if isinstance(hist, tuple) else counts, **kw))
    _same_outcome(lambda: F.threshold_triangle(x, nbins=nbins), lambda: R.triangle(image, nbins=nbins))
    got = F.threshold_mean(x)
    want = R.mean(image)
    # any order of summation stays within (n - 1) u sum|x| of the exact sum: twice that over n separates two of them
    assert isinstance(got, np.float64) and abs(got - want) <= 2 * image.size * R.U * float(np.abs(image.astype(np.float64)).mean())


# ---------------------------------------------------------------- window statistics
def _three_routes(gpu, knob, shape, call, expect_fused=True):
    """the results of `call()` under the three settings, with the route each took checked; other ranks: one generic run"""
    if len(shape) not in (2, 3):
        out = call()
        assert "win_generic_kernel" in gpu.last_kernel(), gpu.last_kernel()
        return [out]
    outs = []
    for small, generic in SETTINGS:
        knob(small, generic)
        outs.append(call())
        name = gpu.last_kernel()
        if generic:
            assert "win_generic_kernel" in name, name
        else:
            assert "win_fused_kernel" in name, name
            if small:
                tile = [min(t, n) for t, n in zip((2 if len(shape) == 3 else 1, 3, 5), (1,) * (3 - len(shape)) + tuple(shape))]
                assert "tile={}x{}x{} ".format(*tile) in name, name
    knob(0, 0)
    return outs


@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("shape,w", WINDOW_CASES, ids=WINDOW_IDS)
def test_window_statistics_on_integers_match_integral_images_bit_for_bit(gpu, F, knob, shape, w, dtype):
    image = seeded(shape, dtype, 21) if dtype == "bool" else \
        np.random.default_rng(21).integers(np.iinfo(dtype).min, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    x = gpu.asarray(image)
    m, s = R.mean_std_integral(image, w)
    want = [m, s, R.niblack_from(m, s, 0.2), R.sauvola_from(m, s, 0.2, None, image.dtype), R.sauvola_from(m, s, 0.34, 77.0)]

    def call():
        md, sd = F._mean_std(x, w)
        return [md.get(), sd.get(), F.threshold_niblack(x, w).get(), F.threshold_sauvola(x, w).get(),
                F.threshold_sauvola(x, w, k=0.34, r=77.0).get()]
    for got in _three_routes(gpu, knob, shape, call):
        for g, t, what in zip(got, want, ("m", "s", "niblack", "sauvola", "sauvola r")):
            assert same_bits(g, t), what


@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32"])
def test_window_statistics_on_a_strided_view(gpu, F, knob, dtype):
    base = seeded((24, 70), dtype, 22)
    view = gpu.asarray(base)[3:21:2, 1:68]
    image = base[3:21:2, 1:68]
    m, s = R.mean_std_direct(image, (5, 7))
    for got_m, got_s in _three_routes(gpu, knob, image.shape, lambda: [a.get() for a in F._mean_std(view, (5, 7))]):
        if dtype == "float32":
            assert max(R.check_mean_std_bounds(image, (5, 7), got_m, got_s)) <= 1.0
        else:
            assert same_bits(got_m, m) and same_bits(got_s, s)


def _mixed_signs(shape, dtype, seed):
    return ((np.random.default_rng(seed).random(shape) - 0.5) * 2000).astype(dtype)


FLOAT_WINDOWS = [((13, 17), (5, 7)), ((9, 7), 15), ((5, 6, 7), 3), ((4, 5, 3, 3), 3)]


@pytest.mark.parametrize("signs", ["positive", "mixed"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,w", FLOAT_WINDOWS, ids=["13x17", "9x7-w15", "5x6x7", "4x5x3x3"])
def test_window_statistics_on_floats_meet_the_derived_bounds(gpu, F, knob, shape, w, dtype, signs):
    """|m_dev - m| <= gamma_n sum|x| / n + u |m|, |g2_dev - g2| <= gamma_(n+1) sum x^2 / n + u g2 and the bound on s^2 that
    follows (tests/helpers/threshold_ref.py check_mean_std_bounds), against exactly rounded rational window sums; the public
    thresholds are the formulas applied in float64 to the device's own m and s; and the three routes add a window's terms in
    one order, so they agree bit for bit"""
    image = seeded(shape, dtype, 23) if signs == "positive" else _mixed_signs(shape, dtype, 24)
    x = gpu.asarray(image)

    def call():
        md, sd = F._mean_std(x, w)
        return [md.get(), sd.get(), F.threshold_niblack(x, w, k=0.3).get(), F.threshold_sauvola(x, w, k=0.25, r=400.0).get()]
    outs = _three_routes(gpu, knob, shape, call)
    for m, s, nib, sau in outs:
        worst = R.check_mean_std_bounds(image, w, m, s)
        print("{} {} {} w={}: error / bound of m {:.3f}, of s^2 {:.3f}".format(dtype, signs, shape, w, *worst))
        assert same_bits(nib, R.niblack_from(m, s, 0.3)) and same_bits(sau, R.sauvola_from(m, s, 0.25, 400.0))
    for other in outs[1:]:
        assert all(same_bits(a, b) for a, b in zip(outs[0], other))


def test_window_statistics_float16_and_wide_integers(gpu, F):
    """float16 is read as astype(float64) reads it; 32- and 64-bit integers take the float64 sums (exact below 2^53)"""
    img16 = seeded((12, 19), "float32", 25).astype(np.float16)
    m, s = F._mean_std(gpu.asarray(img16), 5)
    want = F._mean_std(gpu.asarray(img16.astype(np.float64)), 5)
    assert same_bits(m.get(), want[0].get()) and same_bits(s.get(), want[1].get())
    for dtype in ("int32", "uint32", "int64"):
        image = np.random.default_rng(26).integers(0, 100000, size=(12, 19)).astype(dtype)
        mi, si = R.mean_std_integral(image, (3, 5))
        m, s = F._mean_std(gpu.asarray(image), (3, 5))
        assert same_bits(m.get(), mi) and same_bits(s.get(), si)


# ---------------------------------------------------------------- Li
@pytest.mark.parametrize("dtype,shape", [("uint8", (37, 41)), ("int16", (11, 12, 13)), ("uint16", (64, 64)), ("int32", (37, 41))],
                         ids=["uint8", "int16-negative", "uint16", "int32-sorted-tolerance"])
def test_li_on_integers_matches_host_bit_for_bit(gpu, F, dtype, shape):
    rng = np.random.default_rng(31)
    if dtype == "int32":        # a range above the histogram's bin limit: the tolerance comes from the sort and the gap reduction
        image = (rng.integers(0, 2 ** 20, size=shape) * 173 - 2 ** 26).astype(dtype)
    else:
        image = np.clip(rng.normal(90, 30, size=shape) + (rng.random(shape) < 0.3) * 110, 0, 255).astype(dtype)
        if dtype == "int16":
            image = (image.astype(np.int16) - 128) * 57
    want_seq, got_seq = [], []
    want = R.li(image, iter_callback=want_seq.append)
    got = F.threshold_li(gpu.asarray(image), iter_callback=got_seq.append)
    assert isinstance(got, np.float64) and same_bits(got, want)
    assert len(got_seq) == len(want_seq) >= 2 and all(same_bits(np.float64(a), np.float64(b)) for a, b in zip(got_seq, want_seq))
    # an explicit tolerance and a scalar initial guess
    guess = float(np.percentile(image, 80))
    assert same_bits(F.threshold_li(gpu.asarray(image), tolerance=0.25, initial_guess=guess), R.li(image, tolerance=0.25, initial_guess=guess))
    with pytest.raises(ValueError, match="within the range"):
        F.threshold_li(gpu.asarray(image), initial_guess=float(image.min()) - 5)


def _li_float_image(dtype, seed, mixed):
    """values on a grid of 1 / 10 (none of them a float the dtype holds exactly, so every sum rounds), so that the default
    tolerance, half the smallest gap, is about 0.05: far above the rounding noise"""
    rng = np.random.default_rng(seed)
    v = np.clip(rng.normal(300, 90, size=(48, 50)) + (rng.random((48, 50)) < 0.35) * 420, 0, 999)
    v = np.round(v * 10) - (5000 if mixed else 0)
    return (v / 10).astype(dtype)


@pytest.mark.parametrize("mixed", [False, True], ids=["positive", "mixed-signs"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_li_on_floats(gpu, F, dtype, mixed):
    """against the reference with exactly rounded (math.fsum) means; the device may deviate four times as far as the pairwise
    NumPy means do, at least 16 ulp of the threshold: both are legitimate orders of summation"""
    image = _li_float_image(dtype, 32, mixed)
    image[3, 4] = np.nan
    image[5, 6] = np.inf
    image[7, 8] = -np.inf
    trace, want_seq, got_seq = [], [], []
    want = R.li(image, mean_fn=R.fsum_mean, trace=trace, iter_callback=want_seq.append)
    plain = R.li(image, mean_fn=R.numpy_mean)
    finite = image[np.isfinite(image)]
    tol = float(np.diff(np.unique(finite - finite.min())).min()) / 2
    for t_curr, t_next in trace:
        assert abs(abs(t_next - t_curr) - tol) > 1e-9 * tol          # no iterate decides the loop within rounding noise
    got = F.threshold_li(gpu.asarray(image), iter_callback=got_seq.append)
    allowed = max(4 * abs(plain - want), 16 * np.spacing(abs(want)))
    print("{} {}: numpy - fsum {:.3e}, device - fsum {:.3e}, allowed {:.3e}, {} iterations".format(
        dtype, "mixed" if mixed else "positive", plain - want, got - want, allowed, len(want_seq)))
    assert len(got_seq) == len(want_seq)
    assert abs(got - want) <= allowed
    # reproducible bit for bit
    assert same_bits(F.threshold_li(gpu.asarray(image)), got)


def test_li_callable_initial_guess(gpu, F):
    image = _li_float_image("float32", 33, False)
    seen = []

    def guess(arr):
        seen.append((arr.shape, arr.dtype))
        return float(np.quantile(arr.get(), 0.9))
    got = F.threshold_li(gpu.asarray(image), initial_guess=guess)
    trace = []
    want = R.li(image, initial_guess=lambda v: float(np.quantile(v, 0.9)), mean_fn=R.fsum_mean, trace=trace)
    tol = float(np.diff(np.unique(image - image.min())).min()) / 2
    assert all(abs(abs(b - a) - tol) > 1e-9 * tol for a, b in trace)
    assert seen == [((image.size,), np.dtype("float32"))]
    assert abs(got - want) <= 1e-9 * abs(want)
    with pytest.raises(TypeError):
        F.threshold_li(gpu.asarray(image), initial_guess="mean")


# ---------------------------------------------------------------- multi-Otsu
def _multiotsu_case(gpu, F, image, classes, nbins):
    prob, _ = R.exposure_ref.histogram(image, nbins, "image", normalize=True)
    tup, best, second = R.multiotsu_brute(prob, classes, runner_up=True)
    assert best - second > 1e-9 * best, (best, second)               # a clear winner: no rounding decides it
    got = F.threshold_multiotsu(gpu.asarray(image), classes=classes, nbins=nbins)
    want = R.multiotsu(image, classes, nbins)
    assert isinstance(got, np.ndarray) and same_bits(got, want), (got, want)


@pytest.mark.parametrize("classes", [2, 3, 4])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_multiotsu_matches_brute_force(gpu, F, dtype, classes):
    rng = np.random.default_rng(41)
    modes = rng.choice([20.0, 38.0, 55.0, 71.0, 84.0], size=(37, 41)) + rng.normal(0, 3.5, size=(37, 41))
    image = np.clip(modes, 10, 89).astype(dtype)                      # 80 bins for uint8
    _multiotsu_case(gpu, F, image, classes, 48)


def test_multiotsu_five_classes_on_sixteen_bins(gpu, F):
    rng = np.random.default_rng(42)
    image = (rng.choice([0.1, 0.3, 0.5, 0.7, 0.9], size=(37, 41)) + rng.normal(0, 0.03, size=(37, 41))).astype(np.float32)
    _multiotsu_case(gpu, F, image, 5, 16)


def _sparse_uint16():
    """four narrow clusters across the whole uint16 range: almost every one of the 65536 bins is empty"""
    rng = np.random.default_rng(43)
    base = rng.choice([0, 20000, 45000, 65485], size=(64, 64), p=[0.3, 0.25, 0.2, 0.25])
    image = (base + rng.integers(0, 51, size=(64, 64))).astype(np.uint16)
    image[0, :2] = (0, 65535)
    return image


def test_multiotsu_two_classes_on_65536_bins(gpu, F):
    """the threads of 16 workgroups walk the one threshold; every threshold inside a run of empty bins cuts the image the same
    way and scores the same bits, and the smallest of them is returned"""
    image = _sparse_uint16()
    prob, centers = R.exposure_ref.histogram(image, 256, "image", normalize=True)
    assert prob.size == 65536
    cp, cs = R.multiotsu_tables(prob)
    u = np.arange(prob.size - 1)
    vals = (0.0 + R._term(cp, cs, 0, u)) + R._term(cp, cs, u + 1, prob.size - 1)
    best = vals.max()
    assert (vals == best).sum() > 1000 and best - vals[vals < best].max() > 1e-9 * best      # one best cut, clear of the next
    got = F.threshold_multiotsu(gpu.asarray(image), classes=2)
    assert same_bits(got, centers[[int(np.argmax(vals))]])
    assert same_bits(got, R.multiotsu(image, 2))


@pytest.mark.parametrize("counts,classes,pair", TIE_CASES, ids=["tie-{}bins-{}classes".format(len(c), k) for c, k, _ in TIE_CASES])
def test_multiotsu_exact_tie_returns_the_smaller_tuple(gpu, F, counts, classes, pair):
    got = F.threshold_multiotsu(gpu.asarray(tie_image(counts)), classes=classes)
    assert got.tolist() == list(min(pair))


# ---------------------------------------------------------------- comparisons
REAL_DTYPES = ["bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float16", "float32", "float64"]
OPS = [("gt", lambda a, b: a > b), ("ge", lambda a, b: a >= b), ("lt", lambda a, b: a < b), ("le", lambda a, b: a <= b)]


def _compare_values(dtype, n=131):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(51)
    if dtype.kind == "f":
        v = rng.normal(0, 3, size=n).astype(dtype)
        v[:8] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, 0.5, -2.0]
        return v
    if dtype == np.bool_:
        return rng.random(n) < 0.5
    info = np.iinfo(dtype)
    v = rng.integers(max(info.min, -6), min(info.max, 6) + 1, size=n).astype(dtype)
    v[:4] = [info.min, info.max, 0, 3]
    return v


def _scalars(dtype):
    dtype = np.dtype(dtype)
    out = [0, 3, -1, 300, 2 ** 63, -2 ** 70, 2 ** 70, 0.0, -0.0, 0.5, 2.5, 3.0, float("nan"), float("inf"), -float("inf"), 0.1,
           np.uint8(3), np.int8(-1), np.int64(-3), np.uint64(2 ** 63), np.float32(0.1), np.float64(0.1), np.float16(0.5), np.float32(3.0),
           np.bool_(True), True]
    return out


@pytest.mark.parametrize("dtype", REAL_DTYPES)
def test_comparisons_match_numpy(gpu, dtype):
    values = _compare_values(dtype)
    x = gpu.asarray(values)
    launched = []
    with np.errstate(all="ignore"):
        for name, op in OPS:
            for scalar in _scalars(dtype):
                try:
                    want = op(values, scalar)
                except OverflowError:
                    continue                                      # NumPy refuses: an integer no float of this width holds
                got = op(x, scalar)
                launched.append(gpu.last_kernel())
                assert got.dtype == np.bool_ and got.shape == values.shape and got.flags.c_contiguous
                assert np.array_equal(got.get(), want), (name, dtype, scalar, type(scalar))
            # the reflected forms Python derives from them
            assert np.array_equal((3 < x).get(), 3 < values) and np.array_equal((0.5 >= x).get(), 0.5 >= values)
            for other in REAL_DTYPES:
                b = _compare_values(other)[::-1].copy()
                got = op(x, gpu.asarray(b))
                assert np.array_equal(got.get(), op(values, b)), (name, dtype, other)
    assert all("cmp_scalar_kernel" in k and "one launch" in k for k in launched)


def test_comparisons_take_strided_and_shaped_operands(gpu):
    base = np.random.default_rng(52).normal(size=(12, 14, 9)).astype(np.float32)
    other = np.random.default_rng(53).integers(-2, 3, size=(12, 14, 9)).astype(np.int16)
    x, y = gpu.asarray(base), gpu.asarray(other)
    for name, op in OPS:
        assert np.array_equal(op(x[1:11:3, ::2], 0.1).get(), op(base[1:11:3, ::2], 0.1))
        assert np.array_equal(op(x.transpose(2, 0, 1), y.transpose(2, 0, 1)).get(), op(base.transpose(2, 0, 1), other.transpose(2, 0, 1)))
        assert np.array_equal(op(x[:, 3:, 1:], y[:, 3:, 1:]).get(), op(base[:, 3:, 1:], other[:, 3:, 1:]))      # a misaligned first sample
        assert np.array_equal(op(y.reshape(-1)[1:], 1).get(), op(other.reshape(-1)[1:], 1))
    with pytest.raises(ValueError):
        x > y[:5]
    with pytest.raises(TypeError):
        x > "text"
    assert (gpu.asarray(np.zeros((0, 3), np.uint8)) > 1).shape == (0, 3)


def test_segment_label_end_to_end(gpu, F):
    """label(image > threshold_otsu(image)) with no host round trip of the image"""
    from cupyimg_amd.scipy import ndimage as ndi
    rng = np.random.default_rng(54)
    image = sndi.gaussian_filter(rng.random((64, 64)), 3.0)
    image = ((image - image.min()) / (image.max() - image.min()) * 255).astype(np.uint8)
    x = gpu.asarray(image)
    t = F.threshold_otsu(x)
    assert same_bits(t, R.otsu(image))
    labels, count = ndi.label(x > t)
    want, want_count = sndi.label(image > R.otsu(image))
    assert int(count) == want_count > 1 and np.array_equal(labels.get(), want)


# ---------------------------------------------------------------- poisoned pool
def _poisoned(gpu, inputs, call):
    """the host results of `call(*device inputs)` under every fill byte (the inputs are uploaded before the knob goes on)"""
    dev = [gpu.asarray(a) for a in inputs]
    gpu.synchronize()
    outs = []
    for byte in FILLS:
        with pool_fill(gpu, byte):
            outs.append(call(*dev))
    return outs


def test_poisoned_pool_niblack_fused_and_generic(gpu, F, knob):
    image = np.random.default_rng(61).integers(0, 65536, size=(11, 12, 13)).astype(np.uint16)
    want = R.niblack(image, (5, 3, 7), 0.2)
    for setting, route in (((0, 0), "win_fused_kernel"), ((0, 1), "win_generic_kernel")):
        knob(*setting)
        for got in _poisoned(gpu, [image], lambda x: (F.threshold_niblack(x, (5, 3, 7)).get(), gpu.last_kernel())):
            assert route in got[1] and same_bits(got[0], want)


def test_poisoned_pool_li_multiotsu_and_comparison(gpu, F):
    rng = np.random.default_rng(62)
    image = np.clip(rng.choice([30.0, 60.0, 85.0], size=(37, 41)) + rng.normal(0, 4, size=(37, 41)), 10, 99).astype(np.uint8)
    want_li, want_mo = R.li(image), R.multiotsu(image, 3)
    for got in _poisoned(gpu, [image], lambda x: (F.threshold_li(x), F.threshold_multiotsu(x, 3), (x > 57.5).get(), (x <= x).get())):
        assert same_bits(got[0], want_li) and same_bits(got[1], want_mo)
        assert np.array_equal(got[2], image > 57.5) and got[3].all()
