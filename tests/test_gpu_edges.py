"""skimage.filters' edge operators, apply_hysteresis_threshold and feature.canny on the device (csrc/edges.hip) against the host
transcription of tests/helpers/edges_ref.py, bit for bit, under the three settings of mi_debug_set_edges (the planner's boxes,
small boxes with seams along every axis, the forced unfused composition), the route read back from last_kernel(); the known
answers of tests/golden/edges_kat.json; and the Canny cases tests/test_edges_yardstick.py admitted."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from helpers import edges_ref as R
from test_edges_yardstick import KAT, check_canny_case, check_edge_case

pytestmark = pytest.mark.gpu

# (small tiles, forced composition)
SETTINGS = [(0, 0), (1, 0), (0, 1)]
SETTING_IDS = ["planner", "small", "generic"]
MODES = ["reflect", "constant", "nearest", "mirror", "wrap", "grid-wrap", "grid-constant", "grid-mirror"]
NAMES = ["sobel", "scharr", "prewitt"]
CVAL = 0.37


@pytest.fixture(scope="module")
def filters(gpu):
    from cupyimg_amd.skimage import filters
    return filters


@pytest.fixture(scope="module")
def feature(gpu):
    from cupyimg_amd.skimage import feature
    return feature


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_edges
    fn.argtypes = [ctypes.c_int] * 2
    yield fn
    fn(0, 0)


def same_bits(got, want):
    """equal bit for bit, the sign of zeros included; a NaN matches a NaN (the sign and payload of a generated NaN are the
    processor's)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    view = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(view)[~nan], np.ascontiguousarray(want).view(view)[~nan])


def _edge_route(name, shape, dtype, setting):
    """does last_kernel() name the route this setting must take?"""
    tname = "float32" if np.dtype(dtype) == np.float32 else "float64"
    if setting[1] or len(shape) not in (2, 3):
        return "edge_generic<{}>".format(tname) in name and "rank {}".format(len(shape)) in name
    full = (1,) * (3 - len(shape)) + tuple(shape)
    if setting[0]:
        box = (2 if len(shape) == 3 else 1, 3, 5)
    else:
        box = ((8 if tname == "float32" else 4) if len(shape) == 3 else 1, 8 if len(shape) == 3 else 32, 64)
    box = tuple(min(b, n) for b, n in zip(box, full))
    return "edge_fused_kernel<{},{}>".format(tname, len(shape)) in name and "box={}x{}x{} ".format(*box) in name


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


SHAPES = [(12, 20, 70), (9, 37, 64), (33, 18, 257), (3, 3, 3), (1, 5, 9), (2, 5, 1040), (70, 96), (5, 1040), (2, 2), (1, 7), (17,), (5, 6, 7, 8)]
DTYPES = ["float32", "float64", "uint8", "int16"]


@functools.lru_cache(maxsize=None)
def _image(shape, dtype):
    rng = np.random.RandomState(len(shape) * 1000 + int(np.prod(shape)) % 997)
    if np.dtype(dtype).kind == "f":
        image = (rng.uniform(size=shape) * 4 - 1).astype(dtype)
    else:
        info = np.iinfo(dtype)
        image = rng.randint(info.min, info.max + 1, size=shape).astype(dtype)
    image.setflags(write=False)
    return image


@functools.lru_cache(maxsize=None)
def _mask(shape):
    """a mask that touches the border: the first samples along every axis stay true"""
    mask = np.random.RandomState(11).uniform(size=shape) > 0.04
    mask[tuple(slice(0, 2) for _ in shape)] = True
    mask.setflags(write=False)
    return mask


@functools.lru_cache(maxsize=None)
def _want(name, shape, dtype, axis, mode, masked):
    """the transcription's result, computed once and shared by the three settings"""
    out = R.edge(name, _image(shape, dtype), _mask(shape) if masked else None, axis=axis, mode=mode, cval=CVAL)
    out.setflags(write=False)
    return out


def _float_dtype(dtype):
    return dtype if np.dtype(dtype).kind == "f" else "float64"


def _takes_fma(name, dtype, shape, setting, cval_is_float32=True):
    """the fused kernel's multiply-add instance: float32 samples, weights that are float32 values (not Prewitt's 1 / 3) and,
    where cval enters, a cval that is one"""
    return (np.dtype(dtype) == np.float32 and name != "prewitt" and cval_is_float32 and not setting[1] and len(shape) in (2, 3))


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_magnitude_in_every_mode_matches_host_bit_for_bit(gpu, filters, knob, shape, dtype, setting):
    """every operator in every mode; CVAL is not a float32 value, so 'constant' takes the instance without multiply-adds"""
    knob(*setting)
    x = gpu.asarray(_image(shape, dtype))
    for mode in MODES:
        for name in NAMES:
            got = getattr(filters, name)(x, mode=mode, cval=CVAL)
            kernel = gpu.last_kernel()
            assert _edge_route(kernel, shape, _float_dtype(dtype), setting), (kernel, mode)
            assert (" fma " in kernel) == _takes_fma(name, dtype, shape, setting, "constant" not in mode), (kernel, name, mode)
            assert got.dtype == np.float64
            assert same_bits(got.get(), _want(name, shape, dtype, None, mode, False)), (name, mode)


FMA_SHAPES = [(12, 20, 70), (33, 18, 257), (3, 3, 3), (70, 96), (5, 1040), (2, 2)]


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("cval", [0.0, 0.5, -3.25])
@pytest.mark.parametrize("shape", FMA_SHAPES, ids=_ids(FMA_SHAPES))
def test_constant_mode_with_a_float32_cval_matches_host_bit_for_bit(gpu, filters, knob, shape, cval, setting):
    """what sobel / scharr on a float32 image with mode='constant' and the default cval run: the constant-mode instance with
    multiply-adds (the products with cval are exact too); prewitt and float64 beside it on the instance without"""
    knob(*setting)
    for dtype in ("float32", "float64"):
        image = _image(shape, dtype)
        x = gpu.asarray(image)
        for name in NAMES:
            for mode in ("constant", "grid-constant"):
                for axis in (None, len(shape) - 1):
                    got = getattr(filters, name)(x, axis=axis, mode=mode, cval=cval)
                    kernel = gpu.last_kernel()
                    assert _edge_route(kernel, shape, dtype, setting), kernel
                    assert (" fma " in kernel) == _takes_fma(name, dtype, shape, setting), (kernel, name)
                    assert same_bits(got.get(), R.edge(name, image, axis=axis, mode=mode, cval=cval)), (name, dtype, mode, axis)


def _axes_of(shape):
    axes = [None, 0, -1]
    if len(shape) >= 2:
        axes += [len(shape) - 2, (0, len(shape) - 1), [1]]
    return axes


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_axes_and_masks_match_host_bit_for_bit(gpu, filters, knob, shape, dtype, setting):
    """axis None, an int, a negative int, a 2-tuple (the magnitude, divided by the rank) and a 1-list (signed), with and
    without a mask that touches the border"""
    knob(*setting)
    x = gpu.asarray(_image(shape, dtype))
    mask = gpu.asarray(_mask(shape))
    for i, axis in enumerate(_axes_of(shape)):
        key = tuple(axis) if isinstance(axis, (list, tuple)) else axis
        for masked in (False, True):
            name = NAMES[(i + masked) % 3]
            mode = ("reflect", "mirror", "constant")[i % 3]
            want = R.edge(name, _image(shape, dtype), _mask(shape) if masked else None, axis=axis, mode=mode, cval=CVAL)
            got = getattr(filters, name)(x, mask if masked else None, axis=axis, mode=mode, cval=CVAL)
            assert _edge_route(gpu.last_kernel(), shape, dtype, setting), gpu.last_kernel()
            assert same_bits(got.get(), want), (name, key, masked)


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [(9, 37, 64), (70, 96), (17,)], ids=_ids([(9, 37, 64), (70, 96), (17,)]))
def test_nonfinite_inputs_match_host(gpu, filters, knob, shape, dtype, setting):
    """NaN, inf and -0.0 in the image: zero weights are skipped (inf * 0 never appears), -x * 0 of the mask stays -0.0"""
    knob(*setting)
    image = _image(shape, dtype).copy()
    flat = image.reshape(-1)
    flat[3], flat[flat.size // 2], flat[-2], flat[5:9] = np.nan, np.inf, -np.inf, -0.0
    x = gpu.asarray(image)
    for name in NAMES:
        for axis, masked in ((None, False), (0, True), (None, True)):
            want = R.edge(name, image, _mask(shape) if masked else None, axis=axis)
            got = getattr(filters, name)(x, gpu.asarray(_mask(shape)) if masked else None, axis=axis)
            assert same_bits(got.get(), want), (name, axis, masked)


def test_views_host_inputs_repeatability_and_untouched_inputs(gpu, filters):
    base = np.random.RandomState(3).uniform(size=(14, 40, 80)).astype(np.float32)
    dev = gpu.asarray(base)
    view, hview = dev[1:13:2, 3:, 5:75], base[1:13:2, 3:, 5:75]
    want = R.edge("sobel", np.ascontiguousarray(hview))
    got = filters.sobel(view)
    assert same_bits(got.get(), want)
    assert filters.sobel(view).get().tobytes() == got.get().tobytes()
    assert same_bits(filters.sobel(np.ascontiguousarray(hview)).get(), want)              # a host array
    assert same_bits(filters.sobel(hview.tolist()).get(), R.edge("sobel", np.asarray(hview.tolist())))
    assert np.array_equal(dev.get(), base)
    t = dev[0].T                                                                           # a transposed image
    assert same_bits(filters.scharr(t, axis=1).get(), R.edge("scharr", np.ascontiguousarray(base[0].T), axis=1))
    half = gpu.asarray(base[0].astype(np.float16))                                         # float16: computed in float32
    assert same_bits(filters.prewitt(half).get(), R.edge("prewitt", base[0].astype(np.float16)))
    mask = np.ones(base.shape, bool)
    mask[4] = False
    mdev = gpu.asarray(mask)
    assert same_bits(filters.sobel(dev, mdev).get(), R.edge("sobel", base, mask))
    assert np.array_equal(mdev.get(), mask) and np.array_equal(dev.get(), base)
    assert same_bits(filters.sobel(dev, mode=["mirror"] * 3).get(), R.edge("sobel", base, mode="mirror"))


IMAGES = [(70, 96), (5, 1040), (2, 2)]


@pytest.mark.parametrize("dtype", ["float32", "float64", "uint8"])
@pytest.mark.parametrize("shape", IMAGES, ids=_ids(IMAGES))
def test_fixed_weight_operators_match_host_bit_for_bit(gpu, filters, shape, dtype):
    image = _image(shape, dtype)
    x, mask = gpu.asarray(image), gpu.asarray(_mask(shape))
    fdt = np.dtype(_float_dtype(dtype))
    for name in ("roberts", "roberts_pos_diag", "roberts_neg_diag"):
        got = getattr(filters, name)(x)
        assert got.dtype == fdt and same_bits(got.get(), getattr(R, name)(image)), name
        assert same_bits(getattr(filters, name)(x, mask).get(), getattr(R, name)(image, _mask(shape))), name
    for name in ("farid", "farid_h", "farid_v"):
        got = getattr(filters, name)(x)
        assert got.dtype == fdt and same_bits(got.get(), getattr(R, name)(image)), name
        assert same_bits(getattr(filters, name)(x, mask=mask).get(), getattr(R, name)(image, _mask(shape))), name
    for name in NAMES:
        for suffix, axis in (("_h", 0), ("_v", 1)):
            got = getattr(filters, name + suffix)(x, mask)
            assert got.dtype == np.float64 and same_bits(got.get(), R.edge(name, image, _mask(shape), axis=axis)), name + suffix


LAPLACE_SHAPES = [(70, 96), (5, 1040), (2, 2), (17,), (9, 10, 33)]


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("shape", LAPLACE_SHAPES, ids=_ids(LAPLACE_SHAPES))
def test_laplace_matches_host_bit_for_bit(gpu, filters, shape, ksize):
    for dtype in ("float32", "float64", "int16"):
        image = _image(shape, dtype)
        got = filters.laplace(gpu.asarray(image), ksize=ksize)
        assert got.dtype == np.dtype(_float_dtype(dtype)) and same_bits(got.get(), R.laplace(image, ksize)), dtype
        assert same_bits(filters.laplace(gpu.asarray(image), ksize, gpu.asarray(_mask(shape))).get(), R.laplace(image, ksize, _mask(shape)))


def _funcs(filters):
    def host(fn):
        return lambda image, *a, **k: fn(image, *a, **k).get()
    return {n: host(getattr(filters, n)) for n in ("sobel", "scharr", "prewitt", "roberts", "farid", "laplace", "roberts_pos_diag",
                                                    "roberts_neg_diag", "farid_h", "farid_v", "sobel_h", "sobel_v", "scharr_h", "scharr_v",
                                                    "prewitt_h", "prewitt_v")}


@pytest.mark.parametrize("case", KAT["edges"], ids=[c["name"] for c in KAT["edges"]])
def test_edge_known_answers(gpu, filters, case):
    funcs = _funcs(filters)
    funcs["farid"] = lambda image, mask=None: filters.farid(image, mask=mask).get()
    funcs["farid_h"] = lambda image, mask=None: filters.farid_h(image, mask=mask).get()
    funcs["farid_v"] = lambda image, mask=None: filters.farid_v(image, mask=mask).get()
    funcs["laplace"] = lambda image, mask=None: filters.laplace(image, 3, mask).get()
    check_edge_case(case, funcs)


# ---------------------------------------------------------------- hysteresis
def _serpentine(n=64):
    """a one-pixel path that snakes through the image: its geodesic length (about n * n / 2) far exceeds one block"""
    image = np.zeros((n, n))
    for r in range(0, n, 2):
        image[r, :] = 0.5
        if r + 1 < n:
            image[r + 1, -1 if (r // 2) % 2 == 0 else 0] = 0.5
    image[0, 0] = 1.0
    return image


def _device_label_formulation(gpu, image, low, high):
    """the components of the low mask that hold a sample of the high mask, by this library's label and sum_labels"""
    from cupyimg_amd.scipy import ndimage as ndi
    mask_low, mask_high = R.threshold_masks(image, low, high)
    labels, count = ndi.label(gpu.asarray(mask_low))
    index = np.arange(1, count + 1)
    hits = np.asarray(ndi.sum_labels(gpu.asarray(mask_high.astype(np.float64)), labels, index).get())
    return np.isin(labels.get(), index[hits > 0])


@pytest.mark.parametrize("shape", [(300,), (64, 70), (12, 20, 33)], ids=_ids([(300,), (64, 70), (12, 20, 33)]))
def test_hysteresis_matches_host_and_the_label_formulation(gpu, filters, shape):
    from scipy import ndimage as sndi
    rng = np.random.RandomState(21)
    image = sndi.gaussian_filter(rng.uniform(size=shape), 1.0)
    low, high = (float(v) for v in np.quantile(image, [0.45, 0.8]))
    cases = [(image, low, high), (image.astype(np.float32), low, high), (image, high, low),                   # low > high: clipped
             (image, np.full(shape, low) + 0.01 * rng.uniform(size=shape), high), (image, low, np.full(shape, high)),
             ((image * 255).astype(np.uint8), low * 255, high * 255)]
    for im, lo, hi in cases:
        want = R.apply_hysteresis_threshold(im, lo, hi)
        got = filters.apply_hysteresis_threshold(gpu.asarray(im), lo, hi)
        assert got.dtype == np.bool_ and np.array_equal(got.get(), want)
        assert 0 < want.sum() < want.size
    assert np.array_equal(filters.apply_hysteresis_threshold(gpu.asarray(image), gpu.asarray(cases[3][1]), high).get(),
                          R.apply_hysteresis_threshold(image, cases[3][1], high))
    # both thresholds as device arrays (float32 and float64), the low one above the high one in places: clipped in the launch
    low_a = (np.full(shape, low) + 0.3 * (rng.uniform(size=shape) > 0.7)).astype(np.float32)
    high_a = np.full(shape, high) + 0.02 * rng.uniform(size=shape)
    assert (low_a > high_a).any() and (low_a < high_a).any()
    want = R.apply_hysteresis_threshold(image, low_a, high_a)
    assert 0 < want.sum() < want.size
    assert np.array_equal(filters.apply_hysteresis_threshold(gpu.asarray(image), gpu.asarray(low_a), gpu.asarray(high_a)).get(), want)
    assert np.array_equal(filters.apply_hysteresis_threshold(gpu.asarray(image), low_a, gpu.asarray(high_a)).get(), want)
    with pytest.raises(ValueError):
        filters.apply_hysteresis_threshold(gpu.asarray(image), gpu.asarray(low_a.reshape(-1)[:7]), high)
    assert np.array_equal(_device_label_formulation(gpu, image, low, high), R.apply_hysteresis_threshold(image, low, high))


def test_hysteresis_edge_cases(gpu, filters):
    image = _serpentine()
    want = R.apply_hysteresis_threshold(image, 0.25, 0.75)
    assert want.sum() == (image > 0).sum() > 2000
    assert np.array_equal(filters.apply_hysteresis_threshold(image, 0.25, 0.75).get(), want)            # a host image
    assert np.array_equal(filters.apply_hysteresis_threshold(gpu.asarray(image), 0.25, 2.0).get(), np.zeros(image.shape, bool))   # nothing above high
    assert np.array_equal(filters.apply_hysteresis_threshold(gpu.asarray(image), -1.0, -0.5).get(), np.ones(image.shape, bool))   # full masks
    assert not filters.apply_hysteresis_threshold(gpu.asarray(image), 5.0, 6.0).get().any()               # both masks empty
    example = np.array([1, 2, 3, 2, 1, 2, 1, 3, 2])                                                      # the docstring's example
    assert filters.apply_hysteresis_threshold(gpu.asarray(example), 1.5, 2.5).get().astype(int).tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 1]


# ---------------------------------------------------------------- canny
CANNY_SHAPES = [(70, 96), (37, 131), (5, 1040), (3, 3), (2, 9), (64, 70)]


def _canny_route(name, shape, setting, masks):
    if setting[1]:
        return "canny_generic_kernel" in name
    tile = (min(3 if setting[0] else 16, shape[0]), min(5 if setting[0] else 64, shape[1]))
    return "canny_nms_kernel" in name and "tile={}x{} ".format(*tile) in name and ("no masks" in name) != masks


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("shape", CANNY_SHAPES, ids=_ids(CANNY_SHAPES))
def test_canny_stage_matches_host_bit_for_bit(gpu, feature, knob, shape, setting):
    """magnitude, local maxima and both masks of mi_canny_nms; the Sobel responses of the transcription against ndi.sobel"""
    from cupyimg_amd.scipy import ndimage as ndi
    knob(*setting)
    rng = np.random.RandomState(shape[0] * 7 + shape[1])
    from scipy import ndimage as sndi
    smoothed = sndi.gaussian_filter(rng.uniform(size=shape), 1.0, mode="constant")
    for masked in (False, True):
        mask = rng.uniform(size=shape) > 0.1 if masked else np.ones(shape, bool)
        isobel, jsobel, magnitude, local_max = R.canny_stage(smoothed, mask)
        eroded = sndi.binary_erosion(mask, np.ones((3, 3), bool), border_value=0)
        high, low = (float(v) for v in np.quantile(magnitude, [0.8, 0.5]))
        got = feature._canny_stage(gpu.asarray(smoothed), gpu.asarray(eroded), high, low)
        assert _canny_route(gpu.last_kernel(), shape, setting, True), gpu.last_kernel()
        assert same_bits(got[0].get(), magnitude)
        assert np.array_equal(got[1].get(), local_max)
        assert np.array_equal(got[2].get(), local_max & (magnitude >= high))
        assert np.array_equal(got[3].get(), local_max & (magnitude >= low))
        bare = feature._canny_stage(gpu.asarray(smoothed), gpu.asarray(eroded))
        assert _canny_route(gpu.last_kernel(), shape, setting, False), gpu.last_kernel()
        assert bare[2] is None and same_bits(bare[0].get(), magnitude) and np.array_equal(bare[1].get(), local_max)
    # the cross-check against this library's ndi.sobel, whose fused float64 kernel contracts products into multiply-adds: an
    # evaluation makes at most 11 rounded operations (6 products, 5 sums) on partial sums of at most S = the same filter of
    # |smoothed| with |weights|, so two evaluations differ by at most 22 * 2^-53 * S
    for axis, want in ((0, isobel), (1, jsobel)):
        absw = np.outer([1, 2, 1], [1, 1, 1]) if axis == 1 else np.outer([1, 1, 1], [1, 2, 1])
        bound = 22 * 2.0 ** -53 * sndi.correlate(np.abs(smoothed), absw.astype(float), mode="reflect")
        assert np.all(np.abs(ndi.sobel(gpu.asarray(smoothed), axis=axis).get() - want) <= bound)


CANNY_CASES = R.canny_cases()


@functools.lru_cache(maxsize=None)
def _canny_want(index):
    name, image, kw = CANNY_CASES[index]
    detail = {}
    edges = R.canny(image, detail=detail, **kw)
    return edges, detail


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("index", range(len(CANNY_CASES)), ids=[c[0] for c in CANNY_CASES])
def test_canny_matches_host(gpu, feature, knob, index, setting):
    knob(*setting)
    name, image, kw = CANNY_CASES[index]
    want, detail = _canny_want(index)
    kw = dict(kw)
    if kw.get("mask") is not None:
        kw["mask"] = gpu.asarray(kw["mask"])
    got = feature.canny(gpu.asarray(image), **kw)
    assert got.dtype == np.bool_ and np.array_equal(got.get(), want)
    if kw.get("use_quantiles"):
        mag = gpu.asarray(detail["magnitude"])
        high, low = feature._device_percentiles(mag, (100.0 * kw["high_threshold"], 100.0 * kw["low_threshold"]))
        assert (high, low) == (detail["high"], detail["low"])


def test_canny_smoothing_matches_host(gpu, feature):
    """smooth_with_function_and_mask: float64 for every image dtype; a masked copy, so NaN under the mask leaves no trace.
    Against SciPy's Gaussian to 1e-14 relative: the images and weights are non-negative (no cancellation), each of the two
    9-tap passes makes 17 rounded operations on the image and on the mask, the fused kernel in another order and contracted:
    (2 * 17 + 1) * 2 * 2^-53 < 1e-14."""
    for i, dtype in enumerate(("float64", "float32", "uint8")):
        image = np.array(CANNY_CASES[6 + i][1])
        assert image.dtype == np.dtype(dtype)
        mask = np.random.RandomState(1).uniform(size=image.shape) > 0.1
        if np.dtype(dtype).kind == "f":
            image[~mask] = np.nan
        got = feature._canny_smooth(gpu.asarray(image), gpu.asarray(mask), 1.0)
        want = R.canny_smooth(image, mask, 1.0)
        assert got.dtype == np.float64 and np.isfinite(want).all()
        np.testing.assert_allclose(got.get(), want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("case", KAT["canny"], ids=[c["name"] for c in KAT["canny"]])
def test_canny_known_answers(gpu, feature, case):
    def canny(image, *args, **kw):
        return feature.canny(gpu.asarray(np.asarray(image)) if np.ndim(image) == 2 else image, *args, **kw).get()
    check_canny_case(case, canny)


def test_canny_host_inputs_and_views(gpu, feature):
    name, image, kw = CANNY_CASES[6]
    want, _ = _canny_want(6)
    assert np.array_equal(feature.canny(image, **kw).get(), want)
    padded = gpu.asarray(np.pad(image, 3))
    assert np.array_equal(feature.canny(padded[3:-3, 3:-3], **kw).get(), want)
    assert np.array_equal(feature.canny(gpu.asarray(image), **kw).get(), feature.canny(gpu.asarray(image), **kw).get())
    with pytest.raises(ValueError):
        feature.canny(gpu.asarray(np.zeros((4, 4, 4))))
