"""skimage.feature.structure_tensor and the corner detectors on the device (csrc/corners.hip) against the host transcription of
tests/helpers/corner_ref.py, bit for bit, under the three settings of mi_debug_set_corners (the planner's boxes, small boxes
with seams along every axis, the forced pass-by-pass route), the route read back from last_kernel(); the Gaussian stage
against this library's own filter (same bits) and against a float64 SciPy Gaussian (the bound of the float32 filters); and
the known answers of tests/golden/corner_kat.json."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
from scipy import ndimage as sndi

from helpers import corner_ref as R
from helpers import value_ranges as V
from test_corners_yardstick import (KAT, MODES, SHAPES, admitted_maximum_cases, check_finite_case, check_structure_case, has_unique_maximum_at,
                                    ids, image_of, maximum_image, planted_image, same_bits)

pytestmark = pytest.mark.gpu

# (small tiles, forced pass-by-pass route)
SETTINGS = [(0, 0), (1, 0), (0, 1)]
SETTING_IDS = ["planner", "small", "generic"]
DTYPES = ["float32", "float64", "uint8", "int16"]
# every mode with a cval float32 cannot hold; the constant modes also with one that it can
MODE_CVALS = [(m, 0.37) for m in MODES] + [("constant", 0.5), ("grid-constant", 0.5)]


@pytest.fixture(scope="module")
def feature(gpu):
    from cupyimg_amd.skimage import feature
    return feature


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_corners
    fn.argtypes = [ctypes.c_int] * 2
    yield fn
    fn(0, 0)


def _float_dtype(dtype):
    return np.dtype(dtype if np.dtype(dtype).kind == "f" else "float64")


def _route(name, shape, dtype, setting, products):
    """does last_kernel() name the route this setting must take?"""
    tname = "float32" if _float_dtype(dtype) == np.float32 else "float64"
    what = "products" if products else "derivatives"
    if setting[1] or len(shape) not in (2, 3):
        return "st_generic<{}>".format(tname) in name and "{} rank {} ".format(what, len(shape)) in name
    full = (1,) * (3 - len(shape)) + tuple(shape)
    if setting[0]:
        box = (2 if len(shape) == 3 else 1, 3, 5)
    else:
        box = ((8 if tname == "float32" else 4) if len(shape) == 3 else 1, 8 if len(shape) == 3 else 32, 64)
    box = tuple(min(b, n) for b, n in zip(box, full))
    return "st_fused_kernel<{},{},{}>".format(tname, len(shape), what) in name and "box={}x{}x{} ".format(*box) in name


@functools.lru_cache(maxsize=16)
def _want(shape, dtype, planted, mode, cval):
    """(derivatives, rc products, xy products or None) of the transcription, computed once and shared by the three settings"""
    image = R.prepare(planted_image(shape, dtype) if planted else image_of(shape, dtype))
    derivs = R.derivatives(image, mode, cval)
    return derivs, R.products(derivs, "rc"), R.products(derivs, "xy") if len(shape) == 2 else None


def _rows(block, shape):
    return [block[e].get().reshape(shape) for e in range(block.shape[0])]


def _check_product_stage(gpu, feature, shape, dtype, setting, planted):
    host = planted_image(shape, dtype) if planted else image_of(shape, dtype)
    x = gpu.ascontiguousarray(feature._as_float_device(gpu.asarray(host)))
    assert x.dtype == _float_dtype(dtype)
    for mode, cval in MODE_CVALS:
        derivs, rc, xy = _want(shape, dtype, planted, mode, cval)
        got = _rows(feature._sobel_block(x, False, False, mode, cval), shape)
        kernel = gpu.last_kernel()
        assert _route(kernel, shape, dtype, setting, False), (kernel, mode)
        assert len(got) == len(derivs) and all(same_bits(g, w) for g, w in zip(got, derivs)), (mode, cval, "derivatives")
        for order, want in (("rc", rc), ("xy", xy)):
            if want is None:
                continue
            got = _rows(feature._sobel_block(x, True, order == "xy", mode, cval), shape)
            kernel = gpu.last_kernel()
            assert _route(kernel, shape, dtype, setting, True), (kernel, mode)
            assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), (mode, cval, order)


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_derivatives_and_products_match_host_bit_for_bit(gpu, feature, knob, shape, dtype, setting):
    knob(*setting)
    _check_product_stage(gpu, feature, shape, dtype, setting, False)


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_planted_nonfinite_values_match_host_bit_for_bit(gpu, feature, knob, shape, dtype, setting):
    """NaN, +-inf and -0.0 on the border, one sample inside it and on a box seam: the `* 0.0` term turns an infinite centre into
    NaN, the sign of a zero follows SciPy's order of operations"""
    knob(*setting)
    _check_product_stage(gpu, feature, shape, dtype, setting, True)


# ---------------------------------------------------------------- the whole tensor
def _sigmas(ndim):
    return [1, [0.8 + 0.45 * a for a in range(ndim)]]


def _gauss_bound(products64, sigma, mode, cval):
    """(float64 SciPy Gaussian, B, c) of one product: B the filter of |product| with |cval|, c the sum of taps + 2 over the axes"""
    spec = V.gaussian_spec(products64.ndim, sigma)
    ref = sndi.gaussian_filter(products64, sigma, mode=mode, cval=cval)
    return ref, V.abs_separable(spec, mode, cval)(np.abs(products64)), V.sep_c(spec)


TENSOR_CASES = [("constant", 0.0), ("constant", 0.37), ("reflect", 0.0), ("mirror", 0.0), ("nearest", 0.0), ("wrap", 0.0), ("grid-constant", 0.5),
                ("grid-wrap", 0.0), ("grid-mirror", 0.0)]


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_structure_tensor_is_the_gaussian_of_the_host_products(gpu, feature, knob, shape, dtype, setting):
    """the same call on the same bits: ndi.gaussian_filter of the uploaded transcription products; and within the float32
    filters' bound c . u . B of a float64 SciPy Gaussian of those products.  sigma as a scalar and per axis, both orders in 2-D"""
    from cupyimg_amd.scipy import ndimage as ndi
    knob(*setting)
    host = image_of(shape, dtype)
    x = gpu.asarray(host)
    fdt = _float_dtype(dtype)
    u = V.U32 if fdt == np.float32 else V.U64
    orders = ("rc", "xy") if len(shape) == 2 else ("rc",)
    for i, (mode, cval) in enumerate(TENSOR_CASES):
        sigma = _sigmas(len(shape))[i % 2]
        order = orders[(i // 2) % len(orders)]
        want_products = R.structure_products(host, mode, cval, order)
        got = feature.structure_tensor(x, sigma=sigma, mode=mode, cval=cval, order=order)
        assert len(got) == len(want_products) and all(g.dtype == fdt and g.shape == tuple(shape) for g in got)
        for g, p in zip(got, want_products):
            g = g.get()
            assert same_bits(g, ndi.gaussian_filter(gpu.asarray(p), sigma, mode=mode, cval=cval).get()), (mode, cval, order)
            ref, B, c = _gauss_bound(p.astype(np.float64), sigma, mode, cval)
            ratio, at = V.ratio_of(g, ref, B, c, u)
            assert ratio <= 1.0, (mode, cval, order, ratio, at)


def test_elements_are_views_of_one_block_and_inputs_stay(gpu, feature):
    base = np.random.RandomState(3).uniform(size=(14, 40, 81)).astype(np.float32)
    dev = gpu.asarray(base)
    view, hview = dev[1:13:2, 3:, 5:76], np.ascontiguousarray(base[1:13:2, 3:, 5:76])
    elems = feature.structure_tensor(view, sigma=1.5, mode="mirror")
    assert len(elems) == 6
    step = elems[1].ptr - elems[0].ptr
    assert step >= hview.size * 4 and step % 16 == 0 and all(elems[e + 1].ptr - elems[e].ptr == step for e in range(5))
    again = feature.structure_tensor(hview, sigma=1.5, mode="mirror")                 # a host image, and repeatability
    assert all(a.get().tobytes() == b.get().tobytes() for a, b in zip(elems, again))
    assert np.array_equal(dev.get(), base)
    half = feature.structure_tensor(base[0].astype(np.float16), order="rc")           # float16: computed in float32
    want = feature.structure_tensor(base[0].astype(np.float16).astype(np.float32), order="rc")
    assert all(h.dtype == np.float32 and same_bits(h.get(), w.get()) for h, w in zip(half, want))
    l1, l2 = (e.get() for e in feature.structure_tensor_eigenvalues(feature.structure_tensor(base[0], order="rc")))
    with pytest.warns(FutureWarning):
        m1, m2 = feature.structure_tensor_eigvals(*feature.structure_tensor(base[0], order="rc"))
    assert same_bits(m1.get(), l1) and same_bits(m2.get(), l2) and np.all(l1 >= l2)


def test_empty_images_give_empty_results(gpu, feature):
    empty = gpu.asarray(np.zeros((0, 5), np.float32))
    elems = feature.structure_tensor(empty, order="rc")
    assert len(elems) == 3 and all(e.shape == (0, 5) and e.dtype == np.float32 for e in elems)
    assert feature.corner_harris(empty).shape == (0, 5) and feature.corner_kitchen_rosenfeld(empty).dtype == np.float64
    w, q = feature.corner_foerstner(empty)
    assert w.shape == q.shape == (0, 5)
    assert len(feature.structure_tensor(gpu.asarray(np.zeros((3, 0, 4))))) == 6


# ---------------------------------------------------------------- the detectors
IMAGES =[(70, 96), (5, 1040), (2, 2)]


def _detector_inputs(shape, dtype):
    """a random image, and one with flat regions (a zero trace and a zero denominator must give the 0 of the masked fill)"""
    flat = np.zeros(shape, dtype)
    flat[: max(shape[0] // 3, 1), : shape[1] // 2] = 1
    return [image_of(shape, dtype), flat]


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", IMAGES, ids=ids(IMAGES))
def test_detectors_match_host_on_the_device_tensor_bit_for_bit(gpu, feature, knob, shape, dtype, setting):
    knob(*setting)
    for host in _detector_inputs(shape, dtype):
        x = gpu.asarray(host)
        for sigma in (1, (1.5, 0.7)):
            Arr, Arc, Acc = (e.get() for e in feature.structure_tensor(x, sigma, order="rc"))
            for kw in (dict(), dict(method="eps"), dict(k=0.11), dict(method="eps", eps=0.25)):
                got = feature.corner_harris(x, sigma=sigma, **kw)
                assert "corner_response_kernel<{},harris_{}>".format(dtype, kw.get("method", "k")) in gpu.last_kernel()
                assert got.dtype == np.dtype(dtype) and same_bits(got.get(), R.corner_harris(Arr, Arc, Acc, **kw)), kw
            got = feature.corner_shi_tomasi(x, sigma=sigma)
            assert got.dtype == np.dtype(dtype) and same_bits(got.get(), R.corner_shi_tomasi(Arr, Arc, Acc))
            w, q = feature.corner_foerstner(x, sigma=sigma)
            ww, wq = R.corner_foerstner(Arr, Arc, Acc)
            assert w.dtype == q.dtype == np.float64 and same_bits(w.get(), ww) and same_bits(q.get(), wq)
        for mode, cval in (("constant", 0), ("constant", 0.37), ("reflect", 0), ("wrap", 0)):
            got = feature.corner_kitchen_rosenfeld(x, mode=mode, cval=cval)
            assert "corner_response_kernel<{},kitchen_rosenfeld>".format(dtype) in gpu.last_kernel()
            assert got.dtype == np.float64 and same_bits(got.get(), R.corner_kitchen_rosenfeld(host, mode, cval)), (mode, cval)


def test_detectors_convert_integer_images(gpu, feature):
    """uint8 / int16 images are scaled to float64 first, in corner_kitchen_rosenfeld too (the documented deviation)"""
    for dtype in ("uint8", "int16"):
        host = image_of((70, 96), dtype)
        x = gpu.asarray(host)
        elems = [e.get() for e in feature.structure_tensor(x, 1, order="rc")]
        assert same_bits(feature.corner_harris(x).get(), R.corner_harris(*elems))
        assert same_bits(feature.corner_shi_tomasi(x).get(), R.corner_shi_tomasi(*elems))
        assert same_bits(feature.corner_kitchen_rosenfeld(x).get(), R.corner_kitchen_rosenfeld(host))


# ---------------------------------------------------------------- known answers
def _device_structure_tensor(feature):
    return lambda image, **kw: [e.get() for e in feature.structure_tensor(image, **kw)]


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("case", KAT["structure_tensor"], ids=[c["name"] for c in KAT["structure_tensor"]])
def test_structure_tensor_known_answers(gpu, feature, knob, case, setting):
    knob(*setting)
    check_structure_case(case, _device_structure_tensor(feature))


def test_other_known_answers(gpu, feature):
    for case in KAT["raises"]:
        with pytest.raises(ValueError):
            feature.structure_tensor(gpu.asarray(np.zeros(case["shape"])), sigma=case["sigma"], order=case["order"])

    def host(fn):
        def call(image):
            out = fn(gpu.asarray(image))
            return tuple(o.get() for o in out) if isinstance(out, tuple) else out.get()
        return call

    detectors = {name: host(getattr(feature, name)) for name in ("corner_harris", "corner_shi_tomasi", "corner_foerstner", "corner_kitchen_rosenfeld")}
    for case in KAT["finite"]:
        check_finite_case(case, detectors)
    cases = {c["name"]: c for c in KAT["maximum"]}
    for name, detector in admitted_maximum_cases():
        assert has_unique_maximum_at(detectors[detector](maximum_image(cases[name])), cases[name]["at"]), (name, detector)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                       # 'rc' is the silent default in 3-D
        a = feature.structure_tensor(gpu.asarray(np.zeros((5, 5, 5))), sigma=0.1)
        b = feature.structure_tensor(gpu.asarray(np.zeros((5, 5, 5))), sigma=0.1, order="rc")
    assert all(same_bits(x.get(), y.get()) for x, y in zip(a, b))
