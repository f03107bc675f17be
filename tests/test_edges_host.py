"""What the edge family promises without a device: the entry points are declared, exported and bound; the Python layer exposes
the reference's names and signatures; the dense weights and the Laplace operator built on the host are the transcription's;
the percentile plan is NumPy's; and the argument validation that needs no device raises."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from helpers import edges_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {"mi_edge_filter": 9, "mi_edge_pair_magnitude": 5, "mi_threshold_masks": 8, "mi_canny_nms": 9, "mi_canny_threshold": 7,
              "mi_masked_copy": 4, "mi_canny_normalize": 4}


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    from cupyimg_amd import _lib
    lib = _lib.load()
    text = _header("mi355img.h")
    for name, nargs in PROTOTYPES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    assert re.search(r"\bint\s+mi_debug_set_edges\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", _header("mi355img_debug.h"))
    assert lib.mi_debug_set_edges(0, 0) == 0


def test_kernel_source_is_built_without_contraction():
    from cupyimg_amd import _build
    assert ("edges.hip", ["-ffp-contract=off"]) in _build.SOURCES


def test_python_layer_exposes_the_reference_signatures():
    from cupyimg_amd.skimage import feature, filters
    for name in ("sobel", "scharr", "prewitt"):
        sig = inspect.signature(getattr(filters, name))
        assert list(sig.parameters) == ["image", "mask", "axis", "mode", "cval"]
        assert {n: p.default for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY} == dict(axis=None, mode="reflect", cval=0.0)
        assert getattr(filters, name).__doc__
        for suffix in ("_h", "_v"):
            assert list(inspect.signature(getattr(filters, name + suffix)).parameters) == ["image", "mask"]
    for name in ("roberts", "roberts_pos_diag", "roberts_neg_diag"):
        assert list(inspect.signature(getattr(filters, name)).parameters) == ["image", "mask"]
    for name in ("farid", "farid_h", "farid_v"):
        sig = inspect.signature(getattr(filters, name))
        assert list(sig.parameters) == ["image", "mask"] and sig.parameters["mask"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(filters.laplace).parameters) == ["image", "ksize", "mask"]
    assert list(inspect.signature(filters.apply_hysteresis_threshold).parameters) == ["image", "low", "high"]
    sig = inspect.signature(feature.canny)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [("sigma", 1.0), ("low_threshold", None), ("high_threshold", None),
                                                                      ("mask", None), ("use_quantiles", False)]
    for name in ("sobel", "sobel_h", "sobel_v", "scharr", "scharr_h", "scharr_v", "prewitt", "prewitt_h", "prewitt_v", "farid", "farid_h",
                 "farid_v", "roberts", "roberts_pos_diag", "roberts_neg_diag", "laplace", "apply_hysteresis_threshold"):
        assert name in filters.__all__
    assert "canny" in feature.__all__


@pytest.mark.parametrize("ndim", [1, 2, 3, 4])
def test_dense_weights_are_the_transcriptions(ndim):
    from cupyimg_amd.skimage import filters
    for smooth, ours in ((R.SOBEL_SMOOTH, filters._SOBEL_SMOOTH), (R.SCHARR_SMOOTH, filters._SCHARR_SMOOTH), (R.PREWITT_SMOOTH, filters._PREWITT_SMOOTH)):
        assert np.array_equal(smooth, ours)
        for axis in list(range(ndim)) + [-1]:
            want = R.edge_kernel(ndim, axis, smooth)
            got = filters._edge_kernel(ndim, axis, ours)
            assert got.shape == (3,) * ndim and got.dtype == want.dtype        # (rank 1: the integer edge weights themselves)
            assert np.array_equal(got, want)
    # the order of the products matters for 1 / 3: ((e * s) * s) * s, not e * (s * s * s)
    s = R.PREWITT_SMOOTH[0]
    assert filters._edge_kernel(4, 0, filters._PREWITT_SMOOTH)[0, 0, 0, 0] == ((1 * s) * s) * s
    assert np.array_equal(filters._laplace_operator(ndim), R.laplace_operator(ndim))
    assert filters._laplace_operator(ndim)[(1,) * ndim] == 2 * ndim and filters._laplace_operator(ndim).sum() == 0


def test_fixed_weights_are_the_transcriptions():
    from cupyimg_amd.skimage import filters
    assert np.array_equal(filters._HFARID_WEIGHTS, R.HFARID) and np.array_equal(filters._VFARID_WEIGHTS, R.VFARID)
    assert np.array_equal(filters._ROBERTS_PD_WEIGHTS, R.ROBERTS_PD) and np.array_equal(filters._ROBERTS_ND_WEIGHTS, R.ROBERTS_ND)


def test_axes_and_modes():
    from cupyimg_amd.skimage import filters
    assert filters._edge_axes(None, 3) == ([0, 1, 2], True)
    assert filters._edge_axes(1, 3) == ([1], False)
    assert filters._edge_axes(-1, 3) == ([-1], False)
    assert filters._edge_axes((0, 2), 3) == ([0, 2], True)
    assert filters._edge_axes([1], 3) == ([1], False)
    assert filters._edge_mode("mirror") == "mirror"
    assert filters._edge_mode(["wrap", "wrap"]) == "wrap"
    with pytest.raises(ValueError):
        filters._edge_mode(["wrap", "reflect"])
    with pytest.raises(ValueError):
        filters._edge_mode([])
    with pytest.raises((ValueError, RuntimeError)):
        filters._edge_mode("no such mode")


def test_validation_that_needs_no_device():
    from cupyimg_amd.skimage import feature, filters
    volume = np.zeros((4, 4, 4))
    for name in ("sobel_h", "sobel_v", "scharr_h", "scharr_v", "prewitt_h", "prewitt_v", "roberts", "roberts_pos_diag", "roberts_neg_diag",
                 "farid", "farid_h", "farid_v"):
        with pytest.raises(ValueError):
            getattr(filters, name)(volume)
        with pytest.raises(ValueError):
            getattr(filters, name)(np.zeros(5))
    for name in ("sobel", "scharr", "prewitt"):
        with pytest.raises(ValueError):
            getattr(filters, name)(np.zeros((4, 4)), mode=["reflect", "wrap"])
    with pytest.raises(ValueError):
        filters.laplace(np.zeros((4, 4)), ksize=2)
    with pytest.raises(ValueError):
        feature.canny(volume, 4, 0, 0)
    with pytest.raises(ValueError):
        feature.canny(np.zeros(7))
    image = np.zeros((11, 11))
    for low, high in ((0.5, 3.6), (-5, 0.5), (99, 0.9), (0.5, -100), (50, 150)):
        with pytest.raises(ValueError):
            feature.canny(image, use_quantiles=True, low_threshold=low, high_threshold=high)
    assert feature._dtype_max(np.uint8) == 255 and feature._dtype_max(np.int16) == 32767
    assert feature._dtype_max(np.float32) == 1 and feature._dtype_max(np.bool_) == 1
    assert feature._canny_thresholds(None, None, False, 255) == (0.1, 0.2)
    assert feature._canny_thresholds(25.5, 51, False, 255) == (25.5 / 255, 51 / 255)


def test_percentile_plan_is_numpys():
    """the two order statistics and the weight, so that the thresholds of use_quantiles equal numpy.percentile bit for bit"""
    from cupyimg_amd.skimage import feature
    rng = np.random.RandomState(0)
    for n in (1, 2, 9, 4480, 4847):
        a = rng.uniform(size=n)
        ordered = np.sort(a)
        for q in (0.0, 0.07, 0.29, 0.5, 0.55, 0.6, 0.8, 0.9, 0.999, 1.0):
            k0, k1, gamma = feature._percentile_plan(n, 100.0 * q)
            assert (k0, k1, gamma) == R.percentile_plan(n, 100.0 * q)
            assert feature._lerp(ordered[k0], ordered[k1], gamma) == np.percentile(a, 100.0 * q)


def test_library_refuses_bad_descriptors_without_a_device():
    """the checks of the entry points run before anything is queued"""
    from cupyimg_amd import _lib
    lib = _lib.load()

    def desc(shape, dtype_code=10):
        d = _lib.MiArray()
        d.data = 0x1000 * (1 + dtype_code + len(shape))
        d.dtype = dtype_code
        d.ndim = len(shape)
        st = {10: 8, 9: 4, 0: 1, 2: 1, 5: 4}[dtype_code]
        for i in reversed(range(len(shape))):
            d.shape[i] = shape[i]
            d.strides[i] = st
            st *= shape[i]
        return d

    w = (ctypes.c_double * 27)()
    f64, f32, i32, u8 = desc((4, 5)), desc((4, 5), 9), desc((4, 5), 5), desc((4, 5), 2)
    out = desc((4, 5))
    out.data = 0x9000
    assert lib.mi_edge_filter(ctypes.byref(i32), ctypes.byref(out), None, w, 1, 0, 0, 0.0, None) == _lib.MI_ERR_UNSUPPORTED
    assert lib.mi_edge_filter(ctypes.byref(f32), ctypes.byref(f32), None, w, 1, 0, 0, 0.0, None) == _lib.MI_ERR_INVALID_ARG     # float32 output
    assert lib.mi_edge_filter(ctypes.byref(f64), ctypes.byref(out), None, w, 2, 0, 0, 0.0, None) == _lib.MI_ERR_INVALID_ARG     # signed, two axes
    assert lib.mi_edge_filter(ctypes.byref(f64), ctypes.byref(out), None, w, 1, 1, 9, 0.0, None) == _lib.MI_ERR_INVALID_ARG     # mode
    assert lib.mi_edge_filter(ctypes.byref(f64), ctypes.byref(f64), None, w, 1, 1, 0, 0.0, None) == _lib.MI_ERR_INVALID_ARG     # in place
    assert lib.mi_canny_nms(ctypes.byref(f32), ctypes.byref(u8), ctypes.byref(out), ctypes.byref(u8), None, None, 0.0, 0.0, None) == _lib.MI_ERR_UNSUPPORTED
    vol = desc((3, 4, 5))
    assert lib.mi_canny_nms(ctypes.byref(vol), ctypes.byref(u8), ctypes.byref(out), ctypes.byref(u8), None, None, 0.0, 0.0, None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_canny_nms(ctypes.byref(f64), ctypes.byref(u8), ctypes.byref(out), ctypes.byref(u8), ctypes.byref(u8), None, 0.0, 0.0, None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_threshold_masks(ctypes.byref(f64), None, None, 0.0, 1.0, ctypes.byref(u8), ctypes.byref(u8), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_edge_pair_magnitude(ctypes.byref(f64), ctypes.byref(f32), ctypes.byref(out), 1.0, None) == _lib.MI_ERR_INVALID_ARG
