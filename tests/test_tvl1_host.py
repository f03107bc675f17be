"""What optical_flow_tvl1 promises without a device: the new entry points are exported with the documented prototypes, the
Python layer exposes the documented names and signatures, and the argument validation that needs no device raises."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "mi_tvl1_coords": 3, "mi_tvl1_prepare": 7, "mi_tvl1_data": 6, "mi_tvl1_scratch_size": 2, "mi_tvl1_reg": 9, "mi_tvl1_diff_sum": 4,
}


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
    assert "MI_TVL1_WORK_BYTES" in text
    assert re.search(r"\bint\s+mi_debug_set_tvl1\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", _header("mi355img_debug.h"))
    assert lib.mi_debug_set_tvl1(0, 0) == 0


def test_kernel_source_is_built_without_contraction():
    from cupyimg_amd import _build
    assert ("tvl1.hip", ["-ffp-contract=off"]) in _build.SOURCES


def test_python_layer_exposes_the_documented_names():
    from cupyimg_amd.skimage import registration, transform
    sig = inspect.signature(registration.optical_flow_tvl1)
    kinds = {n: p.kind for n, p in sig.parameters.items()}
    assert list(kinds)[:2] == ["reference_image", "moving_image"]
    defaults = {n: p.default for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert defaults == dict(attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4, prefilter=False, dtype=np.float32)
    for name in ("_tvl1", "coarse_to_fine", "get_pyramid", "resize_flow", "last_tvl1_stats"):
        assert callable(getattr(registration, name)), name
    assert list(inspect.signature(transform.resize).parameters) == [
        "image", "output_shape", "order", "mode", "cval", "clip", "preserve_range", "anti_aliasing", "anti_aliasing_sigma"]
    for fn, factor in ((transform.pyramid_reduce, "downscale"), (transform.pyramid_expand, "upscale")):
        assert list(inspect.signature(fn).parameters) == ["image", factor, "sigma", "order", "mode", "cval", "multichannel",
                                                          "preserve_range"]
    for name in ("resize", "pyramid_reduce", "pyramid_expand", "warp", "warp_coords"):
        assert name in transform.__all__


def test_validation_that_needs_no_device():
    from cupyimg_amd.skimage import registration, transform
    x = np.zeros((4, 4), np.complex64)
    with pytest.raises(TypeError):
        registration.optical_flow_tvl1(x, x)
    with pytest.raises(ValueError):
        transform.pyramid_reduce(None, downscale=1)
    with pytest.raises(ValueError):
        transform.pyramid_expand(None, upscale=1)
    assert registration.last_tvl1_stats() == [] or isinstance(registration.last_tvl1_stats(), list)


def test_library_refuses_bad_descriptors_without_a_device():
    """the checks of the entry points run before anything is queued"""
    from cupyimg_amd import _lib
    lib = _lib.load()

    def desc(shape, dtype_code=9):
        d = _lib.MiArray()
        d.data = 0x1000
        d.dtype = dtype_code
        d.ndim = len(shape)
        st = 4
        for i in reversed(range(len(shape))):
            d.shape[i] = shape[i]
            d.strides[i] = st
            st *= shape[i]
        return d

    need = ctypes.c_int64(-1)
    assert lib.mi_tvl1_scratch_size(ctypes.byref(desc((3, 4, 5, 6))), ctypes.byref(need)) == 0 and need.value == 0
    assert lib.mi_tvl1_scratch_size(ctypes.byref(desc((4, 3, 4, 5, 6))), ctypes.byref(need)) == 0 and need.value == 20 * 360
    assert lib.mi_tvl1_scratch_size(ctypes.byref(desc((3, 1, 5, 6))), ctypes.byref(need)) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_tvl1_scratch_size(ctypes.byref(desc((2, 4, 5, 6))), ctypes.byref(need)) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_tvl1_scratch_size(ctypes.byref(desc((3, 4, 5, 6), 5)), ctypes.byref(need)) == _lib.MI_ERR_UNSUPPORTED
    f = desc((2, 8, 8))
    p = desc((2, 2, 8, 8))
    assert lib.mi_tvl1_reg(ctypes.byref(f), ctypes.byref(p), ctypes.byref(f), ctypes.byref(p), None, 0.25, 0.8, None, None) == _lib.MI_ERR_INVALID_ARG
