"""What the structure-tensor family promises without a device: the entry points are declared, exported and bound; the Python
layer exposes the reference's names and signatures; and every raise and warning of the argument checks is reached before
anything touches the device (the inputs below are host arrays: an upload would fail on a machine without a GPU)."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {"mi_structure_products": 7, "mi_corner_response": 7}
DETECTORS = ("corner_harris", "corner_shi_tomasi", "corner_foerstner", "corner_kitchen_rosenfeld")


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
    assert re.search(r"\bint\s+mi_debug_set_corners\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", _header("mi355img_debug.h"))
    assert lib.mi_debug_set_corners(0, 0) == 0


def test_kernel_source_is_built_without_contraction():
    from cupyimg_amd import _build
    assert ("corners.hip", ["-ffp-contract=off"]) in _build.SOURCES


def test_python_layer_exposes_the_reference_signatures():
    from cupyimg_amd.skimage import feature

    def defaults(fn):
        return [(n, p.default) for n, p in inspect.signature(fn).parameters.items()]

    assert defaults(feature.structure_tensor) == [("image", inspect.Parameter.empty), ("sigma", 1), ("mode", "constant"), ("cval", 0), ("order", None)]
    assert list(inspect.signature(feature.structure_tensor_eigvals).parameters) == ["Axx", "Axy", "Ayy"]
    assert defaults(feature.corner_harris)[1:] == [("method", "k"), ("k", 0.05), ("eps", 1e-6), ("sigma", 1)]
    assert defaults(feature.corner_shi_tomasi)[1:] == [("sigma", 1)]
    assert defaults(feature.corner_foerstner)[1:] == [("sigma", 1)]
    assert defaults(feature.corner_kitchen_rosenfeld)[1:] == [("mode", "constant"), ("cval", 0)]
    for name in ("structure_tensor", "structure_tensor_eigvals") + DETECTORS:
        assert name in feature.__all__ and getattr(feature, name).__doc__
    assert "Peak memory" in feature.structure_tensor.__doc__
    assert "Deviation" in feature.corner_kitchen_rosenfeld.__doc__


def test_order_checks_need_no_device():
    from cupyimg_amd.skimage import feature
    with pytest.raises(ValueError, match="rc"):
        feature.structure_tensor(np.zeros((5, 5, 5)), sigma=0.1, order="xy")
    with pytest.raises(ValueError):
        feature.structure_tensor(np.zeros((5, 5, 5, 5)), order="xy")
    for order in ("yx", "cr", 0, "RC"):
        with pytest.raises(ValueError):
            feature.structure_tensor(np.zeros((5, 5)), order=order)
    # the default: a FutureWarning and 'xy' in 2-D, silently 'rc' in every other rank
    with pytest.warns(FutureWarning, match="the default order of the structure"):
        assert feature._check_structure_args(2, 1, "constant", None) == ("xy", [1.0, 1.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert feature._check_structure_args(3, 1, "constant", None) == ("rc", [1.0, 1.0, 1.0])
        assert feature._check_structure_args(1, 2, "reflect", None) == ("rc", [2.0])
        assert feature._check_structure_args(2, (1, 2.5), "wrap", "rc") == ("rc", [1.0, 2.5])
        assert feature._check_structure_args(2, 1, "grid-constant", "xy") == ("xy", [1.0, 1.0])


def test_the_default_order_warns_from_the_public_function():
    import cupyimg_amd as ca
    from cupyimg_amd.skimage import feature
    with pytest.warns(FutureWarning, match="the default order of the structure"):
        try:
            feature.structure_tensor(np.zeros((5, 5)), sigma=0.1)
        except Exception:
            assert not ca.is_available()            # the warning came before the upload that failed


def test_mode_sigma_and_rank_checks_need_no_device():
    from cupyimg_amd.skimage import feature
    with pytest.raises((ValueError, RuntimeError)):
        feature.structure_tensor(np.zeros((5, 5)), mode="no such mode", order="rc")
    with pytest.raises((ValueError, RuntimeError)):
        feature.structure_tensor(np.zeros((5, 5)), sigma=(1, 2, 3), order="rc")
    with pytest.raises(ValueError):
        feature.structure_tensor(np.zeros(()), order="rc")
    with pytest.raises(ValueError):
        feature.structure_tensor(np.zeros((2,) * 9), order="rc")
    with pytest.raises((ValueError, RuntimeError)):
        feature.corner_kitchen_rosenfeld(np.zeros((5, 5)), mode="no such mode")
    for name in ("corner_harris", "corner_shi_tomasi", "corner_foerstner"):
        with pytest.raises((ValueError, RuntimeError)):
            getattr(feature, name)(np.zeros((5, 5)), sigma=(1, 2, 3))


def test_detectors_take_2d_images_only():
    from cupyimg_amd.skimage import feature
    for name in DETECTORS:
        for image in (np.zeros((4, 4, 4)), np.zeros(7), np.zeros((2, 3, 4, 5))):
            with pytest.raises(ValueError):
                getattr(feature, name)(image)
    for method in ("K", "noble", None):
        with pytest.raises(ValueError):
            feature.corner_harris(np.zeros((5, 5)), method=method)


def test_structure_tensor_eigvals_warns_and_checks_first():
    from cupyimg_amd.skimage import feature
    volume = np.zeros((3, 3, 3))
    with pytest.warns(FutureWarning, match="structure_tensor_eigvals is deprecated"):
        with pytest.raises(ValueError):
            feature.structure_tensor_eigvals(volume, volume, volume)


def test_library_refuses_bad_descriptors_without_a_device():
    """the checks of the entry points run before anything is queued"""
    from cupyimg_amd import _lib
    lib = _lib.load()
    size = {10: 8, 9: 4, 5: 4}

    def desc(shape, dtype_code=10, data=0x10000, row_stride=None):
        d = _lib.MiArray()
        d.data = data
        d.dtype = dtype_code
        d.ndim = len(shape)
        st = size[dtype_code]
        for i in reversed(range(len(shape))):
            d.shape[i] = shape[i]
            d.strides[i] = st
            st *= shape[i]
        if row_stride is not None:
            d.strides[0] = row_stride
        return d

    ref = ctypes.byref
    image, block = desc((4, 5)), desc((3, 20), data=0x20000)
    call = lib.mi_structure_products
    assert call(ref(desc((4, 5), 5)), ref(block), 1, 0, 1, 0.0, None) == _lib.MI_ERR_UNSUPPORTED                       # an integer image
    assert call(ref(image), ref(desc((3, 20), 9, 0x20000)), 1, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG             # another dtype
    assert call(ref(image), ref(desc((2, 20), data=0x20000)), 1, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG           # two rows for products
    assert call(ref(image), ref(block), 0, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG                                 # three rows for derivatives
    assert call(ref(image), ref(desc((3, 19), data=0x20000)), 1, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG           # short rows
    assert call(ref(image), ref(desc((3, 20), data=0x20000, row_stride=152)), 1, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG   # overlapping rows
    assert call(ref(image), ref(desc((3, 20), data=0x20000, row_stride=164)), 1, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG   # not whole elements
    assert call(ref(image), ref(block), 1, 0, 9, 0.0, None) == _lib.MI_ERR_INVALID_ARG                                 # mode
    assert call(ref(desc((3, 4, 5))), ref(desc((6, 60), data=0x20000)), 1, 1, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG # reversed, 3-D
    assert call(ref(image), ref(desc((3, 20), data=0x10000 + 80)), 1, 0, 1, 0.0, None) == _lib.MI_ERR_INVALID_ARG      # shares memory
    assert call(ref(desc((4, 5), row_stride=48)), ref(block), 1, 0, 1, 0.0, None) == _lib.MI_ERR_NOT_CONTIGUOUS
    call = lib.mi_corner_response
    out, out2, out32 = desc((4, 5), data=0x30000), desc((4, 5), data=0x40000), desc((4, 5), 9, 0x30000)
    assert call(ref(block), ref(out), None, 7, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG                            # kind
    assert call(ref(block), ref(out), ref(out2), 0, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG                       # a second output
    assert call(ref(block), ref(out), None, 3, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG                            # Foerstner without one
    assert call(ref(block), ref(out), None, 4, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG                            # three rows for Kitchen-Rosenfeld
    assert call(ref(block), ref(out32), None, 0, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG                          # output dtype
    assert call(ref(desc((3, 20), 9, 0x20000)), ref(out32), None, 3, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG      # float64 for Foerstner
    assert call(ref(desc((3, 20), 5, 0x20000)), ref(out), None, 0, 0.05, 1e-6, None) == _lib.MI_ERR_UNSUPPORTED
    assert call(ref(block), ref(desc((4, 5), data=0x20000 + 160)), None, 0, 0.05, 1e-6, None) == _lib.MI_ERR_INVALID_ARG   # shares memory
