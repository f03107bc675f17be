"""What the selection / sorting / peak family promises without a device: the entry points are declared, exported and bound;
the Python layer exposes the reference's names and signatures; and every raise and warning of the argument checks is reached
before anything touches the device (the inputs below are host arrays: an upload would fail on a machine without a GPU)."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {"mi_select_work_bytes": 2, "mi_select_count": 4, "mi_select_write": 5, "mi_take": 6, "mi_argsort": 5, "mi_peak_count": 8,
              "mi_peak_write": 8, "mi_spacing_init": 5, "mi_spacing_rounds": 9, "mi_scatter_true": 3}
INF = np.inf


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
    debug = _header("mi355img_debug.h")
    assert re.search(r"\bint\s+mi_debug_set_select\s*\(\s*int\s+\w+\s*\)\s*;", debug)
    assert re.search(r"\bint\s+mi_debug_select_launches\s*\(\s*void\s*\)\s*;", debug)
    assert lib.mi_debug_set_select(0) == 0
    assert lib.mi_debug_select_launches() >= 0


def test_kernel_source_is_built_and_is_no_strict_twin_source():
    from cupyimg_amd import _build
    assert ("select.hip", []) in _build.SOURCES
    assert "select.hip" not in _build.STRICT_SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "select.hip"))


def test_public_names_are_exported():
    import cupyimg_amd as ca
    for name in ("count_nonzero", "flatnonzero", "nonzero", "argwhere", "take", "argsort", "sort"):
        assert getattr(ca, name) is getattr(ca.core, name) and getattr(ca, name).__doc__
    assert list(inspect.signature(ca.argsort).parameters.items())[1][1].default is False
    assert list(inspect.signature(ca.argsort).parameters) == ["a", "descending"]
    assert list(inspect.signature(ca.take).parameters) == ["a", "indices"]


def test_python_layer_exposes_the_reference_signatures():
    from cupyimg_amd.skimage import feature

    def defaults(fn):
        return [(n, p.default, p.kind) for n, p in inspect.signature(fn).parameters.items()]

    POS, KW = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    common = [("image", inspect.Parameter.empty, POS), ("min_distance", 1, POS), ("threshold_abs", None, POS), ("threshold_rel", None, POS),
              ("exclude_border", True, POS), ("indices", True, POS), ("num_peaks", INF, POS), ("footprint", None, POS), ("labels", None, POS)]
    assert defaults(feature.peak_local_max) == common + [("num_peaks_per_label", INF, POS), ("p_norm", INF, POS)]
    assert defaults(feature.corner_peaks) == common + [("num_peaks_per_label", INF, KW), ("p_norm", INF, KW)]
    assert [n for n, _, _ in defaults(feature._ensure_spacing)] == ["coords", "shape", "spacing", "p_norm", "inclusive"]
    assert defaults(feature._ensure_spacing)[3][1] == INF and defaults(feature._ensure_spacing)[4][1] is False
    for name in ("peak_local_max", "corner_peaks"):
        assert name in feature.__all__
        doc = getattr(feature, name).__doc__
        assert "Order contract" in doc and "Deviations" in doc and "NotImplementedError" in doc
    assert "raster order" in feature.peak_local_max.__doc__ and "Peak memory" in feature.peak_local_max.__doc__
    assert feature.last_peak_launches() >= 0


IMAGE = np.zeros((5, 5))


@pytest.mark.parametrize("fn", ("peak_local_max", "corner_peaks"))
def test_every_raise_comes_before_the_device(fn):
    from cupyimg_amd.skimage import feature
    call = getattr(feature, fn)
    with pytest.raises(NotImplementedError, match="find_objects"):
        call(IMAGE, labels=np.ones((5, 5), int))
    with pytest.raises(ValueError):
        call(IMAGE, exclude_border=(1,))
    with pytest.raises(TypeError):
        call(IMAGE, exclude_border=1.0)
    with pytest.raises(ValueError, match="must only contain ints"):
        call(IMAGE, exclude_border=(1, "a"))
    with pytest.raises(ValueError):
        call(IMAGE, exclude_border=(1, -1))
    with pytest.raises(ValueError):
        call(IMAGE, exclude_border=-1)
    for p in (3, 1.5, 0, "two"):
        with pytest.raises(ValueError, match="p_norm"):
            call(IMAGE, p_norm=p)
    for d in (1.5, 0.5, np.inf, np.nan):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            with pytest.raises(ValueError, match="min_distance"):
                call(IMAGE, min_distance=d)
    for bad in (IMAGE > 0, IMAGE.astype(complex), np.array([["a"]])):
        with pytest.raises(TypeError):
            call(bad)
    with pytest.raises(ValueError):
        call(np.zeros(()))
    with pytest.raises(ValueError):
        call(np.zeros((2,) * 9))


def test_warnings_come_before_the_device():
    import cupyimg_amd as ca
    from cupyimg_amd.skimage import feature
    with pytest.warns(FutureWarning, match="indices argument is deprecated"):
        with pytest.raises(NotImplementedError):
            feature.peak_local_max(IMAGE, indices=False, labels=IMAGE)
    with pytest.warns(FutureWarning, match="indices argument is deprecated"):
        with pytest.raises(NotImplementedError):
            feature.peak_local_max(IMAGE, 1, None, None, True, True, labels=IMAGE)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(NotImplementedError):
            feature.peak_local_max(IMAGE, labels=IMAGE)
        with pytest.raises(NotImplementedError):
            feature.corner_peaks(IMAGE, indices=False, labels=IMAGE)         # the reference's corner_peaks does not warn
    for kw in (dict(min_distance=0), dict(min_distance=0, footprint=np.ones((1, 1), bool)), dict(min_distance=-1)):
        with pytest.warns(RuntimeWarning, match="When min_distance < 1"):
            try:
                feature.peak_local_max(IMAGE, **kw)
            except Exception:
                assert not ca.is_available()            # the warning came before the upload that failed
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        try:
            feature.peak_local_max(IMAGE, min_distance=0, footprint=np.ones((3, 3), bool))
        except Exception:
            assert not ca.is_available()


def test_ensure_spacing_checks_need_no_device():
    from cupyimg_amd.skimage import feature
    pts = np.zeros((3, 2), np.int64)
    with pytest.raises(ValueError, match="p_norm"):
        feature._ensure_spacing(pts, (5, 5), 2, p_norm=3)
    with pytest.raises(ValueError, match="spacing"):
        feature._ensure_spacing(pts, (5, 5), 2.5)


def test_library_refuses_bad_descriptors_without_a_device():
    """the checks of the entry points run before anything is queued"""
    from cupyimg_amd import _lib
    lib = _lib.load()
    size = {10: 8, 9: 4, 7: 8, 5: 4, 2: 1, 0: 1, 11: 2}

    def desc(shape, dtype_code=9, data=0x10000, row_stride=None):
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
    nbytes, total, equal = ctypes.c_int64(), ctypes.c_int64(7), ctypes.c_int64(7)
    assert lib.mi_select_work_bytes(2 ** 31, ref(nbytes)) == _lib.MI_ERR_UNSUPPORTED
    assert lib.mi_select_work_bytes(-1, ref(nbytes)) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_select_work_bytes(2 ** 31 - 1, ref(nbytes)) == 0 and 0 < nbytes.value < 2 ** 24
    assert lib.mi_select_work_bytes(100, ref(nbytes)) == 0 and nbytes.value == 64 + 8
    a, work, out = desc((4, 5)), desc((4096,), 2, 0x20000), desc((3,), 7, 0x30000)
    huge = desc((2 ** 16, 2 ** 15))
    assert lib.mi_select_count(ref(huge), ref(work), ref(total), None) == _lib.MI_ERR_UNSUPPORTED              # 2^31 elements
    assert lib.mi_select_count(ref(desc((4, 5), 11)), ref(work), ref(total), None) == _lib.MI_ERR_INVALID_ARG     # float16
    assert lib.mi_select_count(ref(desc((4, 5), row_stride=24)), ref(work), ref(total), None) == _lib.MI_ERR_NOT_CONTIGUOUS
    assert lib.mi_select_count(ref(a), ref(desc((8,), 2, 0x20000)), ref(total), None) == _lib.MI_ERR_INVALID_ARG  # a short work block
    assert lib.mi_select_count(ref(desc((0, 5))), ref(work), ref(total), None) == 0 and total.value == 0           # empty: no launch
    assert lib.mi_select_write(ref(a), ref(work), ref(out), 3, None) == _lib.MI_ERR_INVALID_ARG                   # layout
    assert lib.mi_select_write(ref(a), ref(work), ref(desc((3,), 5, 0x30000)), 0, None) == _lib.MI_ERR_INVALID_ARG  # int32 output
    assert lib.mi_select_write(ref(a), ref(work), ref(desc((3, 3), 7, 0x30000)), 1, None) == _lib.MI_ERR_INVALID_ARG  # three columns, rank 2
    assert lib.mi_select_write(ref(a), ref(work), ref(desc((3, 2), 7, 0x30000)), 2, None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_argsort(ref(a), ref(out), None, 0, None) == _lib.MI_ERR_INVALID_ARG                              # 2-D
    line = desc((20,))
    assert lib.mi_argsort(ref(line), None, None, 0, None) == _lib.MI_ERR_INVALID_ARG                               # no output
    assert lib.mi_argsort(ref(line), ref(out), None, 0, None) == _lib.MI_ERR_INVALID_ARG                           # a short output
    assert lib.mi_argsort(ref(line), None, ref(desc((20,), 10, 0x30000)), 0, None) == _lib.MI_ERR_INVALID_ARG      # another dtype
    assert lib.mi_argsort(ref(line), None, ref(desc((20,))), 0, None) == _lib.MI_ERR_INVALID_ARG                   # in place
    assert lib.mi_argsort(ref(desc((20,), 11)), ref(desc((20,), 7, 0x30000)), None, 0, None) == _lib.MI_ERR_INVALID_ARG
    idx = desc((3,), 7, 0x40000)
    flag = ctypes.c_void_p(0x50000)
    assert lib.mi_take(ref(a), ref(idx), ref(desc((3,), 9, 0x30000)), 1, None, None) == _lib.MI_ERR_INVALID_ARG   # no flag
    assert lib.mi_take(ref(a), ref(desc((3,), 5, 0x40000)), ref(desc((3,), 9, 0x30000)), 1, flag, None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_take(ref(a), ref(idx), ref(desc((3,), 10, 0x30000)), 1, flag, None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_take(ref(a), ref(idx), ref(desc((3, 3), 9, 0x30000)), 3, flag, None) == _lib.MI_ERR_INVALID_ARG # 20 elements are no rows of 3
    assert lib.mi_take(ref(a), ref(idx), ref(desc((3, 5), 9, 0x30000)), 4, flag, None) == _lib.MI_ERR_INVALID_ARG
    border = (ctypes.c_int64 * 8)(0, -1)
    assert lib.mi_peak_count(ref(desc((4, 5), 0)), None, 0.0, None, ref(work), ref(total), ref(equal), None) == _lib.MI_ERR_INVALID_ARG   # bool
    assert lib.mi_peak_count(ref(a), ref(desc((4, 5), 10, 0x60000)), 0.0, None, ref(work), ref(total), ref(equal), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_peak_count(ref(a), ref(desc((5, 4), 9, 0x60000)), 0.0, None, ref(work), ref(total), ref(equal), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_peak_count(ref(a), None, 0.0, border, ref(work), ref(total), ref(equal), None) == _lib.MI_ERR_INVALID_ARG               # negative border
    assert lib.mi_peak_count(ref(huge), None, 0.0, None, ref(work), ref(total), ref(equal), None) == _lib.MI_ERR_UNSUPPORTED
    coords, vals = desc((3, 2), 7, 0x30000), desc((3,), 9, 0x70000)
    assert lib.mi_peak_write(ref(a), None, 0.0, None, ref(work), ref(desc((3, 3), 7, 0x30000)), ref(vals), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_peak_write(ref(a), None, 0.0, None, ref(work), ref(coords), ref(desc((4,), 9, 0x70000)), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_peak_write(ref(a), None, 0.0, None, ref(work), ref(coords), ref(desc((3,), 10, 0x70000)), None) == _lib.MI_ERR_INVALID_ARG
    grid, status, bad = desc((4, 5), 5, 0x80000), desc((3,), 2, 0x90000), ctypes.c_int()
    assert lib.mi_spacing_init(ref(coords), ref(desc((4, 5), 9, 0x80000)), ref(status), ref(bad), None) == _lib.MI_ERR_INVALID_ARG          # a float map
    assert lib.mi_spacing_init(ref(desc((3, 3), 7, 0x30000)), ref(grid), ref(status), ref(bad), None) == _lib.MI_ERR_INVALID_ARG            # rank
    assert lib.mi_spacing_init(ref(coords), ref(grid), ref(desc((4,), 2, 0x90000)), ref(bad), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_spacing_rounds(ref(coords), ref(grid), ref(status), 2, 3, 0, 1, ref(bad), None) == _lib.MI_ERR_INVALID_ARG                # p_norm
    assert lib.mi_spacing_rounds(ref(coords), ref(grid), ref(status), -1, 0, 0, 1, ref(bad), None) == _lib.MI_ERR_INVALID_ARG
    assert lib.mi_spacing_rounds(ref(coords), ref(grid), ref(status), 2, 0, 0, 0, ref(bad), None) == _lib.MI_ERR_INVALID_ARG                # no round
    assert lib.mi_scatter_true(ref(coords), ref(desc((4, 5), 2, 0xA0000)), None) == _lib.MI_ERR_INVALID_ARG                                  # a uint8 mask
