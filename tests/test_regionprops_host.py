"""What the region-measurement family promises without a device: the entry points are declared, exported and bound; the kernel
source is built (and is no strict-twin source); the Python layer exposes the reference's names and signatures; and every
TypeError, ValueError, NotImplementedError and warning of the argument checks is reached before anything touches the device
(the inputs below are host arrays: an upload would fail on a machine without a GPU)."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {"mi_rp_extent": 3, "mi_rp_moments": 7, "mi_rp_finish": 6, "mi_rp_keep": 7, "mi_rp_crop": 6}
EMPTY = inspect.Parameter.empty
POS, KW = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY


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
    assert re.search(r"\bint\s+mi_debug_set_regionprops\s*\(\s*int\s+\w+\s*\)\s*;", debug)
    assert re.search(r"\bint\s+mi_debug_regionprops_launches\s*\(\s*void\s*\)\s*;", debug)
    assert lib.mi_debug_set_regionprops(0) == 0
    assert lib.mi_debug_regionprops_launches() >= 0


def test_kernel_source_is_built_and_is_no_strict_twin_source():
    from cupyimg_amd import _build
    assert ("regionprops.hip", ["-ffp-contract=off"]) in _build.SOURCES
    assert "regionprops.hip" not in _build.STRICT_SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "regionprops.hip"))


def _params(fn):
    return [(n, p.default, p.kind) for n, p in inspect.signature(fn).parameters.items()]


def test_public_names_and_signatures_are_the_references():
    from cupyimg_amd.scipy import ndimage as ndi
    from cupyimg_amd.skimage import measure, morphology
    assert "find_objects" in ndi.measurements.__all__ and ndi.find_objects is ndi.measurements.find_objects
    assert _params(ndi.find_objects) == [("input", EMPTY, POS), ("max_label", 0, POS)]
    for name in ("label", "regionprops", "regionprops_table", "RegionProperties", "PROPS", "COL_DTYPES", "OBJECT_COLUMNS"):
        assert name in measure.__all__ and hasattr(measure, name)
    assert _params(measure.regionprops) == [("label_image", EMPTY, POS), ("intensity_image", None, POS), ("cache", True, POS),
                                            ("coordinates", None, POS), ("extra_properties", None, KW)]
    assert _params(measure.regionprops_table) == [("label_image", EMPTY, POS), ("intensity_image", None, POS),
                                                  ("properties", ("label", "bbox"), POS), ("cache", True, KW), ("separator", "-", KW),
                                                  ("extra_properties", None, KW)]
    for name in ("remove_small_objects", "remove_small_holes"):
        assert name in morphology.__all__
    assert _params(morphology.remove_small_objects) == [("ar", EMPTY, POS), ("min_size", 64, POS), ("connectivity", 1, POS),
                                                        ("in_place", False, POS)]
    assert _params(morphology.remove_small_holes) == [("ar", EMPTY, POS), ("area_threshold", 64, POS), ("connectivity", 1, POS),
                                                      ("in_place", False, POS)]
    assert measure.PROPS["Area"] == "area" and measure.PROPS["WeightedHuMoments"] == "weighted_moments_hu" and len(measure.PROPS) == 40
    assert measure.COL_DTYPES["area"] is int and measure.COL_DTYPES["centroid"] is float and measure.COL_DTYPES["image"] is object
    assert measure.OBJECT_COLUMNS == {"image", "coords", "convex_image", "slice", "filled_image", "intensity_image"}
    for fn in (ndi.find_objects, measure.regionprops, measure.regionprops_table, morphology.remove_small_objects, morphology.remove_small_holes):
        assert fn.__doc__


LAB2 = np.zeros((4, 5), np.int32)
LAB3 = np.zeros((3, 4, 5), np.int64)


def test_find_objects_raises_before_the_device():
    from cupyimg_amd.scipy import ndimage as ndi
    for bad in (np.zeros((3, 3)), np.zeros((3, 3), np.float32), np.zeros(3, np.float16)):
        with pytest.raises(TypeError):
            ndi.find_objects(bad)
    for empty in (np.zeros((0,), int), np.zeros((3, 0), np.uint8)):
        with pytest.raises(ValueError):
            ndi.find_objects(empty)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        ndi.find_objects(LAB2, max_label=2 ** 31)
    with pytest.raises(ValueError, match="cap"):
        ndi.find_objects(LAB2, max_label=2 ** 31 - 1)


@pytest.mark.parametrize("fn", ("regionprops", "regionprops_table"))
def test_regionprops_raises_before_the_device(fn):
    from cupyimg_amd.skimage import measure
    call = getattr(measure, fn)
    for bad in (np.zeros((5,), int), np.zeros((2, 2, 2, 2), int)):
        with pytest.raises(TypeError, match="Only 2-D and 3-D"):
            call(bad)
    with pytest.raises(TypeError, match="Non-integer image types are ambiguous"):
        call(LAB2 > 0)
    for bad in (np.zeros((4, 5)), np.zeros((4, 5), np.float32)):
        with pytest.raises(TypeError, match="Non-integer label_image"):
            call(bad)
    with pytest.raises(ValueError, match="shapes must match"):
        call(LAB2, np.zeros((2, 1)))
    with pytest.raises(NotImplementedError, match="multichannel"):
        call(LAB2, np.zeros((4, 5, 3)))
    with pytest.raises(NotImplementedError, match="extra_properties"):
        call(LAB2, extra_properties=(lambda mask: mask.sum(),))


def test_coordinates_keyword_is_the_references():
    from cupyimg_amd.skimage import measure
    with pytest.raises(ValueError, match="no longer supported"):
        measure.regionprops(LAB2, coordinates="xy")
    with pytest.warns(FutureWarning, match="coordinates keyword argument"):
        with pytest.raises(NotImplementedError):
            measure.regionprops(LAB2, coordinates="rc", extra_properties=(len,))


UNSUPPORTED = ("coords", "convex_area", "convex_image", "solidity", "feret_diameter_max", "filled_area", "filled_image", "euler_number",
               "perimeter", "perimeter_crofton")


@pytest.mark.parametrize("prop", UNSUPPORTED)
def test_unsupported_properties_raise_naming_the_property(prop):
    from cupyimg_amd.skimage import measure
    with pytest.raises(NotImplementedError, match=prop):
        measure.regionprops_table(LAB2, properties=("label", prop))


def test_table_property_checks_come_before_the_device():
    from cupyimg_amd.skimage import measure
    for prop in ("eccentricity", "moments_hu", "orientation"):
        with pytest.raises(NotImplementedError, match="3D"):
            measure.regionprops_table(LAB3, properties=(prop,))
    with pytest.raises(NotImplementedError, match="3D"):
        measure.regionprops_table(LAB3, np.zeros(LAB3.shape), properties=("weighted_moments_hu",))
    for prop in ("mean_intensity", "intensity_image", "weighted_centroid"):
        with pytest.raises(AttributeError, match="No intensity image"):
            measure.regionprops_table(LAB2, properties=(prop,))
    with pytest.raises(AttributeError):
        measure.regionprops_table(LAB2, properties=("no_such_property",))


def test_remove_small_raises_and_warns_before_the_device():
    import cupyimg_amd as ca
    from cupyimg_amd.skimage import morphology
    for fn in (morphology.remove_small_objects, morphology.remove_small_holes):
        for bad in (np.random.rand(5, 5), np.zeros((3, 3), np.float32), np.zeros(3, complex)):
            with pytest.raises(TypeError, match="Only bool or integer image types are supported"):
                fn(bad)
    with pytest.warns(UserWarning, match="returned as a boolean array"):
        try:
            morphology.remove_small_holes(np.ones((3, 3), int), 2)
        except Exception:
            assert not ca.is_available()              # the warning came before the upload that failed
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        try:
            morphology.remove_small_holes(np.ones((3, 3), bool), 2)
        except Warning:
            raise
        except Exception:
            assert not ca.is_available()


def test_library_refuses_bad_descriptors_without_a_device():
    """the checks of the entry points run before anything is queued"""
    from cupyimg_amd import _lib
    lib = _lib.load()
    size = {10: 8, 9: 4, 7: 8, 5: 4, 2: 1, 0: 1, 11: 2}

    def desc(shape, dtype_code=5, data=0x10000, row_stride=None):
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
    BAD, NC = _lib.MI_ERR_INVALID_ARG, _lib.MI_ERR_NOT_CONTIGUOUS
    lab, ext = desc((4, 5)), desc((3, 7), 7, 0x20000)
    assert lib.mi_rp_extent(ref(desc((4, 5), 9)), ref(ext), None) == BAD                              # float labels
    assert lib.mi_rp_extent(ref(desc((4, 5), row_stride=40)), ref(ext), None) == NC
    assert lib.mi_rp_extent(ref(lab), ref(desc((3, 10), 7, 0x20000)), None) == BAD                    # columns of another rank
    assert lib.mi_rp_extent(ref(lab), ref(desc((3, 7), 10, 0x20000)), None) == BAD                    # a float table
    assert lib.mi_rp_extent(ref(lab), ref(desc((0, 7), 7, 0x20000)), None) == BAD                     # no rows
    raw, cen = desc((3, 16), 10, 0x30000), desc((3, 2, 2), 10, 0x40000)
    assert lib.mi_rp_moments(ref(desc((20,))), None, ref(desc((3, 4), 7, 0x20000)), ref(raw), None, ref(cen), None) == BAD   # rank 1
    assert lib.mi_rp_moments(ref(lab), None, ref(ext), None, None, ref(cen), None) == BAD             # no table
    assert lib.mi_rp_moments(ref(lab), None, ref(ext), ref(desc((3, 64), 10, 0x30000)), None, ref(cen), None) == BAD
    assert lib.mi_rp_moments(ref(lab), None, ref(ext), ref(raw), None, ref(desc((3, 2, 3), 10, 0x40000)), None) == BAD
    assert lib.mi_rp_moments(ref(lab), ref(desc((5, 4), 9, 0x50000)), ref(ext), ref(raw), None, ref(cen), None) == BAD       # shape
    assert lib.mi_rp_moments(ref(lab), ref(desc((4, 5), 11, 0x50000)), ref(ext), ref(raw), None, ref(cen), None) == BAD      # float16
    assert lib.mi_rp_moments(ref(lab), ref(desc((4, 5), 9, 0x50000)), ref(ext), None, ref(raw), ref(cen), None) == BAD       # central needs raw
    out = desc((3, 40), 10, 0x60000)
    assert lib.mi_rp_finish(ref(ext), 4, None, None, ref(out), None) == BAD
    assert lib.mi_rp_finish(ref(ext), 3, None, None, ref(out), None) == BAD                           # the table is a rank-2 one
    assert lib.mi_rp_finish(ref(ext), 2, None, None, ref(desc((3, 96), 10, 0x60000)), None) == BAD
    assert lib.mi_rp_finish(ref(ext), 2, None, ref(desc((3, 64), 10, 0x30000)), ref(out), None) == BAD
    dst = desc((4, 5), 5, 0x70000)
    assert lib.mi_rp_keep(ref(lab), ref(lab), ref(ext), 3, 3, ref(dst), None) == BAD                  # mode
    assert lib.mi_rp_keep(ref(lab), ref(lab), ref(ext), -1, 0, ref(dst), None) == BAD
    assert lib.mi_rp_keep(ref(lab), ref(lab), ref(ext), 3, 0, ref(desc((4, 5), 2, 0x70000)), None) == BAD     # element sizes differ
    assert lib.mi_rp_keep(ref(desc((4, 6))), ref(lab), ref(ext), 3, 0, ref(dst), None) == BAD
    assert lib.mi_rp_keep(ref(lab), ref(lab), ref(ext), 3, 0, ref(desc((4, 5), 5, 0x70000, row_stride=40)), None) == NC
    origin = (ctypes.c_int64 * 8)(2, 3)
    assert lib.mi_rp_crop(ref(lab), None, 1, origin, ref(desc((3, 2), 0, 0x80000)), None) == BAD      # the box leaves the image
    assert lib.mi_rp_crop(ref(lab), None, 1, origin, ref(desc((2, 2), 2, 0x80000)), None) == BAD      # a uint8 mask
    assert lib.mi_rp_crop(ref(lab), None, 1, None, ref(desc((2, 2), 0, 0x80000)), None) == BAD
    assert lib.mi_rp_crop(ref(lab), ref(desc((4, 5), 9, 0x50000)), 1, origin, ref(desc((2, 2), 10, 0x80000)), None) == BAD
    assert lib.mi_rp_crop(ref(lab), None, 1, origin, ref(desc((2, 0), 0, 0x80000)), None) == 0        # an empty box: no launch
