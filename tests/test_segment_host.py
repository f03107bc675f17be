"""cupyimg_amd.skimage.segmentation boundaries / relabelling, skimage.util.map_array and core.unique without a GPU: the names
exist with the reference's signatures, and every argument error that needs no device is raised before any device work (this
machine may have no device at all)."""
import inspect
import re

import numpy as np
import pytest

# cupyimg/skimage/segmentation/boundaries.py:50, 186; _join.py:5, 49; cupyimg/skimage/util/_map_array.py:28
SIGNATURES = {
    "find_boundaries": "(label_img, connectivity=1, mode='thick', background=0)",
    "mark_boundaries": "(image, label_img, color=(1, 1, 0), outline_color=None, mode='outer', background_label=0, *, order=3)",
    "relabel_sequential": "(label_field, offset=1)",
    "join_segmentations": "(s1, s2)",
}


@pytest.fixture(scope="module")
def seg():
    from cupyimg_amd.skimage import segmentation
    return segmentation


@pytest.fixture(scope="module")
def util():
    from cupyimg_amd.skimage import util
    return util


def test_names_and_signatures(seg, util):
    import cupyimg_amd as ca
    import cupyimg_amd.skimage as sk
    from cupyimg_amd.skimage.segmentation import _boundaries, _join
    assert sk.util is util and sk.segmentation is seg
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(seg, name))) == sig
        assert name in _boundaries.__all__ + _join.__all__
    assert callable(seg.last_boundary_launches)
    assert util.__all__ == ["map_array", "ArrayMap"]
    assert str(inspect.signature(util.map_array)) == "(input_arr, input_vals, output_vals, out=None)"
    for attr in ("__len__", "dtype", "__repr__", "__str__", "__call__", "__getitem__", "__array__", "__setitem__"):
        assert hasattr(util.ArrayMap, attr)
    assert str(inspect.signature(ca.unique)) == "(a, return_index=False, return_inverse=False, return_counts=False)"
    assert ca.unique is ca.core.unique


def test_entry_points_are_declared_and_bound():
    import os
    from cupyimg_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mi355img.h")).read()
    debug = open(os.path.join(root, "include", "mi355img_debug.h")).read()
    for name in ("mi_find_boundaries", "mi_find_boundaries_subpixel", "mi_paint_boundaries", "mi_map_array_table", "mi_map_array_search",
                 "mi_unique_heads", "mi_unique_counts", "mi_unique_inverse", "mi_join_key"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert re.search(r"\bint\s+mi_debug_set_boundaries\s*\(\s*int\s+small_tiles\s*,\s*int\s+force_generic\s*\)\s*;", debug)
    assert re.search(r"\bint\s+mi_debug_segment_launches\s*\(\s*void\s*\)\s*;", debug)
    assert _lib.load().mi_debug_segment_launches() >= 0
    flags = dict(_build.SOURCES)
    assert flags["segment.hip"] == flags["regionprops.hip"]


def test_find_boundaries_argument_errors_come_before_any_device_work(seg):
    labels = np.zeros((6, 7), np.uint8)
    for connectivity in (0, 3, -1, 1.5):
        with pytest.raises(ValueError):
            seg.find_boundaries(labels, connectivity=connectivity)
    with pytest.raises(ValueError):
        seg.find_boundaries(np.zeros((4, 5, 6), np.int32), connectivity=4)
    with pytest.raises(ValueError):
        seg.find_boundaries(labels, mode="thin")
    for dtype in (np.float32, np.float64, np.float16):
        with pytest.raises(TypeError):
            seg.find_boundaries(labels.astype(dtype))
        with pytest.raises(TypeError):
            seg.find_boundaries(labels.astype(dtype), mode="subpixel")
    with pytest.raises(ValueError):
        seg.find_boundaries(np.uint8(3))
    # the size guard of the subpixel output: 2^31 voxels or more (a zero-stride view: no memory behind it)
    with pytest.raises(ValueError):
        seg.find_boundaries(np.broadcast_to(np.uint8(0), (2 ** 15 + 1, 2 ** 14 + 1)), mode="subpixel")
    with pytest.raises(ValueError):
        seg.find_boundaries(np.zeros((0, 4), np.uint8), mode="subpixel")


def test_mark_boundaries_argument_errors_come_before_any_device_work(seg):
    labels = np.zeros((6, 7), np.uint8)
    for dtype in (np.int8, np.int16, np.int32, np.uint32, np.int64, np.float16):
        with pytest.raises(ValueError):
            seg.mark_boundaries(np.zeros((6, 7), dtype), labels)
    for shape in ((6,), (6, 7, 4), (6, 7, 3, 1)):
        with pytest.raises(ValueError):
            seg.mark_boundaries(np.zeros(shape), labels)
    with pytest.raises(ValueError):
        seg.mark_boundaries(np.zeros((6, 7)), labels, color=(1, 1))
    with pytest.raises(ValueError):
        seg.mark_boundaries(np.zeros((6, 7)), labels, outline_color=(1, 1, 1, 1))


def test_relabel_and_join_argument_errors_come_before_any_device_work(seg):
    labels = np.array([1, 1, 5, 5, 8, 99, 42, 0])
    for offset in (0, -3):
        with pytest.raises(ValueError):
            seg.relabel_sequential(labels, offset=offset)
    for bad in (labels.astype(float), labels.astype(np.float32), labels > 2):
        with pytest.raises(TypeError):
            seg.relabel_sequential(bad)
        with pytest.raises(TypeError):
            seg.join_segmentations(bad, labels)
    with pytest.raises(ValueError):
        seg.join_segmentations(np.zeros((3, 4), np.int32), np.zeros((2, 4), np.int32))


def test_map_array_and_unique_argument_errors_come_before_any_device_work(util):
    import cupyimg_amd as ca
    from cupyimg_amd.skimage.util import _map_array
    with pytest.raises(ValueError):
        _map_array.set_route("hash")
    assert _map_array.LDS_MAX_RANGE <= 16384 <= _map_array.TABLE_MAX_RANGE <= 2 ** 31
    for bad in (np.zeros((3, 4)), np.zeros((3, 4), np.float32), np.zeros((3, 4), bool)):
        with pytest.raises(TypeError):
            util.map_array(bad, np.arange(3), np.arange(3.0))
    for bad in (np.zeros(5), np.zeros((2, 3), np.float32)):
        with pytest.raises(TypeError):
            ca.unique(bad)
    if not ca.is_available():
        with pytest.raises(Exception):
            util.map_array(np.zeros((3, 4), np.int32), np.arange(3), np.arange(3.0))
        with pytest.raises(Exception):
            ca.unique(np.arange(5))
