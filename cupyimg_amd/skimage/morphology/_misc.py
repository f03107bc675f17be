"""skimage.morphology.remove_small_objects / remove_small_holes on device arrays (reference:
cupyimg/skimage/morphology/misc.py:51-245: a bincount plus two fancy-indexing passes).

Here: the extent pass of csrc/regionprops.hip counts the voxels of every label in one sweep (integer atomics, exact), and
rp_keep_kernel writes `out = ar where count[label] >= min_size else 0` in one pointwise launch, in the caller's dtype -- or in
bool against the int32 labels `label` just produced.  Signatures, warnings and errors are the reference's; the result is exact.
Deviations: uint64 labels of 2**63 or more, and a largest label whose count table would be above 2 GiB, raise ValueError."""
import ctypes
from warnings import warn

import numpy as np

from ... import core
from ...scipy.ndimage import _support as S
from ...scipy.ndimage import measurements as _m

__all__ = ["remove_small_objects", "remove_small_holes"]


def _check_dtype_supported(ar):
    dt = _m._dtype_of(ar)
    if not (dt == bool or np.issubdtype(dt, np.integer)):
        raise TypeError("Only bool or integer image types are supported. Got %s." % dt)


def _keep(labels, src, ext, min_size, mode, out):
    """mi_rp_keep into the C-contiguous `out`"""
    la = labels._desc() if labels is not None else None
    sa = src._desc() if src is not None else None
    ea = ext._desc() if ext is not None else None
    oa = out._desc()
    S.check(S.lib().mi_rp_keep(ctypes.byref(la) if la is not None else None, ctypes.byref(sa) if sa is not None else None,
                               ctypes.byref(ea) if ea is not None else None, int(min_size), mode, ctypes.byref(oa), None), ValueError)
    return out


def _flat(a):
    """C-contiguous, rank >= 1 (a 0-d array as one element)"""
    a = core.ascontiguousarray(a)
    return a.reshape(1) if a.ndim == 0 else a


def _logical_not(a, dtype):
    """(a == 0) as 0 / 1 in `dtype`, a new C-contiguous array of a's shape"""
    out = core.empty(a.shape, dtype)
    if a.size:
        _keep(None, _flat(a), None, 0, 1, _flat(out))
    return out


def _labels_and_counts(ar, connectivity):
    """(int32 / int64 labels, extent table or None when there is nothing to count, largest label) of a bool (labelled here) or
    integer (taken as labels) device array"""
    if ar.dtype == bool:
        selem = _m._generate_binary_structure(ar.ndim, connectivity)
        labels, num = _m.label(ar, selem)
        labels = _flat(labels)
    else:
        lo, num = _m._max_label(ar, "remove_small_objects")
        if lo < 0:
            raise ValueError("Negative value labels are not supported. Try relabeling the input with `scipy.ndimage.label` or "
                             "`skimage.morphology.label`.")
        labels = _flat(_m._as_int_labels(ar))
    if num < 1:
        return labels, None, 0
    _m._check_table_rows(num, 8 * (1 + 3 * labels.ndim), "remove_small_objects")
    return labels, _m._region_extents(labels, num), num


def remove_small_objects(ar, min_size=64, connectivity=1, in_place=False):
    """Remove objects smaller than the specified size (skimage.morphology.remove_small_objects; misc.py:60-153).

    `ar` is a label image (integers, non-negative) or a bool mask, which is labelled first with
    generate_binary_structure(ar.ndim, connectivity).  Any rank.  Returns an array of ar's shape and dtype; with
    in_place=True, `ar` itself."""
    _check_dtype_supported(ar)
    ar = S.as_device(ar)
    if min_size == 0 or ar.size == 0:       # shortcut for efficiency
        return ar if in_place else ar.copy()
    labels, ext, num = _labels_and_counts(ar, connectivity)
    if num == 1 and ar.dtype != bool:
        warn("Only one label was provided to `remove_small_objects`. Did you mean to use a boolean array?")
    if ext is None:
        return ar if in_place else ar.copy()
    direct = in_place and ar._is_c_contiguous()
    out = ar if direct else core.empty(ar.shape, ar.dtype)
    if direct:
        ar._touch()
    _keep(labels, _flat(ar), ext, max(int(np.ceil(min_size)), 0), 0, _flat(out))
    if in_place and not direct:
        ar[...] = out
        return ar
    return out


def remove_small_holes(ar, area_threshold=64, connectivity=1, in_place=False):
    """Remove contiguous holes smaller than the specified size (skimage.morphology.remove_small_holes; misc.py:156-245):
    logical_not(remove_small_objects(logical_not(ar), area_threshold, connectivity)), the closing negation fused into the
    keep launch.  Returns a bool array; with in_place=True `ar` itself, in its own dtype (0 / 1), as the reference does."""
    _check_dtype_supported(ar)
    if _m._dtype_of(ar) != bool:
        warn("Any labeled images will be returned as a boolean array. Did you mean to use a boolean array?", UserWarning)
    ar = S.as_device(ar)
    if ar.size == 0:
        return ar if in_place else core.empty(ar.shape, np.bool_)
    if in_place and ar.dtype != bool:
        # the reference negates an integer image in its own dtype and hands remove_small_objects a 0 / 1 LABEL image: every
        # background voxel is then one object, whatever its connectivity
        inv = _logical_not(ar, ar.dtype)
        inv = remove_small_objects(inv, area_threshold, connectivity, True)
        ar[...] = _logical_not(inv, ar.dtype)
        return ar
    inv = _logical_not(ar, np.bool_)
    out = core.empty(ar.shape, np.bool_)
    if area_threshold == 0:
        out = _logical_not(inv, np.bool_)
    else:
        labels, ext, num = _labels_and_counts(inv, connectivity)
        if ext is None:
            out = _logical_not(inv, np.bool_)               # no hole at all
        else:
            _keep(labels, None, ext, max(int(np.ceil(area_threshold)), 0), 2, _flat(out))
    if in_place:
        ar[...] = out
        return ar
    return out
