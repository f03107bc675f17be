"""relabel_sequential and join_segmentations (cupyimg/skimage/segmentation/_join.py) on `core.unique`, `map_array` and the
key kernel of csrc/segment.hip."""
import ctypes

import numpy as np

from ... import core
from ...scipy.ndimage import _support as S
from ..util._map_array import ArrayMap, map_array

__all__ = ["relabel_sequential", "join_segmentations"]


def _label_field(label_field, name="label_field"):
    if not isinstance(label_field, core.ndarray):
        label_field = core.asarray(label_field) if hasattr(label_field, "__cuda_array_interface__") else np.asarray(label_field)
    if np.dtype(label_field.dtype).kind not in "iu":
        raise TypeError("{} must have an integer dtype".format(name))
    return label_field


def _relabel(label_field, offset, input_type=None):
    """(relabeled, in_vals, out_vals, largest output value); `input_type`: the dtype the reference's rule starts from"""
    if offset <= 0:
        raise ValueError("Offset must be strictly positive.")
    label_field = core.asarray(_label_field(label_field))
    if not label_field.size:
        raise ValueError("Cannot relabel an empty array.")
    offset = int(offset)
    lo, _ = S.min_max(label_field)                     # (a double: the sign is what is asked of it)
    if lo < 0:
        raise ValueError("Cannot relabel array that contains negative values.")
    in_vals = core.unique(label_field)
    count = in_vals.size
    if count > np.iinfo(np.int32).max:
        raise ValueError("Too many unique values in label_field (the tables use 32-bit indexing).")
    out_val_dtype = np.min_scalar_type(offset + count)
    first = out_val_dtype.type(offset)
    if lo == 0:                                         # always map 0 to 0
        out_host = np.concatenate([np.zeros(1, out_val_dtype), first + np.arange(count - 1, dtype=out_val_dtype)])
    else:
        out_host = first + np.arange(count, dtype=out_val_dtype)
    # never a narrower type than the input's; the minimal unsigned type when the largest output value overflows it
    input_type = label_field.dtype if input_type is None else np.dtype(input_type)
    out_max = int(out_host[-1])
    required_type = np.min_scalar_type(out_max)
    if input_type.itemsize < required_type.itemsize or out_max > np.iinfo(input_type).max:
        output_type = required_type
    else:
        output_type = input_type
    out_vals = core.asarray(out_host.astype(output_type, copy=False))
    relabeled = core.ndarray(label_field.shape, output_type)
    map_array(label_field, in_vals, out_vals, out=relabeled)
    return relabeled, in_vals, out_vals, out_max


def relabel_sequential(label_field, offset=1):
    """Relabel arbitrary non-negative labels to offset .. offset + number_of_labels - 1, 0 staying 0 (_join.py:49-173).
    Returns (relabeled, forward_map, inverse_map), the maps as `ArrayMap`s over device arrays.  One min / max reduction,
    `unique`, and one `map_array` call."""
    relabeled, in_vals, out_vals, _ = _relabel(label_field, offset)
    return relabeled, ArrayMap(in_vals, out_vals), ArrayMap(out_vals, in_vals)


def join_segmentations(s1, s2):
    """The segmentation in which two voxels share a segment exactly when they do in both s1 and s2 (_join.py:5-46).  The
    key (m2 + 1) r1 + r2 of the relabelled fields is formed in int64 (the reference multiplies in the relabelled dtype and
    wraps, e.g. for two uint8 fields of 20 labels each); where the reference's key does not wrap, values and dtype are
    its."""
    s1, s2 = _label_field(s1, "s1"), _label_field(s2, "s2")
    if tuple(s1.shape) != tuple(s2.shape):
        raise ValueError("Cannot join segmentations of different shape. s1.shape: %s, s2.shape: %s" % (tuple(s1.shape), tuple(s2.shape)))
    result_type = np.result_type(s1.dtype, s2.dtype)
    r1, _, _, m1 = _relabel(s1, 1)
    r2, _, _, m2 = _relabel(s2, 1)
    if (m1 + 1) * (m2 + 1) >= 2 ** 63:
        raise ValueError("join_segmentations: the key (m2 + 1) * s1 + s2 does not fit int64")
    key = core.ndarray(r1.shape, np.int64)
    d1, d2, kd = r1._desc(), r2._desc(), key._desc()
    S.check(S.lib().mi_join_key(ctypes.byref(d1), ctypes.byref(d2), m2 + 1, ctypes.byref(kd), None))
    return _relabel(key, 1, input_type=result_type)[0]
