"""skimage.measure.label on device arrays (cupyimg/skimage/measure/_label.py): a thin wrapper over the greyscale mode
of scipy.ndimage.label -- neighbours connect only when their values are equal, `background` voxels get label 0.
regionprops and regionprops_table (the tables of csrc/regionprops.hip) live in ._regionprops."""
import numpy as np

from ...scipy.ndimage import _support as S
from ...scipy.ndimage import measurements as _m
from ... import core
from ._regionprops import COL_DTYPES, OBJECT_COLUMNS, PROPS, RegionProperties, regionprops, regionprops_table

__all__ = ["label", "regionprops", "regionprops_table", "RegionProperties", "PROPS", "COL_DTYPES", "OBJECT_COLUMNS"]


def _get_structure(ndim, connectivity):
    if connectivity is None:
        connectivity = ndim                  # full connectivity by default
    if not 1 <= connectivity <= ndim:
        raise ValueError("Connectivity below 1 or above %d is illegal." % ndim)
    return _m._generate_binary_structure(ndim, connectivity)


def label(input, background=None, return_num=False, connectivity=None):
    """Label connected regions of an integer array (skimage.measure.label).  Returns int32 labels (and the count with
    return_num=True)."""
    input = S.as_device(input)
    structure = _get_structure(input.ndim, connectivity)
    if input.dtype.kind not in "bui":
        input = input.astype(np.int64)       # skimage works on an intp copy of non-integer images
    bg = 0 if background is None else int(background)
    labels = core.empty(input.shape, np.int32)
    if input.size == 0:
        num = 0
    else:
        num = _m._label(input, structure, labels, greyscale_mode=True, background=bg)
    if return_num:
        return labels, num
    return labels
