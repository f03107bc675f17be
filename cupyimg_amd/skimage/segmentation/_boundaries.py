"""find_boundaries and mark_boundaries (cupyimg/skimage/segmentation/boundaries.py) on the kernels of csrc/segment.hip.

The reference forms `dilation != erosion` (two grey morphology launches and a compare), for mode="outer" two more on the full
window plus a masked copy and four logical passes, and for mode="subpixel" a Python loop with a `unique` per output element.
Here every mode is one launch: the closed forms are in the header of csrc/segment.hip and derived in DESIGN.md 4.20."""
import ctypes
import math

import numpy as np

from ... import core
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ..filters import _img_as_float

__all__ = ["find_boundaries", "mark_boundaries"]

_MODES = {"thick": 0, "inner": 1, "outer": 2}
_MAX_VOXELS = 2 ** 31
_boundary_launches = None


def last_boundary_launches():
    """Kernel launches the most recent `find_boundaries` call of this process queued on the label image it was given once
    that was a contiguous device array (not the upload or the compaction of a strided view).  None before the first call.
    A diagnostic for benchmarks and tests."""
    return _boundary_launches


def _launch_counter():
    fn = S.lib().mi_debug_segment_launches
    fn.argtypes = []
    fn.restype = ctypes.c_int
    return fn


def _check_args(dtype, shape, connectivity, mode):
    ndim = len(shape)
    if mode not in _MODES and mode != "subpixel":
        raise ValueError("mode must be one of 'thick', 'inner', 'outer', 'subpixel'; got {!r}".format(mode))
    if dtype.kind not in "iub":
        raise TypeError("find_boundaries takes integer and bool label images, not {}".format(dtype))
    if ndim < 1:
        raise ValueError("find_boundaries takes arrays of rank 1 to 8")
    if int(connectivity) != connectivity or not 1 <= connectivity <= ndim:
        raise ValueError("connectivity must be in 1 .. {} for a {}-dimensional image; got {!r}".format(ndim, ndim, connectivity))
    if mode == "subpixel":
        if any(s < 1 for s in shape):
            raise ValueError("find_boundaries(mode='subpixel') needs at least one sample along every axis")
        if math.prod(2 * s - 1 for s in shape) >= _MAX_VOXELS:
            raise ValueError("find_boundaries(mode='subpixel'): outputs of 2**31 voxels or more are not supported; got "
                             "shape {}".format(tuple(2 * s - 1 for s in shape)))


def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
    """Bool array that is True where regions of an integer or bool label image meet (boundaries.py:50-183).  `mode`:
    "thick", "inner", "outer" (an output of the image's shape) or "subpixel" (2 s - 1 samples per axis of s).  One kernel
    launch for every mode."""
    global _boundary_launches
    if not isinstance(label_img, core.ndarray):
        label_img = core.asarray(label_img) if hasattr(label_img, "__cuda_array_interface__") else np.asarray(label_img)
    _check_args(np.dtype(label_img.dtype), tuple(label_img.shape), connectivity, mode)
    labels = core.ascontiguousarray(core.asarray(label_img))
    count = _launch_counter()
    before = count()
    ld = labels._desc()
    if mode == "subpixel":
        shape = tuple(2 * s - 1 for s in labels.shape)
        out = core.ndarray(shape, np.bool_)
        od = out._desc()
        S.check(S.lib().mi_find_boundaries_subpixel(ctypes.byref(ld), ctypes.byref(od), None))
    else:
        out = core.ndarray(labels.shape, np.bool_)
        od = out._desc()
        info = np.iinfo(np.uint8 if labels.dtype == np.bool_ else labels.dtype)
        bg = int(background)
        has_bg = bg == background and info.min <= bg <= info.max
        bits = (bg - 2 ** 64 if bg >= 2 ** 63 else bg) if has_bg else 0
        S.check(S.lib().mi_find_boundaries(ctypes.byref(ld), int(connectivity), _MODES[mode], int(has_bg), bits, ctypes.byref(od), None))
    _boundary_launches = count() - before
    return out


def _as_float_rgb(image):
    """img_as_float(image, force_copy=True) and gray2rgb, as a fresh C-contiguous (M, N, 3) array"""
    if not isinstance(image, core.ndarray):
        image = core.asarray(image) if hasattr(image, "__cuda_array_interface__") else np.asarray(image)
    dt = np.dtype(image.dtype)
    if dt not in (np.dtype(np.bool_), np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("mark_boundaries takes bool, uint8, uint16, float32 and float64 images, not {}".format(dt))
    shape = tuple(image.shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
        raise ValueError("mark_boundaries takes (M, N) or (M, N, 3) images; got shape {}".format(shape))
    image = core.asarray(image)
    flt = _img_as_float(image)
    marked = core.ndarray(shape[:2] + (3,), flt.dtype)
    if len(shape) == 2:
        for k in range(3):
            marked[:, :, k] = flt
    else:
        marked[...] = flt
    return marked


def mark_boundaries(image, label_img, color=(1, 1, 0), outline_color=None, mode="outer", background_label=0, *, order=3):
    """(M, N, 3) float image with the boundaries of `label_img` painted in `color` (boundaries.py:186-253); with
    `outline_color`, the pixels next to a boundary in that colour.  mode="subpixel" first zooms the image to
    (2 M - 1, 2 N - 1) with this library's `zoom`."""
    color = [float(c) for c in color]
    if len(color) != 3 or (outline_color is not None and len(outline_color) != 3):
        raise ValueError("colours are length-3 sequences")
    marked = _as_float_rgb(image)
    if mode == "subpixel":
        marked = core.ascontiguousarray(ndi.zoom(marked, [2 - 1 / s for s in marked.shape[:-1]] + [1], mode="reflect", order=order))
    boundaries = find_boundaries(label_img, mode=mode, background=background_label)
    if boundaries.ndim != 2 or boundaries.shape != marked.shape[:2]:
        raise ValueError("the label image's boundaries have shape {}, the image {}".format(boundaries.shape, marked.shape[:2]))
    col, colp = S.c_doubles(color)
    outp = None
    if outline_color is not None:
        outl, outp = S.c_doubles([float(c) for c in outline_color])
    bd, md = boundaries._desc(), marked._desc()
    S.check(S.lib().mi_paint_boundaries(ctypes.byref(bd), ctypes.byref(md), colp, outp, None))
    return marked
