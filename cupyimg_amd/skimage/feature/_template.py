"""skimage.feature.match_template (cupyimg/skimage/feature/template.py) as one launch of csrc/template.hip."""
import ctypes
import math
import numbers

import numpy as np

from ... import core, _lib
from ...scipy.ndimage import _support as S

__all__ = ["match_template"]

# numpy.pad's mode -> the index map of include/mi355img.h that extends an array the same way
_PAD_MODES = {"constant": "constant", "edge": "nearest", "reflect": "mirror", "symmetric": "reflect", "wrap": "grid-wrap"}
_OTHER_PAD_MODES = ("linear_ramp", "maximum", "mean", "median", "minimum", "empty")
_MAX_VOXELS = 2 ** 31
# what the kernels load as it is; every other real dtype is converted on the device first
_NATIVE = (np.uint8, np.uint16, np.int16, np.float32, np.float64)
_CONVERTED = {np.dtype(np.bool_): np.uint8, np.dtype(np.int8): np.int16, np.dtype(np.float16): np.float32}


def _shape_dtype(a):
    """(array or None, shape, dtype) of a device array or anything array-like on the host, without touching the device"""
    if isinstance(a, core.ndarray):
        return a, tuple(a.shape), np.dtype(a.dtype)
    a = np.asarray(a)
    return a, a.shape, a.dtype


def _check_args(image_shape, image_dtype, template_shape, template_dtype, mode, constant_values):
    """every check of match_template's arguments, on shapes and dtypes alone"""
    for name, shape, dtype in (("image", image_shape, image_dtype), ("template", template_shape, template_dtype)):
        if dtype.kind == "c":
            raise TypeError("Complex type not supported")
        if dtype.kind not in "biuf":
            raise TypeError("match_template takes arrays of a real dtype, not {} ({})".format(dtype, name))
    if math.prod(image_shape) == 0:
        raise ValueError("The parameter `image` cannot be an empty array")
    if len(image_shape) not in (2, 3):
        raise ValueError("The parameter `image` must be a 2-or-3-dimensional array")
    if len(image_shape) < len(template_shape):
        raise ValueError("Dimensionality of template must be less than or equal to the dimensionality of image.")
    if math.prod(template_shape) == 0:
        raise ValueError("The parameter `template` cannot be an empty array")
    if any(si < st for si, st in zip(image_shape, template_shape)):
        raise ValueError("Image must be larger than template.")
    if len(template_shape) < len(image_shape):
        raise ValueError("template must have the image's number of dimensions ({}), got {}".format(len(image_shape), len(template_shape)))
    if not isinstance(mode, str) or mode not in _PAD_MODES:
        if mode in _OTHER_PAD_MODES:
            raise NotImplementedError("mode {!r} is not supported: constant, edge, reflect, symmetric and wrap are".format(mode))
        raise ValueError("mode {!r} is not a mode of numpy.pad".format(mode))
    if isinstance(constant_values, (core.ndarray, np.ndarray)) and constant_values.ndim == 0:
        constant_values = constant_values.item() if isinstance(constant_values, np.ndarray) else constant_values.get().item()
    if isinstance(constant_values, (list, tuple, dict, core.ndarray, np.ndarray)):
        raise NotImplementedError("constant_values must be one scalar; a value per axis or side is not supported")
    if isinstance(constant_values, (bool, np.bool_)):
        constant_values = int(constant_values)
    if not isinstance(constant_values, (numbers.Real, np.integer, np.floating)):
        raise TypeError("constant_values must be a real scalar, got {!r}".format(constant_values))
    if math.prod(image_shape) >= _MAX_VOXELS:
        raise ValueError("match_template: images of 2**31 voxels or more are not supported; got shape {}".format(tuple(image_shape)))
    return float(constant_values)


def match_template(image, template, pad_input=False, mode="constant", constant_values=0):
    """Match a template to a 2-D or 3-D image using normalized correlation (template.py:38-205): the correlation coefficient,
    between -1 and 1, of the template and the window of the image under it, as a fresh C-contiguous float64 device array.  With
    `pad_input` the output has the image's shape and a match is reported at the template's centre; otherwise the shape is
    `image.shape - template.shape + 1` and a match is reported at the template's origin.  `mode` and `constant_values` are
    numpy.pad's: how the image continues outside with `pad_input` ('constant', 'edge', 'reflect', 'symmetric', 'wrap').

    `image` and `template` are device arrays or anything array-like on the host, of any real dtype (integers, float16 and bool
    are taken at their values, nothing is rescaled; a strided view is compacted first).

    One launch (mi_match_template, csrc/template.hip); the padded image, the integral images, the cross-correlation and the
    denominator of the reference never exist in memory.  The contract is the reference's formula evaluated in float64.  Per axis
    the window of output index o starts at image index o - t // 2 with `pad_input`, else at o (t the template's extent); a sample
    outside the image is the one numpy.pad puts there, reflected or wrapped as often as it takes.  Over the window, every sample
    converted to float64 first, every product and sum rounded on its own, the taps in raster order:

        x = sum(I * T),  s1 = sum(I),  s2 = sum(I * I)
        mean = template.mean(),  V = template.size,  ssd = sum((template - mean) ** 2)      (NumPy, float64, on the host)
        num = x - s1 * mean
        d = s2 - (s1 * s1) / V;  d = d * ssd;  d = maximum(d, 0);  den = sqrt(d)
        r = num / den where den > finfo(float64).eps, else 0.0

    A window that holds a NaN or an infinity gives 0.0 (NaN fails `den > eps`, as in the reference); no result is ever NaN.

    Deviations: float32 and 16-bit-or-narrower integer images are computed in float64, where the reference computes them in
    float32 (its integral images are float32 cumsums, so its window variance keeps few digits); 64-bit integers are converted to
    float64 (exact below 2**53); a template of lower rank than the image raises ValueError at once (the reference fails later,
    inside pad); of numpy.pad's modes only the five above are supported (the others raise NotImplementedError) and
    `constant_values` is one scalar; images and results of 2**31 voxels or more raise ValueError."""
    image, ishape, idtype = _shape_dtype(image)
    template, tshape, tdtype = _shape_dtype(template)
    cval = _check_args(ishape, idtype, tshape, tdtype, mode, constant_values)
    oshape = tuple(ishape) if pad_input else tuple(n - t + 1 for n, t in zip(ishape, tshape))

    thost = core.host_copy(template) if isinstance(template, core.ndarray) else template
    thost = np.ascontiguousarray(thost, dtype=np.float64)
    mean = thost.mean()
    dev = thost - mean
    dev *= dev
    ssd = np.sum(dev)

    if not isinstance(image, core.ndarray):
        image = core.asarray(image)
    if idtype.type not in _NATIVE:
        image = image.astype(_CONVERTED.get(idtype, np.float64))
    image = core.ascontiguousarray(image)
    tdev = core.asarray(thost)
    out = core.empty(oshape, np.float64)
    idesc, tdesc, odesc = image._desc(), tdev._desc(), out._desc()
    S.check(S.lib().mi_match_template(ctypes.byref(idesc), ctypes.byref(tdesc), ctypes.byref(odesc), int(bool(pad_input)),
                                      _lib.MODE_CODES[_PAD_MODES[mode]], cval, float(mean), float(ssd), None), ValueError)
    return out
