"""skimage.filters subset: gaussian (cupyimg/skimage/filters/_gaussian.py:13-145) and the Hessian ridge filters meijering, sato,
frangi and hessian (cupyimg/skimage/filters/ridges.py) on the fused kernels of csrc/ridges.hip."""
import ctypes
import warnings
from collections.abc import Iterable

import numpy as np

from ... import core, _lib
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S

__all__ = ["gaussian", "compute_hessian_eigenvalues", "meijering", "sato", "frangi", "hessian"]

_INT_RANGE = {np.dtype(t): (np.iinfo(t).min, np.iinfo(t).max)
              for t in (np.uint8, np.uint16, np.uint32, np.int8, np.int16, np.int32)}


def _guess_spatial_dimensions(image):
    """_gaussian.py:148-172: None when (M, N, 3) is ambiguous."""
    if image.ndim == 2:
        return 2
    if image.ndim == 3 and image.shape[-1] != 3:
        return 3
    if image.ndim == 3 and image.shape[-1] == 3:
        return None
    if image.ndim == 4 and image.shape[-1] == 3:
        return 3
    raise ValueError("Expected 2D, 3D, or 4D array, got %iD." % image.ndim)


def _img_as_float(image):
    """skimage.img_as_float for the dtypes the engine carries: floats pass
    through, bool -> {0, 1}, unsigned ints scale to [0, 1], signed to [-1, 1]."""
    dt = image.dtype
    if dt.kind == "f":
        return image
    if dt == np.bool_:
        return image.astype(np.float64)
    if dt not in _INT_RANGE:
        raise ValueError("cannot convert {} images to float".format(dt))
    lo, hi = _INT_RANGE[dt]
    if dt.itemsize <= 2:
        # conversion and scaling in one pass (same arithmetic: the sample as a double, one multiply-add)
        if dt.kind == "u":
            return S.scale_shift(image, 1.0 / hi, 0.0, dtype=np.float64)
        return S.scale_shift(image, 2.0 / (hi - lo), 1.0 / (hi - lo), dtype=np.float64)
    out = image.astype(np.float64)
    if dt.kind == "u":
        return S.scale_shift(out, 1.0 / hi, 0.0)
    return S.scale_shift(out, 2.0 / (hi - lo), 1.0 / (hi - lo))      # (2 x + 1) / (hi - lo)


def convert_to_float(image, preserve_range):
    """_shared/utils.py:393-422"""
    if preserve_range:
        if image.dtype.char not in "df":
            image = image.astype(np.float64)
        return image
    return _img_as_float(image)


def gaussian(image, sigma=1, output=None, mode="nearest", cval=0, multichannel=None, preserve_range=False,
             truncate=4.0):
    """Multi-dimensional Gaussian filter; default mode 'nearest', integer images
    are converted to float, the channel axis (if any) gets sigma 0."""
    image = image if isinstance(image, core.ndarray) else core.asarray(np.asarray(image))
    try:
        spatial_dims = _guess_spatial_dimensions(image)
    except ValueError:
        spatial_dims = image.ndim
    if spatial_dims is None and multichannel is None:
        warnings.warn(RuntimeWarning("Images with dimensions (M, N, 3) are interpreted as 2D+RGB by default. "
                                     "Use `multichannel=False` to interpret as 3D image with last dimension "
                                     "of length 3."))
        multichannel = True
    if not isinstance(sigma, Iterable):
        if sigma < 0:
            raise ValueError("Sigma values less than zero are not valid")
    elif any(s < 0 for s in sigma):
        raise ValueError("Sigma values less than zero are not valid")
    if multichannel:
        if not isinstance(sigma, Iterable):
            sigma = [sigma] * (image.ndim - 1)
        if len(sigma) != image.ndim:
            sigma = tuple(sigma) + (0,)
        sigma = tuple(sigma)
    image = convert_to_float(image, preserve_range)
    if output is None:
        output = core.empty_like(image)
    elif not np.issubdtype(output.dtype, np.floating):
        raise ValueError("Provided output data type is not float")
    ndi.gaussian_filter(image, sigma, output=output, mode=mode, cval=cval, truncate=truncate)
    return output


# ------------------------------------------------------------------ Hessian ridge filters (ridges.py)
_RIDGE_EIGENVALUES, _RIDGE_FRANGI, _RIDGE_SATO, _RIDGE_MEIJERING = 0, 1, 2, 3       # MI_RIDGE_*
_RIDGE_SORTING = {"none": 0, "val": 1, "abs": 2}                                      # MI_RIDGE_SORT_*


def _check_sigmas(sigmas):
    """ridges.py:84-109"""
    if isinstance(sigmas, core.ndarray):
        sigmas = sigmas.get()
    sigmas = np.asarray(sigmas).ravel()
    if np.any(sigmas < 0.0):
        raise ValueError("Sigma values should be equal to or greater than zero.")
    return sigmas


def _check_nD(image, ndims, arg_name="image"):
    """_shared/utils.py check_nD"""
    if image.size == 0:
        raise ValueError("The parameter `%s` cannot be an empty array" % arg_name)
    if image.ndim not in ndims:
        raise ValueError("The parameter `%s` must be a %s-dimensional array"
                         % (arg_name, "-or-".join(str(n) for n in ndims)))


def _device(image):
    return image if isinstance(image, core.ndarray) else core.asarray(np.asarray(image))


def _invert(image):
    """util.invert (util/_invert.py:64-76) with signed_float=False: ~x for bool, max - x for unsigned and -1 - x for signed
    integers in their own dtype, 1 - x for floats (float16 in float32)"""
    dt = image.dtype
    if dt == np.bool_:
        return S.scale_shift(image.astype(np.float64), -1.0, 1.0)          # {0, 1} either way round img_as_float
    if dt.kind in "ui":
        top = np.iinfo(dt).max if dt.kind == "u" else -1
        out = core.empty(image.shape, dt)
        return S.elementwise("subtract", core.full(image.shape, top, dt), image, out)
    if dt == np.float16:
        image = image.astype(np.float32)
    return S.scale_shift(image, -1.0, 1.0)


def _ridge_input(image, invert):
    """device array -> C-contiguous float32 / float64 array, inverted before img_as_float as the reference does"""
    if invert:
        image = _invert(image)
    image = _img_as_float(image)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    if image.ndim < 1 or image.ndim > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    if any(n < 2 for n in image.shape):
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")
    return core.ascontiguousarray(image)


def _ridge_scale(g, out, kind, sorting, sigma, p=(0.0, 0.0, 0.0), scratch=None, slot=None):
    """mi_ridge_scale: one launch (meijering: two) from the smoothed array to `out`"""
    gd, od = g._desc(), out._desc()
    sd = scratch._desc() if scratch is not None else None
    S.check(S.lib().mi_ridge_scale(ctypes.byref(gd), ctypes.byref(od), kind, sorting, float(sigma), float(p[0]), float(p[1]),
                                   float(p[2]), ctypes.byref(sd) if sd is not None else None,
                                   ctypes.c_void_p(slot) if slot is not None else None, None), ValueError)


def _key_to_float(key):
    """the value behind mi_ridge_scale's order-preserving key (include/mi355img.h)"""
    key = int(key)
    bits = key & 0x7FFFFFFFFFFFFFFF if key >> 63 else ~key & 0xFFFFFFFFFFFFFFFF
    return float(np.array([bits], np.uint64).view(np.float64)[0])


def _ridge_filter(image, sigmas, kind, p, mode, cval, debug=None):
    """max over the scales of one response, updated in place scale by scale; image: _ridge_input's result"""
    out = core.zeros(image.shape, np.float64)
    if len(sigmas) == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    scratch = work = None
    if kind == _RIDGE_MEIJERING:
        scratch = core.empty(image.shape, image.dtype)
        work = core.empty((8 * len(sigmas),), np.uint8)
        S.check(S.lib().mi_memset(work.ptr, 0xFF, work.nbytes, None))
    for i, sigma in enumerate(sigmas):
        g = core.ascontiguousarray(ndi.gaussian_filter(image, sigma=float(sigma), mode=mode, cval=cval))
        _ridge_scale(g, out, kind, _RIDGE_SORTING["abs"], sigma, p, scratch, None if work is None else work.ptr + 8 * i)
    if debug is not None and work is not None:
        debug["aux"] = scratch                                       # of the last scale
        debug["min"] = [_key_to_float(k) for k in work.get().view(np.uint64)]
    return out


def compute_hessian_eigenvalues(image, sigma, sorting="none", mode="constant", cval=0):
    """Eigenvalues of sigma^2 times the Hessian of the Gaussian-smoothed image as a (ndim, ...) device array of the image's
    float dtype: decreasing ('none'), increasing ('val') or by magnitude ('abs') (ridges.py:112-173).  After the Gaussian
    one launch (the "eigenvalues" mode of the fused kernel): the Hessian is never stored."""
    image = _ridge_input(_device(image), False)
    g = core.ascontiguousarray(ndi.gaussian_filter(image, sigma=float(sigma), mode=mode, cval=cval))
    out = core.empty((image.ndim, image.size), image.dtype)
    _ridge_scale(g, out, _RIDGE_EIGENVALUES, _RIDGE_SORTING.get(sorting, 0), sigma)
    return out.reshape((image.ndim,) + tuple(image.shape))


def meijering(image, sigmas=range(1, 10, 2), alpha=None, black_ridges=True, mode="reflect", cval=0):
    """Meijering neuriteness (ridges.py:176-291): per scale aux = the eigenvalue of largest magnitude times the
    coefficients the reference sums for it, the response where(aux < 0, aux / min(aux), 0) with the minimum taken over the
    whole array on the device, and the maximum over the scales.  float64, a new array.  Besides the input a call holds one
    smoothed volume and one scratch volume of the image's float dtype and the float64 result."""
    sigmas = _check_sigmas(sigmas)
    image = _device(image)
    ndim = image.ndim
    if alpha is None:
        alpha = 1.0 / ndim
    image = _ridge_input(image, black_ridges)
    if ndim == 1:
        return core.zeros(image.shape, np.float64)
    return _ridge_filter(image, sigmas, _RIDGE_MEIJERING, (alpha, 0.0, 0.0), mode, cval)


def sato(image, sigmas=range(1, 10, 2), black_ridges=True, mode=None, cval=0):
    """Sato tubeness (ridges.py:294-383), 2-D and 3-D: per scale |l2| (sqrt(|l2 l3|) in 3-D) of the eigenvalues in
    increasing order where the largest is positive, else 0; the maximum over the scales.  float64, a new array."""
    image = _device(image)
    _check_nD(image, [2, 3])
    sigmas = _check_sigmas(sigmas)
    if mode is None:
        warnings.warn("Previously, sato implicitly used 'constant' as the border mode when dealing with the edge of the "
                      "array. The new behavior is 'reflect'. To recover the old behavior, use mode='constant'. To avoid "
                      "this warning, please explicitly set the mode.", category=FutureWarning, stacklevel=2)
        mode = "reflect"
    image = _ridge_input(image, not black_ridges)
    return _ridge_filter(image, sigmas, _RIDGE_SATO, (0.0, 0.0, 0.0), mode, cval)


def frangi(image, sigmas=range(1, 10, 2), scale_range=None, scale_step=None, alpha=0.5, beta=0.5, gamma=15,
           black_ridges=True, mode="reflect", cval=0):
    """Frangi vesselness (ridges.py:386-533), 2-D and 3-D: per scale the product of the plate, blob and structure factors
    of the eigenvalues ordered by magnitude, 0 where one of the larger ones is positive; the maximum over the scales.
    float64, a new array.  After each Gaussian one launch that reads the smoothed volume once and updates the result in
    place; besides the input a call holds one smoothed volume and the float64 result."""
    if scale_range is not None and scale_step is not None:
        warnings.warn("Use keyword parameter `sigmas` instead of `scale_range` and `scale_range` which will be removed in "
                      "version 0.17.", stacklevel=2)
        sigmas = np.arange(scale_range[0], scale_range[1], scale_step)
    image = _device(image)
    _check_nD(image, [2, 3])
    sigmas = _check_sigmas(sigmas)
    p = (2 * alpha ** 2, 2 * beta ** 2, 2 * gamma ** 2)
    image = _ridge_input(image, black_ridges)
    return _ridge_filter(image, sigmas, _RIDGE_FRANGI, p, mode, cval)


def hessian(image, sigmas=range(1, 10, 2), scale_range=None, scale_step=None, alpha=0.5, beta=0.5, gamma=15,
            black_ridges=True, mode=None, cval=0):
    """Hybrid Hessian filter (ridges.py:536-635): frangi, then every value <= 0 becomes 1."""
    if mode is None:
        warnings.warn("Previously, hessian implicitly used 'constant' as the border mode when dealing with the edge of the "
                      "array. The new behavior is 'reflect'. To recover the old behavior, use mode='constant'. To avoid "
                      "this warning, please explicitly set the mode.", category=FutureWarning, stacklevel=2)
        mode = "reflect"
    filtered = frangi(image, sigmas=sigmas, scale_range=scale_range, scale_step=scale_step, alpha=alpha, beta=beta,
                      gamma=gamma, black_ridges=black_ridges, mode=mode, cval=cval)
    fd = filtered._desc()
    S.check(S.lib().mi_ridge_fill_nonpositive(ctypes.byref(fd), 1.0, None))
    return filtered
