"""skimage.filters subset: gaussian (cupyimg/skimage/filters/_gaussian.py:13-145), the Hessian ridge filters meijering, sato,
frangi and hessian (cupyimg/skimage/filters/ridges.py) on the fused kernels of csrc/ridges.hip, the edge operators of
cupyimg/skimage/filters/edges.py (sobel, scharr and prewitt on the fused kernel of csrc/edges.hip) and
apply_hysteresis_threshold (cupyimg/skimage/filters/thresholding.py:1182-1227); the threshold_* functions of that file live in
_thresholding.py (csrc/threshold.hip) and are re-exported here."""
import ctypes
import math
import warnings
from collections.abc import Iterable

import numpy as np

from ... import core, _lib
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S

__all__ = ["gaussian", "compute_hessian_eigenvalues", "meijering", "sato", "frangi", "hessian",
           "sobel", "sobel_h", "sobel_v", "scharr", "scharr_h", "scharr_v", "prewitt", "prewitt_h", "prewitt_v",
           "farid", "farid_h", "farid_v", "roberts", "roberts_pos_diag", "roberts_neg_diag", "laplace",
           "apply_hysteresis_threshold"]

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


# ------------------------------------------------------------------ edge operators (edges.py)
_EDGE_WEIGHTS = np.array([1, 0, -1])
_SOBEL_SMOOTH = np.array([1, 2, 1]) / 4
_SCHARR_SMOOTH = np.array([3, 10, 3]) / 16
_PREWITT_SMOOTH = np.full((3,), 1 / 3)
_ROBERTS_PD_WEIGHTS = np.array([[1, 0], [0, -1]], dtype=np.double)
_ROBERTS_ND_WEIGHTS = np.array([[0, 1], [-1, 0]], dtype=np.double)
# Farid & Simoncelli (2004), table 1, rows 3 and 4, with the further decimals edges.py:46-49 carries
_FARID_P = np.array([[0.0376593171958126, 0.249153396177344, 0.426374573253687, 0.249153396177344, 0.0376593171958126]])
_FARID_D1 = np.asarray([[0.109603762960254, 0.276690988455557, 0, -0.276690988455557, -0.109603762960254]])
_HFARID_WEIGHTS = _FARID_D1.T * _FARID_P
_VFARID_WEIGHTS = np.copy(_HFARID_WEIGHTS.T)


def _edge_kernel(ndim, edge_dim, smooth_weights, edge_weights=_EDGE_WEIGHTS):
    """The dense 3^ndim convolution kernel of one edge axis with the reference's values (edges.py:188-191): the edge weights
    along `edge_dim`, multiplied in double by the smoothing weights along every other axis, lowest axis first (the order of
    the products matters for Prewitt's 1 / 3).  "Other" means: not equal to `edge_dim` as given, so a negative `edge_dim`
    is smoothed along the edge axis too -- the reference's behaviour, kept."""
    def along(weights, axis):
        return np.asarray(weights).reshape([3 if a == axis % ndim else 1 for a in range(ndim)])

    if not -ndim <= edge_dim < ndim:
        raise IndexError("axis {} is out of range for rank {}".format(edge_dim, ndim))
    kernel = along(edge_weights, edge_dim)
    for axis in range(ndim):
        if axis != edge_dim:
            kernel = kernel * along(smooth_weights, axis)
    return kernel


def _edge_axes(axis, ndim):
    """(edge axes, whether the magnitude is returned): all axes for None, one for a scalar (the signed response), a sequence
    as given -- the magnitude whenever it names more than one (edges.py:172-178)"""
    axes = list(range(ndim)) if axis is None else ([axis] if np.isscalar(axis) else list(axis))
    if not axes:
        raise ValueError("axis must name at least one axis")
    return axes, len(axes) > 1


def _edge_mode(mode):
    """one boundary mode: a sequence is accepted when all its entries are equal (our convolve takes one mode)"""
    if not isinstance(mode, str):
        modes = list(mode)
        if not modes or any(m != modes[0] for m in modes):
            raise ValueError("the edge filters take one boundary mode for all axes, got {!r}".format(mode))
        mode = modes[0]
    S.check_mode(mode)
    return mode


def _laplace_operator(ndim):
    """The discrete Laplace operator the reference convolves with (the impulse response of restoration/uft.py::laplacian):
    3^ndim zeros, 2 ndim at the centre and -1 at the centre's 2 ndim axis neighbours.  laplace's `ksize` only sizes the
    transfer function returned next to it, which edges.py:711 throws away."""
    op = np.zeros((3,) * ndim)
    centre = [1] * ndim
    op[tuple(centre)] = 2.0 * ndim
    for axis in range(ndim):
        for side in (0, 2):
            op[tuple(centre[:axis] + [side] + centre[axis + 1:])] = -1.0
    return op


def _host_ndim(image):
    return image.ndim if isinstance(image, core.ndarray) else np.ndim(image)


def _check_2d(image):
    """_shared/utils.py check_nD(image, 2) on the rank alone, before anything touches the device"""
    if _host_ndim(image) != 2:
        raise ValueError("The parameter `image` must be a 2-dimensional array")


def _edge_input(image):
    """device array, img_as_float (float32 stays, integers scale to float64; float16 is computed in float32, the
    convention of the ridge filters), C-contiguous"""
    image = _img_as_float(_device(image))
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    if image.ndim < 1 or image.ndim > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    return core.ascontiguousarray(image)


def _eroded_mask(mask, shape):
    """edges.py:61-63: the mask eroded with the full-connectivity structure, border value 0; None stays None"""
    if mask is None:
        return None
    mask = S.as_device(mask, "mask")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError("mask and image must have one shape")
    selem = ndi.generate_binary_structure(mask.ndim, mask.ndim)
    return core.ascontiguousarray(ndi.binary_erosion(mask, selem, border_value=0))


def _mask_filter_result(result, mask):
    """edges.py:55-65: result *= eroded mask, as a multiplication (-x * 0 = -0.0, NaN * 0 = NaN)"""
    mask = _eroded_mask(mask, result.shape)
    if mask is None:
        return result
    return S.elementwise("multiply", result, mask, core.empty(result.shape, result.dtype))


def _generic_edge_filter(image, smooth_weights, axis, mode, cval, mask):
    """edges.py:128-200 and :55-65 as one call of mi_edge_filter"""
    mode = _edge_mode(mode)
    ndim = _host_ndim(image)
    if ndim < 1:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    axes, magnitude = _edge_axes(axis, ndim)
    if len(axes) > _lib.MI_MAX_NDIM:
        raise ValueError("at most {} edge axes".format(_lib.MI_MAX_NDIM))
    flip = (slice(None, None, -1),) * ndim
    weights = np.concatenate([np.ascontiguousarray(_edge_kernel(ndim, a, smooth_weights)[flip], dtype=np.float64).ravel()
                              for a in axes])
    image = _edge_input(image)
    mask = _eroded_mask(mask, image.shape)
    out = core.empty(image.shape, np.float64)
    if image.size == 0:
        return out
    S.check_cval(mode, cval, False)
    _, wp = S.c_doubles(weights)
    idesc, odesc = image._desc(), out._desc()
    mdesc = mask._desc() if mask is not None else None
    S.check(S.lib().mi_edge_filter(ctypes.byref(idesc), ctypes.byref(odesc), ctypes.byref(mdesc) if mdesc is not None else None,
                                   wp, len(axes), int(magnitude), S.mode_code(mode), float(cval), None), ValueError)
    return out


_EDGE_DOC = """Find edges with the {name} filter (edges.py:{lines}): per edge axis the dense 3^ndim kernel -- [1, 0, -1] along the
    axis times {smooth} along the others -- applied as `ndi.convolve` does, rounded to the image's float dtype; `axis=None` or
    a sequence longer than one gives the magnitude sqrt(sum of the squares / ndim) (by the rank, also for a sequence), a
    scalar `axis` the signed response.  float64, a new device array, in both cases.  `mask`: the result is multiplied by
    the mask eroded with the full-connectivity structure (-x * 0 = -0.0 and NaN * 0 = NaN, as in the reference).

    Images and volumes take one launch that reads the image once and writes the result once (csrc/edges.hip); other
    ranks one dense convolution per axis plus per-voxel passes, with the same bits.  Deviations from the reference:
    `cval` is honoured (the reference accepts and drops it; with the default 0.0 the two agree); float16 images are
    computed in float32; a sequence of modes must hold one mode.  As in the reference a negative `axis` also smooths
    along the edge axis (it is not removed from the smoothing axes)."""


def sobel(image, mask=None, *, axis=None, mode="reflect", cval=0.0):
    return _generic_edge_filter(image, _SOBEL_SMOOTH, axis, mode, cval, mask)


def scharr(image, mask=None, *, axis=None, mode="reflect", cval=0.0):
    return _generic_edge_filter(image, _SCHARR_SMOOTH, axis, mode, cval, mask)


def prewitt(image, mask=None, *, axis=None, mode="reflect", cval=0.0):
    return _generic_edge_filter(image, _PREWITT_SMOOTH, axis, mode, cval, mask)


sobel.__doc__ = _EDGE_DOC.format(name="Sobel", lines="203-257", smooth="[1, 2, 1] / 4")
scharr.__doc__ = _EDGE_DOC.format(name="Scharr", lines="320-379", smooth="[3, 10, 3] / 16")
prewitt.__doc__ = _EDGE_DOC.format(name="Prewitt", lines="451-507", smooth="[1/3, 1/3, 1/3]")


def sobel_h(image, mask=None):
    """Horizontal edges of a 2-D image: sobel(image, mask=mask, axis=0) (edges.py:260-287)."""
    _check_2d(image)
    return sobel(image, mask=mask, axis=0)


def sobel_v(image, mask=None):
    """Vertical edges of a 2-D image: sobel(image, mask=mask, axis=1) (edges.py:290-317)."""
    _check_2d(image)
    return sobel(image, mask=mask, axis=1)


def scharr_h(image, mask=None):
    """Horizontal edges of a 2-D image: scharr(image, mask=mask, axis=0) (edges.py:382-414)."""
    _check_2d(image)
    return scharr(image, mask=mask, axis=0)


def scharr_v(image, mask=None):
    """Vertical edges of a 2-D image: scharr(image, mask=mask, axis=1) (edges.py:417-448)."""
    _check_2d(image)
    return scharr(image, mask=mask, axis=1)


def prewitt_h(image, mask=None):
    """Horizontal edges of a 2-D image: prewitt(image, mask=mask, axis=0) (edges.py:510-537)."""
    _check_2d(image)
    return prewitt(image, mask=mask, axis=0)


def prewitt_v(image, mask=None):
    """Vertical edges of a 2-D image: prewitt(image, mask=mask, axis=1) (edges.py:540-567)."""
    _check_2d(image)
    return prewitt(image, mask=mask, axis=1)


def _convolve_masked(image, weights, mask):
    """ndi.convolve with fixed weights (mode 'reflect') in the image's float dtype, then the mask"""
    image = _edge_input(image)
    return _mask_filter_result(ndi.convolve(image, weights), mask)


def _pair_magnitude(a, b):
    """sqrt(a * a + b * b) / sqrt(2) in the arrays' dtype, in the operation order of edges.py:601-609 / 761-768"""
    out = core.empty(a.shape, a.dtype)
    if a.size:
        ad, bd, od = a._desc(), b._desc(), out._desc()
        S.check(S.lib().mi_edge_pair_magnitude(ctypes.byref(ad), ctypes.byref(bd), ctypes.byref(od), math.sqrt(2), None), ValueError)
    return out


def roberts_pos_diag(image, mask=None):
    """Roberts' cross, the kernel [[1, 0], [0, -1]] (edges.py:614-645); the image's float dtype."""
    _check_2d(image)
    return _convolve_masked(image, _ROBERTS_PD_WEIGHTS, mask)


def roberts_neg_diag(image, mask=None):
    """Roberts' cross, the kernel [[0, 1], [-1, 0]] (edges.py:648-679); the image's float dtype."""
    _check_2d(image)
    return _convolve_masked(image, _ROBERTS_ND_WEIGHTS, mask)


def roberts(image, mask=None):
    """Edge magnitude by Roberts' cross operator: sqrt(pos_diag^2 + neg_diag^2) / sqrt(2), every operation in the image's
    float dtype and in the reference's order, the division after the square root (edges.py:570-611)."""
    _check_2d(image)
    return _pair_magnitude(roberts_pos_diag(image, mask), roberts_neg_diag(image, mask))


def farid_h(image, *, mask=None):
    """Horizontal edges by the 5-tap Farid & Simoncelli derivative (edges.py:772-805); the image's float dtype."""
    _check_2d(image)
    return _convolve_masked(image, _HFARID_WEIGHTS, mask)


def farid_v(image, *, mask=None):
    """Vertical edges by the 5-tap Farid & Simoncelli derivative (edges.py:808-838); the image's float dtype."""
    _check_2d(image)
    return _convolve_masked(image, _VFARID_WEIGHTS, mask)


def farid(image, *, mask=None):
    """Edge magnitude by the Farid transform: sqrt(h^2 + v^2) / sqrt(2) in the image's float dtype, the division after
    the square root (edges.py:716-769)."""
    _check_2d(image)
    return _pair_magnitude(farid_h(image, mask=mask), farid_v(image, mask=mask))


def laplace(image, ksize=3, mask=None):
    """Edges by the discrete Laplace operator, n-D (edges.py:682-713): `ndi.convolve` with the 3^ndim operator of
    restoration/uft.py::laplacian (2 ndim at the centre, -1 at its axis neighbours), built on the host without an FFT.  As in
    the reference `ksize` only sizes a transfer function that is thrown away; the operator is 3^ndim for every ksize >= 3
    (smaller ones cannot hold it and raise ValueError)."""
    if int(ksize) < 3:
        raise ValueError("ksize must be at least 3: the Laplace operator has 3 samples along every axis")
    ndim = _host_ndim(image)
    if ndim < 1:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    return _convolve_masked(image, _laplace_operator(ndim), mask)


def _threshold_arg(value, shape):
    """scalar -> (None, float); array -> (C-contiguous float64 device array of the image's shape, 0.0).  A device array stays on
    the device; a host array is broadcast and uploaded."""
    if isinstance(value, core.ndarray):
        if value.size == 1:
            return None, float(value.get().reshape(-1)[0])
        if tuple(value.shape) != tuple(shape):
            raise ValueError("a threshold array must have the image's shape")
        return core.ascontiguousarray(value if value.dtype == np.float64 else value.astype(np.float64)), 0.0
    value = np.asarray(value, dtype=np.float64)
    if value.ndim == 0:
        return None, float(value)
    return core.asarray(np.ascontiguousarray(np.broadcast_to(value, shape))), 0.0


def apply_hysteresis_threshold(image, low, high):
    """Hysteresis thresholding, n-D (thresholding.py:1182-1227): the samples above `low` that are connected (connectivity 1)
    to a sample above `high`, as a bool device array.  `low` is clipped to `high`; either may be a scalar or an array of the
    image's shape (device arrays stay on the device: the clip is part of the launch).  Both masks come from one launch, and
    the linking is `binary_propagation(image > high, mask=image > low)` on the block-wise until-stable kernel: no label
    volume and no component count read by the host (image > high lies inside image > low, so this is the set the reference
    gathers through label and sum).  Deviations: the comparisons are made in float64 for every dtype (NumPy compares a
    float32 image with a Python float in float32), so 64-bit integer images and thresholds are exact only up to 2^53;
    float16 is compared as float32."""
    image = _device(image)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    elif image.dtype in (np.int64, np.uint64):
        image = image.astype(np.float64)
    if image.ndim < 1 or image.ndim > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    image = core.ascontiguousarray(image)
    high_d, high_s = _threshold_arg(high, image.shape)
    low_d, low_s = _threshold_arg(low, image.shape)
    mask_low = core.empty(image.shape, np.bool_)
    mask_high = core.empty(image.shape, np.bool_)
    if image.size == 0:
        return mask_low
    idesc, ld, hd = image._desc(), mask_low._desc(), mask_high._desc()
    lad = low_d._desc() if low_d is not None else None
    had = high_d._desc() if high_d is not None else None
    S.check(S.lib().mi_threshold_masks(ctypes.byref(idesc), ctypes.byref(lad) if lad is not None else None,
                                       ctypes.byref(had) if had is not None else None, low_s, high_s, ctypes.byref(ld),
                                       ctypes.byref(hd), None), ValueError)
    return ndi.binary_propagation(mask_high, structure=ndi.generate_binary_structure(image.ndim, 1), mask=mask_low)


from ._thresholding import (_mean_std, threshold_isodata, threshold_li, threshold_local, threshold_mean, threshold_minimum,  # noqa: E402,F401
                            threshold_multiotsu, threshold_niblack, threshold_otsu, threshold_sauvola, threshold_triangle,
                            threshold_yen, try_all_threshold)
from . import _thresholding  # noqa: E402

__all__ += _thresholding.__all__
