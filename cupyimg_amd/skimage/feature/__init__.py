"""skimage.feature subset: the Hessian matrix and its eigenvalues (cupyimg/skimage/feature/corner.py:141-211, 260-458) on
HIP kernels (csrc/ridges.hip), and the Canny edge detector (cupyimg/skimage/feature/_canny.py) with its Sobel, magnitude and
non-maximum-suppression stage as one kernel (csrc/edges.hip)."""
import ctypes

import numpy as np

from ... import core, _lib
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ..filters import _img_as_float

__all__ = ["hessian_matrix", "hessian_matrix_eigvals", "structure_tensor_eigenvalues", "canny"]


def _as_float_device(image):
    """device array, img_as_float; float16 is computed in float32 (the deviation the TV module has)"""
    if not isinstance(image, core.ndarray):
        image = core.asarray(np.asarray(image))
    image = _img_as_float(image)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    return image


def _check_gradient_shape(shape):
    if len(shape) < 1 or len(shape) > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    if any(n < 2 for n in shape):
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")


def hessian_matrix(image, sigma=1, mode="constant", cval=0, order="rc"):
    """The elements gradient(gradient(G)[a0], axis=a1) of the Hessian of the Gaussian-smoothed image G, as a list of device
    arrays, for (a0, a1) in combinations_with_replacement(axes, 2) with axes = ndim-1 .. 0 for order 'rc' and 0 .. ndim-1
    for 'xy' (corner.py:201-209).  One launch after the Gaussian (mi_hessian_matrix); bit-identical to numpy.gradient
    applied twice to the same G.  The elements are views of one (n_elements, image.size) block."""
    image = _as_float_device(image)
    _check_gradient_shape(image.shape)
    g = core.ascontiguousarray(ndi.gaussian_filter(image, sigma=sigma, mode=mode, cval=cval))
    ne = image.ndim * (image.ndim + 1) // 2
    out = core.empty((ne, image.size), g.dtype)
    gd, od = g._desc(), out._desc()
    S.check(S.lib().mi_hessian_matrix(ctypes.byref(gd), ctypes.byref(od), int(order != "rc"), None), ValueError)
    return [out[e].reshape(image.shape) for e in range(ne)]


def _symmetric_compute_eigenvalues(elems):
    elems = [e if isinstance(e, core.ndarray) else core.asarray(np.asarray(e)) for e in elems]
    if not elems:
        raise ValueError("no elements")
    shape = elems[0].shape
    ndim = len(shape)
    if len(elems) != ndim * (ndim + 1) // 2:
        raise ValueError("{} elements do not make the upper triangle of a {} x {} matrix".format(len(elems), ndim, ndim))
    if ndim < 1 or ndim > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    dtype = np.result_type(*[e.dtype for e in elems])
    if dtype == np.float16:
        dtype = np.dtype(np.float32)
    elif dtype.kind != "f":
        dtype = np.dtype(np.float64)
    size = int(np.prod(shape))
    packed = core.empty((len(elems), size), dtype)
    for i, e in enumerate(elems):
        if e.shape != shape:
            raise ValueError("the elements must have one shape")
        packed[i] = core.ascontiguousarray(e.astype(dtype, copy=False)).reshape(size)
    out = core.empty((ndim, size), dtype)
    pd, od = packed._desc(), out._desc()
    S.check(S.lib().mi_symmetric_eigvals(ctypes.byref(pd), ctypes.byref(od), ndim, None), ValueError)
    return out.reshape((ndim,) + tuple(shape))


def hessian_matrix_eigvals(H_elems):
    """Eigenvalues of the symmetric matrices whose upper triangles are `H_elems` (as hessian_matrix returns them), in
    decreasing order along a new leading axis (corner.py:428-458).  2 x 2: the reference's closed form, bit for bit;
    larger matrices: cyclic Jacobi on the device in the elements' dtype, every eigenvalue within a few
    eps * ||H||_F of the exact one (the reference calls LAPACK in float64; its bits are not reproduced)."""
    return _symmetric_compute_eigenvalues(H_elems)


def structure_tensor_eigenvalues(A_elems):
    """Eigenvalues of a structure tensor given by its upper-triangle elements, decreasing (corner.py:338-369)."""
    return _symmetric_compute_eigenvalues(A_elems)


# ------------------------------------------------------------------ canny (_canny.py)
def _dtype_max(dtype):
    """dtype_limits(image, clip_negative=False)[1] (util/dtype.py): 1 for floats and bool, the type's maximum for integers"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f" or dtype == np.bool_:
        return 1
    if dtype.kind in "iu":
        return np.iinfo(dtype).max
    raise ValueError("cannot find the intensity range of {} images".format(dtype))


def _canny_thresholds(low_threshold, high_threshold, use_quantiles, dtype_max):
    """(low, high) as fractions: the defaults 0.1 and 0.2; given quantiles must lie in [0, 1]; given absolute thresholds are
    divided by the dtype's maximum (the rules of _canny.py:168-182)"""
    out = []
    for given, default in ((low_threshold, 0.1), (high_threshold, 0.2)):
        if given is None:
            out.append(default)
        elif not use_quantiles:
            out.append(given / dtype_max)
        elif 0.0 <= given <= 1.0:
            out.append(given)
        else:
            raise ValueError("with use_quantiles the thresholds are quantiles in [0, 1], got {!r}".format(given))
    return tuple(out)


def _percentile_plan(n, q):
    """numpy.percentile(a, q) with linear interpolation on n samples: the two order statistics and the weight NumPy's
    `_quantile` takes ((n - 1) * (q / 100), its floor, the fraction)"""
    quantile = np.true_divide(q, 100)
    virtual = (n - 1) * quantile
    if virtual >= n - 1:
        return n - 1, n - 1, 0.0
    previous = np.floor(virtual)
    return int(previous), int(previous) + 1, float(virtual - previous)


def _lerp(a, b, t):
    """numpy.lib._function_base_impl._lerp on scalars, its t >= 0.5 branch included"""
    diff = b - a
    return b - diff * (1 - t) if t >= 0.5 else a + diff * t


def _device_percentiles(magnitude, qs):
    """numpy.percentile(magnitude, q) for every q: the order statistics by the radix select of
    segmentation._percentile_40 on the device (one small read per percentile), interpolated on the host as NumPy does"""
    from ..segmentation import _WORK_BYTES
    work = core.empty((_WORK_BYTES,), np.uint8)
    mdesc = magnitude._desc()
    out = []
    for q in qs:
        k0, k1, gamma = _percentile_plan(magnitude.size, q)
        S.check(S.lib().mi_snake_order_stats(ctypes.byref(mdesc), k0, k1, ctypes.c_void_p(work.ptr), None))
        a, b = (float(v) for v in work[48:64].get().view(np.float64))
        out.append(_lerp(a, b, gamma))
    return out


def _canny_stage(smoothed, eroded, high=None, low=None):
    """mi_canny_nms: (magnitude, local_max, high_mask, low_mask) of a float64 smoothed image; no masks without thresholds"""
    magnitude = core.empty(smoothed.shape, np.float64)
    local_max = core.empty(smoothed.shape, np.bool_)
    masks = high is not None
    high_mask = core.empty(smoothed.shape, np.bool_) if masks else None
    low_mask = core.empty(smoothed.shape, np.bool_) if masks else None
    sd, ed, md, ld = smoothed._desc(), eroded._desc(), magnitude._desc(), local_max._desc()
    hd = high_mask._desc() if masks else None
    lod = low_mask._desc() if masks else None
    S.check(S.lib().mi_canny_nms(ctypes.byref(sd), ctypes.byref(ed), ctypes.byref(md), ctypes.byref(ld),
                                 ctypes.byref(hd) if masks else None, ctypes.byref(lod) if masks else None,
                                 float(high) if masks else 0.0, float(low) if masks else 0.0, None), ValueError)
    return magnitude, local_max, high_mask, low_mask


def _canny_smooth(image, mask, sigma):
    """smooth_with_function_and_mask (_canny.py:24-51) with fsmooth = img_as_float(gaussian(x, sigma, mode='constant')):
    float64 for every image dtype, because bleed_over is"""
    from ..filters import gaussian
    ones = core.ones(image.shape, np.float64) if mask is None else mask.astype(np.float64)
    bleed_over = gaussian(ones, sigma, mode="constant")
    if mask is not None:
        masked = core.empty(image.shape, image.dtype)
        idesc, mdesc, odesc = image._desc(), mask._desc(), masked._desc()
        S.check(S.lib().mi_masked_copy(ctypes.byref(idesc), ctypes.byref(mdesc), ctypes.byref(odesc), None), ValueError)
        image = masked
    smoothed = _as_float_device(gaussian(image, sigma, mode="constant"))
    smoothed = core.ascontiguousarray(smoothed)
    out = core.empty(image.shape, np.float64)
    sd, bd, od = smoothed._desc(), bleed_over._desc(), out._desc()
    S.check(S.lib().mi_canny_normalize(ctypes.byref(sd), ctypes.byref(bd), ctypes.byref(od), None), ValueError)
    return out


def canny(image, sigma=1.0, low_threshold=None, high_threshold=None, mask=None, use_quantiles=False):
    """Canny edge detector, 2-D (_canny.py:54-305): Gaussian smoothing that ignores masked pixels, Sobel gradients,
    non-maximum suppression along the four direction classes with the reference's interpolation, and hysteresis linking
    (8-connectivity) of the local maxima above `low_threshold` to those above `high_threshold` (defaults 0.1 and 0.2 of
    the dtype's maximum; quantiles of the magnitude with `use_quantiles`).  Returns a bool device array.

    After the two Gaussians and the mask erosion one launch (mi_canny_nms) reads the smoothed image once and writes the
    magnitude, the local maxima and both threshold masks; the linking is
    `binary_propagation(high_mask, structure=ones((3, 3)), mask=low_mask)`, no labelling and no count read by the host.
    With `use_quantiles` the two thresholds are numpy.percentile of the magnitude, bit for bit, from order statistics
    selected on the device (two small reads; the reference synchronises there too).

    Deviations: the magnitude is sqrt(isobel^2 + jsobel^2) with every operation rounded on its own where the reference
    calls hypot, whose last bit depends on the libm (at most 1 ulp apart on the tested images, with identical edge
    maps); float16 images are computed in float32."""
    if (image.ndim if isinstance(image, core.ndarray) else np.ndim(image)) != 2:
        raise ValueError("The parameter `image` must be a 2-dimensional array")
    in_dtype = image.dtype if isinstance(image, (core.ndarray, np.ndarray)) else np.asarray(image).dtype
    low_threshold, high_threshold = _canny_thresholds(low_threshold, high_threshold, use_quantiles, _dtype_max(in_dtype))
    if not isinstance(image, core.ndarray):
        image = core.asarray(np.asarray(image))
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    image = core.ascontiguousarray(image)
    if mask is not None:
        mask = S.as_device(mask, "mask")
        if tuple(mask.shape) != tuple(image.shape):
            raise ValueError("mask and image must have one shape")
        mask = core.ascontiguousarray(mask if mask.dtype == np.bool_ else mask.astype(np.bool_))
    if image.size == 0:
        return core.empty(image.shape, np.bool_)
    smoothed = _canny_smooth(image, mask, sigma)
    full = core.ones(image.shape, np.bool_) if mask is None else mask
    eroded = core.ascontiguousarray(ndi.binary_erosion(full, ndi.generate_binary_structure(2, 2), border_value=0))
    if use_quantiles:
        magnitude, local_max, _, _ = _canny_stage(smoothed, eroded)
        high, low = _device_percentiles(magnitude, (100.0 * high_threshold, 100.0 * low_threshold))
        high_mask = core.empty(image.shape, np.bool_)
        low_mask = core.empty(image.shape, np.bool_)
        md, ld, hd, lod = magnitude._desc(), local_max._desc(), high_mask._desc(), low_mask._desc()
        S.check(S.lib().mi_canny_threshold(ctypes.byref(md), ctypes.byref(ld), ctypes.byref(hd), ctypes.byref(lod), high, low, None),
                ValueError)
    else:
        _, _, high_mask, low_mask = _canny_stage(smoothed, eroded, high_threshold, low_threshold)
    return ndi.binary_propagation(high_mask, structure=np.ones((3, 3), bool), mask=low_mask)
