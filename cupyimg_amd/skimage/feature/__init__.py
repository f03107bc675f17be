"""skimage.feature subset: the Hessian matrix and its eigenvalues (cupyimg/skimage/feature/corner.py:141-211, 260-458) on
HIP kernels (csrc/ridges.hip), the Canny edge detector (cupyimg/skimage/feature/_canny.py) with its Sobel, magnitude and
non-maximum-suppression stage as one kernel (csrc/edges.hip), the structure tensor with the corner detectors built on it
(corner.py:18-138, 384-425, 533-830; csrc/corners.hip), and peak_local_max / corner_peaks (peak.py, corner.py:833-953) on the
device compaction, sort and greedy-spacing kernels of csrc/select.hip, and match_template (template.py; _template.py here, one
launch of csrc/template.hip)."""
import ctypes
import functools
import inspect
import warnings

import numpy as np

from ... import core, _lib
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ..filters import _img_as_float
from ._template import match_template

__all__ = ["hessian_matrix", "hessian_matrix_eigvals", "structure_tensor_eigenvalues", "canny", "structure_tensor",
           "structure_tensor_eigvals", "corner_harris", "corner_shi_tomasi", "corner_foerstner", "corner_kitchen_rosenfeld",
           "peak_local_max", "corner_peaks", "match_template"]


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


# ------------------------------------------------------------------ structure tensor and corner detectors (corner.py)
_CORNER_KINDS = {"harris_k": 0, "harris_eps": 1, "shi_tomasi": 2, "foerstner": 3, "kitchen_rosenfeld": 4}


def _ndim_of(image):
    return image.ndim if isinstance(image, (core.ndarray, np.ndarray)) else np.ndim(image)


def _row_block(rows, size, dtype):
    """an uninitialised (rows, size) block whose rows start on 16-byte boundaries (the rows of an odd-sized image are padded),
    so that a row is as good an input or output of the fused filters as an array of its own"""
    per16 = 16 // np.dtype(dtype).itemsize
    padded = -(-size // per16) * per16
    return core.empty((rows, padded), dtype)[:, :size]


def _rows_as_images(block, shape):
    return [block[e].reshape(shape) for e in range(block.shape[0])]


def _sobel_block(image, products, reverse, mode, cval, out=None):
    """mi_structure_products: the Sobel derivatives of every axis (products false) or their pairwise products as the rows of
    one block"""
    rows = image.ndim * (image.ndim + 1) // 2 if products else image.ndim
    if out is None:
        out = _row_block(rows, image.size, image.dtype)
    idesc, odesc = image._desc(), out._desc()
    S.check(S.lib().mi_structure_products(ctypes.byref(idesc), ctypes.byref(odesc), int(products), int(reverse), S.mode_code(mode),
                                          float(cval), None), ValueError)
    return out


def _check_structure_args(ndim, sigma, mode, order):
    """(order, sigmas): every check of structure_tensor's arguments, before anything touches the device"""
    if order not in (None, "rc", "xy"):
        raise ValueError("order must be 'rc' or 'xy', got {!r}".format(order))
    if order == "xy" and ndim > 2:
        raise ValueError('Only "rc" order is supported for dim > 2.')
    if ndim < 1 or ndim > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    S.check_mode(mode)
    sigmas = [float(s) for s in S.normalize_sequence(sigma, ndim)]
    if order is None:
        if ndim == 2:
            warnings.warn('deprecation warning: the default order of the structure tensor values will be "row-column" instead of '
                          '"xy" starting in skimage version 0.20. Use order="rc" or order="xy" to set this explicitly.  (Specify '
                          'order="xy" to maintain the old behavior.)', category=FutureWarning, stacklevel=3)
            order = "xy"
        else:
            order = "rc"
    return order, sigmas


def _structure_tensor_block(image, sigmas, mode, cval, order):
    image = core.ascontiguousarray(_as_float_device(image))
    products = _sobel_block(image, True, order == "xy", mode, cval)
    out = _row_block(products.shape[0], image.size, image.dtype)
    if image.size:
        for src, dst in zip(_rows_as_images(products, image.shape), _rows_as_images(out, image.shape)):
            ndi.gaussian_filter(src, sigmas, output=dst, mode=mode, cval=cval)
    return out, image.shape


def structure_tensor(image, sigma=1, mode="constant", cval=0, order=None):
    """The structure tensor's upper-triangle elements gaussian_filter(d_i * d_j, sigma) as a list of device arrays, d_a the Sobel
    derivative along axis a, for (i, j) in combinations_with_replacement(axes, 2) (corner.py:46-138).  `order` applies in 2-D
    only: 'rc' gives Arr, Arc, Acc, 'xy' gives Axx, Axy, Ayy; None means 'xy' in 2-D (with a FutureWarning, as in the
    reference) and 'rc' otherwise.  `sigma` is a scalar or one value per axis.

    One launch (mi_structure_products) reads the image once and writes the products; the derivatives never exist in memory.
    Every derivative is scipy.ndimage.sobel's own arithmetic (each 1-D pass accumulated in double and rounded to the image
    dtype), the products are formed in the image dtype, and this library's gaussian_filter smooths each of them: the result
    is bit-identical to that filter applied to the products of tests/helpers/corner_ref.py.  The elements are views of one
    (n_elements, image.size) block.  Peak memory in 3-D: the image plus two blocks of six volumes (the products and the
    smoothed elements).  Integers are scaled to float64 (img_as_float), float16 is computed in float32."""
    order, sigmas = _check_structure_args(_ndim_of(image), sigma, mode, order)
    out, shape = _structure_tensor_block(image, sigmas, mode, float(cval), order)
    return _rows_as_images(out, shape)


def structure_tensor_eigvals(Axx, Axy, Ayy):
    """(l1, l2), the larger and the smaller eigenvalue of the 2 x 2 structure tensor (corner.py:384-425; deprecated there in
    favour of structure_tensor_eigenvalues, with the same FutureWarning here)."""
    warnings.warn("deprecation warning: the function structure_tensor_eigvals is deprecated and will be removed in version 0.20. "
                  "Please use structure_tensor_eigenvalues instead.", category=FutureWarning, stacklevel=2)
    if any(_ndim_of(e) != 2 for e in (Axx, Axy, Ayy)):
        raise ValueError("structure_tensor_eigvals takes the three elements of a 2-D structure tensor")
    eigs = _symmetric_compute_eigenvalues([Axx, Axy, Ayy])
    return eigs[0], eigs[1]


def _require_2d(image, name):
    if _ndim_of(image) != 2:
        raise ValueError("{} takes 2-dimensional images".format(name))


def _corner_response(block, shape, kind, out_dtype, k=0.0, eps=0.0):
    """mi_corner_response: one pointwise launch over the rows of `block`"""
    outs = [core.empty(shape, out_dtype) for _ in range(2 if kind == "foerstner" else 1)]
    bdesc, descs = block._desc(), [o._desc() for o in outs]
    S.check(S.lib().mi_corner_response(ctypes.byref(bdesc), ctypes.byref(descs[0]), ctypes.byref(descs[1]) if len(descs) > 1 else None,
                                       _CORNER_KINDS[kind], float(k), float(eps), None), ValueError)
    return outs


def corner_harris(image, method="k", k=0.05, eps=1e-6, sigma=1):
    """Harris corner response, 2-D (corner.py:593-671): det(A) - k * trace(A)^2 for method 'k', 2 * det(A) / (trace(A) + eps)
    for 'eps', A = structure_tensor(image, sigma, order='rc') with its default mode 'constant'.  One pointwise launch after the
    tensor, every operation in the elements' dtype in the reference's order (`k` and `eps` act as weak scalars: a float32
    tensor gives a float32 response)."""
    _require_2d(image, "corner_harris")
    if method not in ("k", "eps"):
        raise ValueError("method must be 'k' or 'eps', got {!r}".format(method))
    _, sigmas = _check_structure_args(2, sigma, "constant", "rc")
    block, shape = _structure_tensor_block(image, sigmas, "constant", 0, "rc")
    return _corner_response(block, shape, "harris_" + method, block.dtype, k, eps)[0]


def corner_shi_tomasi(image, sigma=1):
    """Shi-Tomasi (Kanade-Tomasi) corner response, 2-D (corner.py:674-743), exactly what the reference computes:
    (Arr + Acc) - sqrt((Arr - Acc)^2 + 4 * Arc * Arc) / 2, twice the smaller eigenvalue of the structure tensor."""
    _require_2d(image, "corner_shi_tomasi")
    _, sigmas = _check_structure_args(2, sigma, "constant", "rc")
    block, shape = _structure_tensor_block(image, sigmas, "constant", 0, "rc")
    return _corner_response(block, shape, "shi_tomasi", block.dtype)[0]


def corner_foerstner(image, sigma=1):
    """Foerstner corner measures (w, q), 2-D (corner.py:746-830): w = det(A) / trace(A), q = 4 * det(A) / trace(A)^2 where the
    trace is not 0, else 0; the quotients are formed in the tensor's dtype and stored as float64, as in the reference."""
    _require_2d(image, "corner_foerstner")
    _, sigmas = _check_structure_args(2, sigma, "constant", "rc")
    block, shape = _structure_tensor_block(image, sigmas, "constant", 0, "rc")
    w, q = _corner_response(block, shape, "foerstner", np.float64)
    return w, q


def corner_kitchen_rosenfeld(image, mode="constant", cval=0):
    """Kitchen-Rosenfeld corner response, 2-D (corner.py:533-590): (imxx * imy^2 + imyy * imx^2 - 2 * imxy * imx * imy) /
    (imx^2 + imy^2) where the denominator is not 0, else 0, float64; imx, imy the Sobel derivatives of the image along the
    two axes and imxx, imxy, imyy theirs.  Three derivative launches (image, imx, imy) and one response launch.

    Deviation: the reference feeds integer images unconverted into ndi.sobel here, where they wrap; this function converts
    the image like the other detectors do (integers scaled to float64, float16 computed in float32)."""
    _require_2d(image, "corner_kitchen_rosenfeld")
    S.check_mode(mode)
    cval = float(cval)
    image = core.ascontiguousarray(_as_float_device(image))
    block = _row_block(6, image.size, image.dtype)
    if image.size:
        _sobel_block(image, False, False, mode, cval, out=block[0:2])
        _sobel_block(block[0].reshape(image.shape), False, False, mode, cval, out=block[2:4])
        _sobel_block(block[1].reshape(image.shape), False, False, mode, cval, out=block[4:6])
    return _corner_response(block, image.shape, "kitchen_rosenfeld", np.float64)[0]


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


# ------------------------------------------------------------------ peak_local_max, corner_peaks (peak.py, corner.py:833-953)
_peak_launches = 0
_P_NORMS = {np.inf: 0, 1: 1, 2: 2}
_SPACING_FIRST_BATCH = 4          # rounds queued before the first look at the "still live" flag


def last_peak_launches():
    """Kernel launches of csrc/select.hip the last `peak_local_max`, `corner_peaks` or `_ensure_spacing` call of this process
    queued (no-op spacing rounds included; the maximum filter and the reductions of the threshold are not counted): a
    diagnostic for benchmarks and tests."""
    return _peak_launches


def _select_launches():
    fn = S.lib().mi_debug_select_launches
    fn.argtypes = []
    fn.restype = ctypes.c_int
    return fn()


def _counts_launches(func):
    """the outermost decorated call records the launches it queued"""
    @functools.wraps(func)
    def counted(*args, **kwargs):
        global _peak_launches
        if counted.depth:
            return func(*args, **kwargs)
        counted.depth += 1
        try:
            before = _select_launches()
            try:
                return func(*args, **kwargs)
            finally:
                _peak_launches = _select_launches() - before
        finally:
            counted.depth -= 1
    counted.depth = 0
    return counted


def _removed_arg(name, version):
    """FutureWarning when the deprecated argument `name` is passed at all (remove_arg of _shared/utils.py)"""
    def wrap(func):
        position = list(inspect.signature(func).parameters).index(name)

        @functools.wraps(func)
        def checked(*args, **kwargs):
            if len(args) > position or name in kwargs:
                warnings.warn("{0} argument is deprecated and will be removed in version {1}. To avoid this warning, please do not use "
                              "the {0} argument. Please see {2} documentation for more details.".format(name, version, func.__name__),
                              FutureWarning, stacklevel=2)
            return func(*args, **kwargs)
        return checked
    return wrap


def _p_norm_code(p_norm):
    try:
        return _P_NORMS[float(p_norm)]
    except (KeyError, TypeError, ValueError):
        raise ValueError("p_norm must be 1, 2 or inf on the device (exact integer distances), got {!r}".format(p_norm))


def _integral_distance(value, name):
    if isinstance(value, (bool, np.bool_)) or not np.isscalar(value) or not np.isfinite(value) or int(value) != value:
        raise ValueError("{} must be an integer on the device (exact integer distances), got {!r}".format(name, value))
    return int(value)


def _get_excluded_border_width(ndim, min_distance, exclude_border):
    """border widths per axis, every error of peak.py:87-117"""
    if isinstance(exclude_border, bool):
        return (min_distance if exclude_border else 0,) * ndim
    if isinstance(exclude_border, int):
        if exclude_border < 0:
            raise ValueError("`exclude_border` cannot be a negative value")
        return (exclude_border,) * ndim
    if isinstance(exclude_border, tuple):
        if len(exclude_border) != ndim:
            raise ValueError("`exclude_border` should have the same length as the dimensionality of the image.")
        for exclude in exclude_border:
            if not isinstance(exclude, int):
                raise ValueError("`exclude_border`, when expressed as a tuple, must only contain ints.")
            if exclude < 0:
                raise ValueError("`exclude_border` can not be a negative value")
        return exclude_border
    raise TypeError("`exclude_border` must be bool, int, or tuple with the same length as the dimensionality of the image.")


def _check_peak_image(image):
    """(ndim, dtype) of an image the peak functions take, before anything touches the device"""
    if not isinstance(image, (core.ndarray, np.ndarray)):
        image = np.asarray(image)
    dtype = np.dtype(image.dtype)
    if dtype == np.bool_ or dtype.kind not in "iuf":
        raise TypeError("peak_local_max takes images of a real dtype, not {}".format(dtype))
    if image.ndim < 1 or image.ndim > _lib.MI_MAX_NDIM:
        raise ValueError("arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    return image.ndim, dtype


def _get_threshold(image, threshold_abs, threshold_rel):
    """peak.py:74-84 with the image's minimum and maximum from the device reductions"""
    lo, hi = S.min_max(image) if (threshold_abs is None or threshold_rel is not None) else (0.0, 0.0)
    threshold = threshold_abs if threshold_abs is not None else lo
    if threshold_rel is not None:
        threshold = max(threshold, threshold_rel * float(hi))
    return float(threshold)


def _peak_candidates(image, image_max, threshold, border):
    """(coords (K, ndim) int64 in raster order, values (K,)): the fused predicate through the count / write compaction; the
    mask never exists in memory.  A "trivial" image (every voxel equal to its filtered maximum) has no candidates."""
    lib = S.lib()
    nbytes = ctypes.c_int64()
    core._select_check(lib.mi_select_work_bytes(image.size, ctypes.byref(nbytes)))
    work = core.empty((nbytes.value,), np.uint8)
    total, equal = ctypes.c_int64(), ctypes.c_int64()
    bw = (ctypes.c_int64 * _lib.MI_MAX_NDIM)(*[int(b) for b in border])
    idesc, wdesc = image._desc(), work._desc()
    mdesc = image_max._desc() if image_max is not None else None
    mref = ctypes.byref(mdesc) if image_max is not None else None
    core._select_check(lib.mi_peak_count(ctypes.byref(idesc), mref, threshold, bw, ctypes.byref(wdesc), ctypes.byref(total),
                                         ctypes.byref(equal), None))
    k = total.value
    if image_max is not None and equal.value == image.size:
        k = 0
    coords, values = core.empty((k, image.ndim), np.int64), core.empty((k,), image.dtype)
    if k:
        cdesc, vdesc = coords._desc(), values._desc()
        core._select_check(lib.mi_peak_write(ctypes.byref(idesc), mref, threshold, bw, ctypes.byref(wdesc), ctypes.byref(cdesc),
                                             ctypes.byref(vdesc), None))
    return coords, values


@_counts_launches
def _ensure_spacing(coords, shape, spacing, p_norm=np.inf, inclusive=False):
    """The points of `coords` -- a (K, ndim) int64 device array of distinct points inside `shape`, in rank order -- that the
    greedy walk of ensure_spacing (_shared/coord.py) keeps: every point not yet rejected rejects the later points at a
    distance below `spacing` (`inclusive`: at or below it, the rule of corner_peaks, corner.py:929-945).  That is the
    lexicographically first maximal independent set of the conflict graph, computed in rounds on the device (keep the live
    points without a live conflicting point of lower rank, reject the live points in conflict with a kept one) with one
    4-byte read per batch of rounds, and compacted in order.  Distances are exact integers (max |d|, sum |d|, sum d^2 against
    spacing^2); p_norm other than 1, 2, inf and a non-integral spacing raise ValueError."""
    p = _p_norm_code(p_norm)
    spacing = _integral_distance(spacing, "spacing")
    shape = tuple(int(s) for s in shape)
    coords = core.ascontiguousarray(coords)
    if coords.dtype != np.int64 or coords.ndim != 2 or coords.shape[1] != len(shape):
        raise ValueError("coords must be a (K, {}) int64 array".format(len(shape)))
    k = coords.shape[0]
    if k == 0 or spacing < (0 if inclusive else 1) or (spacing == 0 and inclusive):
        return coords
    lib = S.lib()
    grid = core.empty(shape, np.int32)
    status = core.empty((k,), np.uint8)
    cdesc, gdesc, sdesc = coords._desc(), grid._desc(), status._desc()
    flag = ctypes.c_int()
    core._select_check(lib.mi_spacing_init(ctypes.byref(cdesc), ctypes.byref(gdesc), ctypes.byref(sdesc), ctypes.byref(flag), None))
    if flag.value:
        raise ValueError("coords holds points outside shape {}".format(shape))
    done, batch = 0, _SPACING_FIRST_BATCH
    while True:
        core._select_check(lib.mi_spacing_rounds(ctypes.byref(cdesc), ctypes.byref(gdesc), ctypes.byref(sdesc), spacing, p, int(inclusive),
                                                 batch, ctypes.byref(flag), None))
        done += batch
        if not flag.value:
            break
        if done >= k:           # every round with a live point keeps at least the live point of lowest rank
            raise RuntimeError("greedy spacing did not finish in {} rounds for {} points".format(done, k))
        batch = min(2 * batch, 64, k - done)
    keep = core.flatnonzero(status)
    return coords if keep.shape[0] == k else core._take_rows(coords, keep, coords.shape[1])


def _coords_to_mask(coords, shape):
    out = core.empty(shape, np.bool_)
    cdesc, odesc = coords._desc(), out._desc()
    core._select_check(S.lib().mi_scatter_true(ctypes.byref(cdesc), ctypes.byref(odesc), None))
    return out


def _limit(coords, num_peaks):
    if num_peaks is None or num_peaks == np.inf or coords.shape[0] <= num_peaks:
        return coords
    return coords[:max(int(num_peaks), 0)]


@_counts_launches
def _peak_local_max(image, min_distance, threshold_abs, threshold_rel, exclude_border, num_peaks, footprint, labels, p_norm):
    """(coords, shape); every check before the first device call"""
    if labels is not None:
        raise NotImplementedError("labels= needs a device find_objects, which this library does not have yet")
    ndim, dtype = _check_peak_image(image)
    if footprint is not None:
        footprint = core.host_copy(footprint) if isinstance(footprint, core.ndarray) else np.asarray(footprint)
    if (footprint is None or footprint.size == 1) and min_distance < 1:
        warnings.warn("When min_distance < 1, peak_local_max acts as finding image > max(threshold_abs, threshold_rel * max(image)).",
                      RuntimeWarning, stacklevel=4)
    border = _get_excluded_border_width(ndim, min_distance, exclude_border)
    _p_norm_code(p_norm)
    min_distance = _integral_distance(min_distance, "min_distance")
    border = tuple(max(int(b), 0) for b in border)
    if not isinstance(image, core.ndarray):
        image = core.asarray(np.asarray(image))
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    image = core.ascontiguousarray(image)
    if image.size == 0:
        return core.empty((0, ndim), np.int64), image.shape
    threshold = _get_threshold(image, threshold_abs, threshold_rel)
    image_max = None
    if (footprint is None and min_distance >= 1 or footprint is not None and footprint.size != 1) and image.size != 1:
        if footprint is None:
            image_max = ndi.maximum_filter(image, size=2 * min_distance + 1, mode="constant")
        else:
            image_max = ndi.maximum_filter(image, footprint=footprint.astype(bool), mode="constant")
        image_max = core.ascontiguousarray(image_max)
    coords, values = _peak_candidates(image, image_max, threshold, border)
    if coords.shape[0] > 1:
        order = core.argsort(values, descending=True)         # highest first, ties in raster order
        coords = core._take_rows(coords, order, ndim)
    coords = _ensure_spacing(coords, image.shape, min_distance, p_norm)
    return _limit(coords, num_peaks), image.shape


@_removed_arg("indices", "0.20")
def peak_local_max(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, indices=True, num_peaks=np.inf,
                   footprint=None, labels=None, num_peaks_per_label=np.inf, p_norm=np.inf):
    """Peaks of an image as a (K, ndim) int64 device array of coordinates, highest first (peak.py:120-345): the voxels equal
    to the maximum over their (2 * min_distance + 1)-wide neighbourhood (or `footprint`), above the threshold
    (`threshold_abs`, default the image's minimum, raised to `threshold_rel * max(image)`), outside the excluded border
    (`exclude_border`: True = min_distance, an int, or one int per axis), thinned so that no two are closer than
    `min_distance` in the `p_norm` metric, and cut to `num_peaks`.  With `indices=False` (deprecated, FutureWarning) a bool
    array of the image's shape.  No peaks: a (0, ndim) array.  The image is not written.

    Order contract: the candidates are sorted by `-value` with a stable sort, so peaks of equal value come in raster order
    (the reference leaves the order of ties to cupy.argsort); the greedy thinning walks them in that order.

    Everything runs on the device: the maximum filter, one fused predicate through a count / scan / scatter compaction (the
    mask never exists in memory; one read sizes the result and tells whether the image is trivial), a stable radix sort, the
    greedy thinning in rounds (`_ensure_spacing`), `[:num_peaks]`.  Peak memory: the image, its filtered maximum, the int32
    map of the image's shape and two (key, index) pair buffers of the candidates.

    Deviations: `labels=` raises NotImplementedError (the reference loops over find_objects regions on the host and writes
    into the caller's image); `_prominent_peaks` is not provided (it needs regionprops); `p_norm` must be 1, 2 or inf and
    `min_distance` an integer (ValueError otherwise: distances are exact integers); float16 images are computed in float32;
    a NaN never is a peak and is skipped by the threshold's minimum and maximum; a negative `min_distance` excludes no
    border; an empty result is (0, ndim), not (0, 2)."""
    coords, shape = _peak_local_max(image, min_distance, threshold_abs, threshold_rel, exclude_border, num_peaks, footprint, labels, p_norm)
    return coords if indices else _coords_to_mask(coords, shape)


@_counts_launches
def corner_peaks(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, indices=True, num_peaks=np.inf,
                 footprint=None, labels=None, *, num_peaks_per_label=np.inf, p_norm=np.inf):
    """Peaks of a corner response (corner.py:833-953): `peak_local_max` with num_peaks=inf and the Chebyshev metric, then a
    second greedy pass in which every peak not yet rejected rejects the later peaks at a distance of `min_distance` or less
    in the `p_norm` metric (so connected peaks of one value collapse to the first in raster order), then `[:num_peaks]`.
    Returns a (K, ndim) int64 device array, or a bool array with `indices=False`.

    Order contract: that of `peak_local_max` (highest first, peaks of equal value in raster order); both greedy passes walk
    the peaks in that order.

    Deviations: those of `peak_local_max` (`labels=` raises NotImplementedError, `p_norm` must be 1, 2 or inf and
    `min_distance` an integer, an empty result is (0, ndim))."""
    _p_norm_code(p_norm)
    coords, shape = _peak_local_max(image, min_distance, threshold_abs, threshold_rel, exclude_border, np.inf, footprint, labels, np.inf)
    coords = _ensure_spacing(coords, shape, min_distance, p_norm, inclusive=True)
    coords = _limit(coords, None if num_peaks is None or np.isinf(num_peaks) else num_peaks)
    return coords if indices else _coords_to_mask(coords, shape)
