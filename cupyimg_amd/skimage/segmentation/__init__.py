"""skimage.segmentation subset: morphological snakes (cupyimg/skimage/segmentation/morphsnakes.py) as fused HIP kernels
(csrc/morphsnakes.hip): one main launch per iteration, no host round trip inside the loop."""
import ctypes
import functools
import math
import warnings

import numpy as np

from ... import core
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S

__all__ = [
    "morphological_chan_vese",
    "morphological_geodesic_active_contour",
    "inverse_gaussian_gradient",
    "circle_level_set",
    "disk_level_set",
    "checkerboard_level_set",
]
# find_boundaries, mark_boundaries, relabel_sequential and join_segmentations are imported at the end of this file from
# _boundaries.py and _join.py, whose `__all__` list them: tests/test_morphsnakes_host.py pins this list to the snakes.

_STATE_BYTES = 64                                   # MI_SNAKE_STATE_BYTES
_WORK_BYTES = _STATE_BYTES + 32 * 65536             # MI_SNAKE_WORK_BYTES
_MAX_SMOOTHING = 64
_snake_launches = None


def last_snake_launches():
    """Kernel launches the evolution of the most recent `morphological_chan_vese` / `morphological_geodesic_active_contour`
    call of this process queued (the loop, the first sums of MorphACWE and the order statistics of threshold="auto"; not the
    conversion of the inputs): a function of `iterations`, `smoothing` and the settings alone, never of the data.  None
    before the first call.  A diagnostic for benchmarks and tests."""
    return _snake_launches


def _launch_counter():
    fn = S.lib().mi_debug_morphsnakes_launches
    fn.argtypes = []
    fn.restype = ctypes.c_int
    return fn


def _check_rank(ndim, name="image"):
    if ndim not in (2, 3):
        raise ValueError("The parameter `{}` must be a 2-or-3-dimensional array".format(name))


def _host_or_device(a):
    """a device array as it is, anything else through np.asarray (complex: TypeError)"""
    if isinstance(a, core.ndarray):
        return a
    if not isinstance(a, np.ndarray) and hasattr(a, "__cuda_array_interface__"):
        return core.asarray(a)
    host = np.asarray(a)
    if host.dtype.kind == "c":
        raise TypeError("Complex type not supported")
    return host


def _binarize(a, nonzero=False):
    """a new C-contiguous int8 device array: a > 0 (a != 0 with `nonzero`)"""
    a = core.ascontiguousarray(core.asarray(a))
    if a.dtype == np.float16:
        a = a.astype(np.float32)
    out = core.empty(a.shape, np.int8)
    if a.size:
        ad, od = a._desc(), out._desc()
        S.check(S.lib().mi_snake_binarize(ctypes.byref(ad), ctypes.byref(od), int(nonzero), None))
    return out


def _float_image(image):
    """C-contiguous float32 / float64 device array: float32 and float64 as they are, float16 as float32, bool and integers as
    float64 (exact)"""
    image = core.asarray(image)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    elif image.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        image = image.astype(np.float64)
    return core.ascontiguousarray(image)


def _curvature(u, ops):
    """ops: a sequence of "SI" / "IS", applied left to right, on an int8 0 / 1 device array -> new int8 array"""
    out = core.empty(u.shape, np.int8)
    if u.size == 0:
        return out
    tmp = core.empty(u.shape, np.int8)
    bits = 0
    for i, op in enumerate(ops):
        bits |= (op == "SI") << i
    ud, od, td = u._desc(), out._desc(), tmp._desc()
    S.check(S.lib().mi_snake_curvature(ctypes.byref(ud), ctypes.byref(od), ctypes.byref(td), len(ops), bits, None))
    return out


def sup_inf(u):
    """SI operator (morphsnakes.py:55-72): the maximum over the 4 lines (2-D) / 9 planes (3-D) through a voxel of the binary
    erosion of `u != 0` by that element, border value 0.  One launch; int8 result."""
    u = _host_or_device(u)
    if u.ndim not in (2, 3):
        raise ValueError("u has an invalid number of dimensions (should be 2 or 3)")
    return _curvature(_binarize(u, nonzero=True), ["SI"])


def inf_sup(u):
    """IS operator (morphsnakes.py:75-92): the minimum over the same elements of the binary dilation.  One launch; int8 result."""
    u = _host_or_device(u)
    if u.ndim not in (2, 3):
        raise ValueError("u has an invalid number of dimensions (should be 2 or 3)")
    return _curvature(_binarize(u, nonzero=True), ["IS"])


def _check_input(image, init_level_set):
    """Check that shapes of `image` and `init_level_set` match."""
    _check_rank(image.ndim)
    if len(image.shape) != len(init_level_set.shape):
        raise ValueError("The dimensions of the initial level set do not match the dimensions of the image.")
    if tuple(image.shape) != tuple(init_level_set.shape):
        raise ValueError("The shape of the initial level set {} does not match the shape of the image {}.".format(
            tuple(init_level_set.shape), tuple(image.shape)))


def _init_level_set(init_level_set, image_shape):
    """A level set from its name, on the host (uploaded with the others); anything else through `_host_or_device`."""
    if isinstance(init_level_set, str):
        if init_level_set == "checkerboard":
            res = _checkerboard(image_shape, 5)
        # TODO: remove me in 0.19.0
        elif init_level_set == "circle":
            _circle_warning(4)
            res = _disk(image_shape, None, None)
        elif init_level_set == "disk":
            res = _disk(image_shape, None, None)
        else:
            raise ValueError("`init_level_set` not in ['checkerboard', 'circle', 'disk']")
    else:
        res = _host_or_device(init_level_set)
    return res


def _circle_warning(stacklevel):
    warnings.warn("circle_level_set is deprecated in favor of disk_level_set."
                  "circle_level_set will be removed in version 0.19", FutureWarning, stacklevel=stacklevel)


def _disk(image_shape, center, radius):
    """The reference's arithmetic (morphsnakes.py:191-200) on open grids: one squared distance per axis, added in axis order
    by broadcasting, so a 256^3 level set costs one volume on the host instead of the reference's rank + 2."""
    image_shape = tuple(int(i) for i in image_shape)
    if center is None:
        center = tuple(i // 2 for i in image_shape)
    if radius is None:
        radius = min(image_shape) * 3.0 / 8.0
    center = np.asarray(center)
    if center.shape != (len(image_shape),):
        raise ValueError("center must have one coordinate per axis")
    total = None
    for g, c in zip(np.ogrid[tuple(slice(i) for i in image_shape)], center):
        sq = (g - c) ** 2
        total = sq if total is None else total + sq
    phi = radius - np.sqrt(total)
    return (phi > 0).astype(np.int8)


def _checkerboard(image_shape, square_size):
    image_shape = tuple(int(i) for i in image_shape)
    grids = [(g // square_size) & 1 for g in np.ogrid[tuple(slice(i) for i in image_shape)]]
    return np.ascontiguousarray(np.broadcast_to(functools.reduce(np.bitwise_xor, grids), image_shape)).astype(np.int8)


def circle_level_set(image_shape, center=None, radius=None):
    """Create a circle level set with binary values (deprecated name of `disk_level_set`, morphsnakes.py:133-164)."""
    _circle_warning(3)
    return core.asarray(_disk(image_shape, center, radius))


def disk_level_set(image_shape, center=None, radius=None):
    """Create a disk level set with binary values (morphsnakes.py:167-201): 1 where the distance to `center` (default: the
    middle of the image) is below `radius` (default: 3 / 8 of the smallest extent).  Built on the host and uploaded; int8."""
    return core.asarray(_disk(image_shape, center, radius))


def checkerboard_level_set(image_shape, square_size=5):
    """Create a checkerboard level set with binary values (morphsnakes.py:204-234), squares of `square_size` voxels.  Built
    on the host and uploaded; int8."""
    return core.asarray(_checkerboard(image_shape, square_size))


def inverse_gaussian_gradient(image, alpha=100.0, sigma=5.0):
    """Inverse of gradient magnitude (morphsnakes.py:237-266): `1 / sqrt(1 + alpha * g)` with
    `g = ndi.gaussian_gradient_magnitude(image, sigma, mode="nearest")`, on the device.  Flat areas come out close to 1,
    areas near borders close to 0: the usual preprocessing for `morphological_geodesic_active_contour`.  float32 stays
    float32, float16 is computed and returned as float32, everything else is float64."""
    image = _host_or_device(image)
    gradnorm = _float_image(ndi.gaussian_gradient_magnitude(core.asarray(image), sigma, mode="nearest"))
    out = core.empty(gradnorm.shape, gradnorm.dtype)
    if gradnorm.size:
        gd, od = gradnorm._desc(), out._desc()
        S.check(S.lib().mi_snake_inverse_gradient(ctypes.byref(gd), ctypes.byref(od), float(alpha), None))
    return out


def _prepare(image, iterations, init_level_set, smoothing):
    """Every argument check, on the host, before the device is touched -> (image, level set) still where they were"""
    image = _host_or_device(image)
    if image.dtype.kind == "c":
        raise TypeError("Complex type not supported")
    _check_rank(image.ndim)
    iterations, smoothing = int(iterations), int(smoothing)
    if iterations < 0:
        raise ValueError("iterations must not be negative")
    if smoothing < 0 or smoothing > _MAX_SMOOTHING:
        raise ValueError("smoothing must be 0 to {}".format(_MAX_SMOOTHING))
    init_level_set = _init_level_set(init_level_set, image.shape)
    _check_input(image, init_level_set)
    if iterations > 0 and image.size and min(image.shape) < 2:
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least 2 elements are required "
                         "along every axis.")
    return image, init_level_set, iterations, smoothing


def _evolve(u, iterations, step, callback):
    """The loop: step(i, u_in, u_out, u_tmp) queues iteration i.  `callback` (None: the default no-op) gets a copy of its
    own, because the buffers are reused two iterations later."""
    if callback is not None:
        callback(u.copy())
    if iterations:
        other, tmp = core.empty(u.shape, np.int8), core.empty(u.shape, np.int8)
        for i in range(iterations):
            step(i, u, other, tmp)
            u, other = other, u
            if callback is not None:
                callback(u.copy())
    return u


def morphological_chan_vese(image, iterations, init_level_set="checkerboard", smoothing=1, lambda1=1, lambda2=1,
                            iter_callback=lambda x: None):
    """Morphological Active Contours without Edges (MorphACWE, morphsnakes.py:269-378).

    Segments objects without well defined borders whose inside differs on average from their outside.  `image`: a 2-D or
    3-D array; `iterations`: how many to run; `init_level_set`: "checkerboard", "disk", "circle" (deprecated) or an array of
    the image's shape, binarised with `> 0`; `smoothing`: applications of the curvature operator per iteration; `lambda1`,
    `lambda2`: weights of the outer and inner region (Python numbers); `iter_callback`: called with the level set before
    the loop and after every iteration.  Returns the final level set, a new int8 device array.

    One iteration is one launch that keeps the level set of a box in LDS, updates it from the two region means and applies
    up to 2 smoothing steps (further ones: one launch per 2), plus a one-workgroup launch that turns the launch's partial
    sums into the means of the next iteration; the host reads nothing inside the loop.  The arithmetic is the reference's,
    in the image dtype: float32 and float64 keep theirs, bool and integers are computed in float64, float16 in float32.
    Deviations: the masked sums behind the means are accumulated in double in a fixed order (the reference: in the image
    dtype, in its reduction's order), which can change a voxel only where `lambda1 (I - c1)^2 - lambda2 (I - c0)^2` is within
    summation error of 0; every call starts its alternation of the smoothing operator with SI o IS (the reference keeps one
    cycle per process, so there it depends on every earlier call); a level set of another shape, an axis shorter than 2
    with iterations > 0, negative `iterations` or `smoothing` raise ValueError and complex images TypeError.  A callback
    other than the default receives a copy the library never writes again; with the default nothing is copied."""
    global _snake_launches
    image, init_level_set, iterations, smoothing = _prepare(image, iterations, init_level_set, smoothing)
    callback = None if iter_callback is _DEFAULT_CALLBACKS[0] else iter_callback
    if image.size == 0:
        _snake_launches = 0
        return core.empty(image.shape, np.int8)
    u = _binarize(init_level_set)
    if iterations == 0:
        _snake_launches = 0
        if callback is not None:
            callback(u.copy())
        return u
    img = _float_image(image)
    lib = S.lib()
    count = _launch_counter()
    before = count()
    work = core.empty((_WORK_BYTES,), np.uint8)
    wptr = ctypes.c_void_p(work.ptr)
    idesc = img._desc()
    ud = u._desc()
    S.check(lib.mi_snake_acwe_init(ctypes.byref(idesc), ctypes.byref(ud), wptr, None))
    lam1, lam2 = float(lambda1), float(lambda2)

    def step(i, u_in, u_out, u_tmp):
        a, b, c = u_in._desc(), u_out._desc(), u_tmp._desc()
        S.check(lib.mi_snake_acwe_step(ctypes.byref(idesc), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), lam1, lam2,
                                       smoothing, (i * smoothing) & 1, wptr, None))

    u = _evolve(u, iterations, step, callback)
    _snake_launches = count() - before
    return u


def _percentile_40(img, work):
    """numpy.percentile(img, 40) in float64 (linear interpolation): the two order statistics are selected on the device and
    read once."""
    n = img.size
    virtual = (n - 1) * 0.4
    previous = math.floor(virtual)
    gamma = virtual - previous
    k0 = int(previous)
    k1 = min(k0 + 1, n - 1)
    idesc = img._desc()
    S.check(S.lib().mi_snake_order_stats(ctypes.byref(idesc), k0, k1, ctypes.c_void_p(work.ptr), None))
    a, b = (float(v) for v in work[48:64].get().view(np.float64))
    diff = b - a
    return b - diff * (1 - gamma) if gamma >= 0.5 else a + diff * gamma


def morphological_geodesic_active_contour(gimage, iterations, init_level_set="circle", smoothing=1, threshold="auto", balloon=0,
                                          iter_callback=lambda x: None):
    """Morphological Geodesic Active Contours (MorphGAC, morphsnakes.py:381-510).

    Segments objects with visible but noisy, cluttered or broken borders.  `gimage`: the preprocessed 2-D or 3-D image
    (see `inverse_gaussian_gradient`); the contour stops where it is small.  `iterations`, `init_level_set`, `smoothing`,
    `iter_callback`: as for `morphological_chan_vese`.  `threshold`: areas below it count as borders, "auto" is the 40th
    percentile of the image; `balloon`: positive values expand the contour where `gimage > threshold / |balloon|`,
    negative ones shrink it there, 0 turns the force off.  Returns the final level set, a new int8 device array.

    One iteration is one launch: the balloon (a 3^ndim binary dilation or erosion, border value 0), the attachment step
    `sum_axis gradient(gimage) * gradient(u)` with the image gradient formed in the kernel, and up to 2 smoothing steps
    (further ones: one launch per 2).  The arithmetic is the reference's in the image dtype (bool and integers: float64,
    float16: float32).  Deviations: the balloon mask compares `double(gimage) > double(threshold) / |balloon|` (the
    reference compares in float32 when a float32 image meets a Python float); threshold="auto" is interpolated in float64
    between two order statistics found by a radix select on the device, read once per call, and is only computed when
    `balloon` is not 0, its only use; the alternation of the smoothing operator and the errors are as described for
    `morphological_chan_vese`."""
    global _snake_launches
    image, init_level_set, iterations, smoothing = _prepare(gimage, iterations, init_level_set, smoothing)
    callback = None if iter_callback is _DEFAULT_CALLBACKS[1] else iter_callback
    auto = isinstance(threshold, str)
    if auto and threshold != "auto":
        raise ValueError("threshold must be a number or 'auto'")
    balloon = float(balloon)
    if image.size == 0:
        _snake_launches = 0
        return core.empty(image.shape, np.int8)
    u = _binarize(init_level_set)
    if iterations == 0:
        _snake_launches = 0
        if callback is not None:
            callback(u.copy())
        return u
    img = _float_image(image)
    lib = S.lib()
    count = _launch_counter()
    before = count()
    mask_threshold = 0.0
    if balloon != 0:
        if auto:
            threshold = _percentile_40(img, core.empty((_WORK_BYTES,), np.uint8))
        elif isinstance(threshold, core.ndarray):
            threshold = float(threshold.get().reshape(-1)[0])
        mask_threshold = float(threshold) / abs(balloon)
    sign = (balloon > 0) - (balloon < 0)
    idesc = img._desc()

    def step(i, u_in, u_out, u_tmp):
        a, b, c = u_in._desc(), u_out._desc(), u_tmp._desc()
        S.check(lib.mi_snake_gac_step(ctypes.byref(idesc), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), mask_threshold, sign,
                                      smoothing, (i * smoothing) & 1, None))

    u = _evolve(u, iterations, step, callback)
    _snake_launches = count() - before
    return u


# the default no-op callbacks, recognised by identity: nothing is copied for them
_DEFAULT_CALLBACKS = (morphological_chan_vese.__defaults__[-1], morphological_geodesic_active_contour.__defaults__[-1])

from ._boundaries import find_boundaries, last_boundary_launches, mark_boundaries  # noqa: E402,F401
from ._join import join_segmentations, relabel_sequential  # noqa: E402,F401
