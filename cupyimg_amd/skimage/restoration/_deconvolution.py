"""skimage.restoration.richardson_lucy (cupyimg/skimage/restoration/deconvolution.py:356-416) as fused HIP kernels
(csrc/richardson_lucy.hip): one C-ABI call per iteration, nothing read back inside the loop."""
import ctypes
import math

import numpy as np

from ... import core, _lib
from ...scipy.ndimage import _support as S

__all__ = ["richardson_lucy"]

_MAX_VOXELS = 2 ** 31


def _shape_dtype(a):
    """(array, shape, dtype) of a device array or anything array-like on the host, without touching the device"""
    if isinstance(a, core.ndarray):
        return a, tuple(a.shape), np.dtype(a.dtype)
    a = np.asarray(a)
    return a, a.shape, a.dtype


def _float_type(image_dtype):
    """the dtype T the loop runs in: promote_types(image.dtype, float32), the reference's rule (no img_as_float)"""
    return np.promote_types(image_dtype, np.float32)


def _plan(image_shape, image_dtype, psf_shape, psf_dtype, iterations):
    """Every check of richardson_lucy's arguments, on shapes and dtypes alone -> (T, number of iterations to queue)."""
    for name, dtype in (("image", image_dtype), ("psf", psf_dtype)):
        if dtype.kind == "c":
            raise TypeError("Complex type not supported")
        if dtype.kind not in "biuf":
            raise TypeError("richardson_lucy takes arrays of a real dtype, not {} ({})".format(dtype, name))
    if len(image_shape) == 0:
        raise ValueError("richardson_lucy takes arrays of rank 1 to {}, not rank 0".format(_lib.MI_MAX_NDIM))
    if len(image_shape) > _lib.MI_MAX_NDIM:
        raise ValueError("richardson_lucy takes arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    if len(psf_shape) != len(image_shape):
        raise ValueError("psf must have the image's number of dimensions ({}), got {}".format(len(image_shape), len(psf_shape)))
    if math.prod(psf_shape) == 0:
        raise ValueError("The parameter `psf` cannot have an empty axis; got shape {}".format(tuple(psf_shape)))
    if math.prod(image_shape) >= _MAX_VOXELS:
        raise ValueError("richardson_lucy: images of 2**31 voxels or more are not supported; got shape {}".format(tuple(image_shape)))
    return _float_type(image_dtype), max(0, int(iterations))


def richardson_lucy(image, psf, iterations=50, clip=True, filter_epsilon=None):
    """Richardson-Lucy deconvolution (deconvolution.py:356-416) of an image of rank 1 to MI_MAX_NDIM with the point spread
    function `psf` of the same rank, as a new C-contiguous device array.  `iterations` plays the role of regularisation
    (`iterations <= 0` returns the starting estimate, 0.5 everywhere, as `range()` does in the reference); with `clip` results
    above 1 or below -1 are set to 1 and -1; where the blurred estimate is below `filter_epsilon` (if truthy) the intermediate
    ratio becomes 0.  `image` and `psf` are device arrays or anything array-like on the host; a strided view is compacted first.

    One C-ABI call per iteration (mi_richardson_lucy_step, csrc/richardson_lucy.hip), two estimates ping-ponging, nothing read
    back inside the loop.  Ranks 2 and 3 take one launch per iteration of a fused kernel that streams along axis 0 with the
    estimate and the ratio in LDS rings, so the ratio never exists in memory; other ranks and PSFs whose rings do not fit LDS
    take two launches (one thread per voxel) with the ratio in a scratch volume.  Both give the same bits.

    The contract is the reference's loop with this library's `scipy.signal.convolve(..., mode="same")` as the convolution,
    evaluated step by step in T = promote_types(image.dtype, float32): float16, bool and 8/16-bit integers run in float32,
    float32 stays, 32/64-bit integers and float64 run in float64; values are taken as they are (no img_as_float).

        image = image.astype(T);  psf = psf.astype(T);  u = full(image.shape, T(0.5))
        repeat `iterations` times:
            c = convolve(u, psf, "same")              # c[i] = sum_k psf[k] * u[i + (s-1)//2 - k], zero outside the image
            r = image / c                             # one division in T
            if filter_epsilon: r = where(c < T(filter_epsilon), T(0), r)
            u = u * convolve(r, mirror(psf), "same")  # u[i] * sum_j psf[j] * r[i - s//2 + j], zero outside the image
        if clip: u[u > 1] = 1;  u[u < -1] = -1

    Every convolution follows `ndimage.correlate(dtype_mode="numpy")`: the non-zero taps in C order (of the reversed PSF for the
    first sum, of the PSF for the second), every product formed and added in float64 from +0.0, an outside sample a 0 multiplied
    and added like any other, the sum rounded once to T.  NaN, infinities and a zero `c` propagate as IEEE arithmetic dictates.

    Deviations: `mirror(psf)` reverses every axis, as scikit-image does since 0.18 (the reference's `psf[::-1, ::-1]` reverses
    the first two only: the same for rank 2, wrong for rank 3 and above, an IndexError for rank 1); the sums are accumulated in
    float64 for float32 data too (the reference accumulates in T, or goes through an FFT); `clip` is folded into the last
    iteration's store; a complex image or PSF raises TypeError, a PSF of another rank than the image's, a PSF with an empty axis
    and rank 0 raise ValueError, all before anything is uploaded; an empty image returns an empty array; images of 2**31 voxels
    or more raise ValueError.

    Besides the converted image a call holds two volumes of T, plus one more on the two-launch route, all from the pool."""
    image, ishape, idtype = _shape_dtype(image)
    psf, pshape, pdtype = _shape_dtype(psf)
    T, n_iter = _plan(ishape, idtype, pshape, pdtype, iterations)
    if math.prod(ishape) == 0:
        return core.empty(ishape, T)

    phost = core.host_copy(psf) if isinstance(psf, core.ndarray) else psf
    phost = np.ascontiguousarray(np.asarray(phost).astype(T), dtype=np.float64)      # rounded to T, handed over as doubles
    if not isinstance(image, core.ndarray):
        image = core.asarray(image)
    if image.dtype != T:
        image = image.astype(T)
    image = core.ascontiguousarray(image)

    u = [core.full(ishape, 0.5, T), None]
    if n_iter == 0:
        return u[0]
    u[1] = core.empty(ishape, T)
    lib = S.lib()
    idesc = image._desc()
    udesc = [u[0]._desc(), u[1]._desc()]
    pshape_c = (ctypes.c_int64 * len(pshape))(*pshape)
    pptr = phost.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    needs = ctypes.c_int(0)
    S.check(lib.mi_richardson_lucy_needs_scratch(ctypes.byref(idesc), pshape_c, ctypes.byref(needs)), ValueError)
    scratch = core.empty(ishape, T) if needs.value else None
    sptr = ctypes.c_void_p(scratch.ptr) if scratch is not None else None
    use_eps = bool(filter_epsilon)
    eps = float(filter_epsilon) if use_eps else 0.0
    for i in range(n_iter):
        S.check(lib.mi_richardson_lucy_step(ctypes.byref(idesc), ctypes.byref(udesc[i & 1]), ctypes.byref(udesc[(i + 1) & 1]), pptr, pshape_c,
                                            eps, int(use_eps), int(bool(clip) and i == n_iter - 1), sptr, None), ValueError)
    return u[n_iter & 1]
