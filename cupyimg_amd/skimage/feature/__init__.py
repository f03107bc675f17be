"""skimage.feature subset: the Hessian matrix and its eigenvalues (cupyimg/skimage/feature/corner.py:141-211, 260-458) on
HIP kernels (csrc/ridges.hip)."""
import ctypes

import numpy as np

from ... import core, _lib
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ..filters import _img_as_float

__all__ = ["hessian_matrix", "hessian_matrix_eigvals", "structure_tensor_eigenvalues"]


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
