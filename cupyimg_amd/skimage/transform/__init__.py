"""skimage.transform subset: warp on top of ndimage.map_coordinates
(cupyimg/skimage/transform/_warps.py:790-1028; mode translation :163-169,
`warp_coords` :640-742, output clipping :745-787), resize on top of
ndimage.affine_transform (:30-248) and the two pyramid steps (pyramids.py:27-165).

`inverse_map` may be a coordinate array of shape (ndim, *output_shape), a 3x3
homogeneous matrix acting on (x, y) column/row coordinates, or a callable
mapping (N, 2) output (x, y) pairs to input (x, y) pairs.  Spline orders 0-5
(prefilter for orders > 1; the default for non-bool images is 1, as in the reference)."""
import math
import warnings

import numpy as np

from ... import core
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ..filters import convert_to_float

__all__ = ["warp", "warp_coords", "resize", "pyramid_reduce", "pyramid_expand"]

_NDI_MODE = {"constant": "constant", "edge": "nearest", "symmetric": "reflect", "reflect": "mirror",
             "wrap": "wrap"}


def _to_ndimage_mode(mode):
    """numpy.pad names -> ndimage names (_warps.py:163-169, _geometric.py:14-21)."""
    if mode not in _NDI_MODE:
        raise ValueError("Unknown mode: '{}', or cannot translate mode. The mode should be one of "
                         "'constant', 'edge', 'symmetric', 'reflect', or 'wrap'.".format(mode))
    return _NDI_MODE[mode]


def _validate_interpolation_order(image_dtype, order):
    """_shared/utils.py:425-464"""
    if order is None:
        return 0 if image_dtype == np.bool_ else 1
    if order < 0 or order > 5:
        raise ValueError("Spline interpolation order has to be in the range 0-5.")
    return order


def warp_coords(coord_map, shape, dtype=np.float64):
    """Source coordinates for every output pixel of `shape` (rows, cols[, bands]);
    `coord_map` works on (N, 2) arrays of (col, row) pairs (_warps.py:640-742)."""
    shape = tuple(int(s) for s in shape)
    rows, cols = shape[0], shape[1]
    coords_shape = [len(shape), rows, cols] + ([shape[2]] if len(shape) == 3 else [])
    coords = np.empty(coords_shape, dtype=dtype)
    tf = np.indices((cols, rows), dtype=dtype).reshape(2, -1).T
    tf = np.asarray(coord_map(tf))
    tf = tf.T.reshape((-1, cols, rows)).swapaxes(1, 2)
    if len(shape) == 3:
        coords[1, ...] = tf[0][..., None]
        coords[0, ...] = tf[1][..., None]
        coords[2, ...] = np.arange(shape[2], dtype=dtype)
    else:
        coords[1, ...] = tf[0]
        coords[0, ...] = tf[1]
    return coords


def warp(image, inverse_map, map_args={}, output_shape=None, order=None, mode="constant", cval=0.0, clip=True,
         preserve_range=False):
    """Warp an image according to an inverse coordinate map (_warps.py:790-1028)."""
    image = image if isinstance(image, core.ndarray) else core.asarray(np.asarray(image))
    if image.size == 0:
        raise ValueError("Cannot warp empty image with dimensions", image.shape)
    order = _validate_interpolation_order(image.dtype, order)
    image = convert_to_float(image, preserve_range)
    input_shape = tuple(image.shape)
    output_shape = input_shape if output_shape is None else tuple(int(s) for s in output_shape)

    if isinstance(inverse_map, core.ndarray):
        coords = inverse_map
    else:
        if isinstance(inverse_map, np.ndarray) and inverse_map.shape == (3, 3):
            H = np.asarray(inverse_map, dtype=np.float64)

            def inverse_map(xy, H=H):
                src = np.c_[xy, np.ones(len(xy))] @ H.T
                return src[:, :2] / src[:, 2:3]
        if isinstance(inverse_map, np.ndarray):
            coords = inverse_map
        else:
            if image.ndim < 2 or image.ndim > 3:
                raise ValueError("Only 2-D images (grayscale or color) are supported, when providing a "
                                 "callable `inverse_map`.")
            if len(input_shape) == 3 and len(output_shape) == 2:
                output_shape = (output_shape[0], output_shape[1], input_shape[2])
            coords = warp_coords(lambda xy: inverse_map(xy, **map_args), output_shape)
        coords = core.asarray(np.ascontiguousarray(coords))

    warped = ndi.map_coordinates(image, coords, prefilter=order > 1, mode=_to_ndimage_mode(mode), order=order,
                                 cval=cval)
    if clip and order != 0:
        # clip to the input range, keeping cval where it marks the outside (_warps.py:745-787)
        lo, hi = S.min_max(image)
        keep = (mode == "constant") and not (lo <= cval <= hi)
        warped = S.clip(warped, lo, hi, cval if keep else None)
    return warped


def _clip_like_warp(image, out, order, mode, cval, clip):
    """clip to the input range, keeping cval where it marks the outside (_warps.py:745-787)"""
    if clip and order != 0:
        lo, hi = S.min_max(image)
        keep = (mode == "constant") and not (lo <= cval <= hi)
        out = S.clip(out, lo, hi, cval if keep else None)
    return out


def resize(image, output_shape, order=None, mode="reflect", cval=0, clip=True, preserve_range=False, anti_aliasing=None,
           anti_aliasing_sigma=None):
    """Resize an n-dimensional image to `output_shape` (_warps.py:30-248).

    Output sample i of an axis reads the input at factor * (i + 0.5) - 0.5, factor = input length / output length
    (pixel centres at half-integers).  An `output_shape` one shorter than the rank is the multi-channel case: the
    leading axes are resized and the last axis is kept; a longer one appends axes of length 1 to the image.  With
    `anti_aliasing` (the default for non-bool images) one `gaussian_filter` call with sigma max(0, (factor - 1) / 2)
    per axis (or `anti_aliasing_sigma`) comes first, on the image as it is, before the conversion to float.  The
    result is clipped to the input's range as `warp` clips.

    One launch of the affine route with a diagonal matrix and an offset at every rank (what `zoom(grid_mode=True)`
    uses; no coordinate array is made).  Deviation: for 2-D images (and 2-D plus channels) the reference reaches the
    same map through an AffineTransform estimated from three corner points, which can differ from this map in the
    last bit of a coordinate."""
    image = image if isinstance(image, core.ndarray) else core.asarray(np.asarray(image))
    output_shape = tuple(int(s) for s in output_shape)
    output_ndim = len(output_shape)
    input_shape = tuple(image.shape)
    if output_ndim > image.ndim:
        input_shape = input_shape + (1,) * (output_ndim - image.ndim)
        image = image.reshape(input_shape)
    elif output_ndim == image.ndim - 1:
        output_shape = output_shape + (image.shape[-1],)
    elif output_ndim < image.ndim - 1:
        raise ValueError("len(output_shape) cannot be smaller than the image dimensions")
    if image.size == 0 or any(s < 1 for s in output_shape):
        raise ValueError("Cannot resize an empty image or to an empty shape")

    if anti_aliasing is None:
        anti_aliasing = not image.dtype == np.bool_
    if image.dtype == np.bool_ and anti_aliasing:
        warnings.warn("Input image dtype is bool. Gaussian convolution is not defined with bool data type. Please set "
                      "anti_aliasing to False or explicitely cast input image to another data type. Starting from "
                      "version 0.19 a ValueError will be raised instead of this warning.", FutureWarning, stacklevel=2)

    factors = np.asarray(input_shape, dtype=float) / np.asarray(output_shape, dtype=float)

    if anti_aliasing:
        if anti_aliasing_sigma is None:
            anti_aliasing_sigma = np.maximum(0, (factors - 1) / 2)
        else:
            anti_aliasing_sigma = np.atleast_1d(anti_aliasing_sigma) * np.ones_like(factors)
            if np.any(anti_aliasing_sigma < 0):
                raise ValueError("Anti-aliasing standard deviation must be greater than or equal to zero")
            elif np.any((anti_aliasing_sigma > 0) & (factors <= 1)):
                warnings.warn("Anti-aliasing standard deviation greater than zero but not down-sampling along all axes")
        image = ndi.gaussian_filter(image, [float(s) for s in anti_aliasing_sigma], cval=cval, mode=_to_ndimage_mode(mode))

    order = _validate_interpolation_order(image.dtype, order)
    image = convert_to_float(image, preserve_range)
    ndi_mode = _to_ndimage_mode(mode)
    out = ndi.affine_transform(image, np.diag(factors), offset=0.5 * factors - 0.5, output_shape=output_shape, order=order,
                               mode=ndi_mode, cval=cval)
    return _clip_like_warp(image, out, order, mode, cval, clip)


def _smooth(image, sigma, mode, cval, multichannel=None):
    """every channel smoothed by the Gaussian filter (pyramids.py:11-19; `mode` goes to ndimage as it is)"""
    smoothed = core.empty_like(image)
    if multichannel:
        sigma = (sigma,) * (image.ndim - 1) + (0,)
    ndi.gaussian_filter(image, sigma, output=smoothed, mode=mode, cval=cval)
    return smoothed


def _check_factor(factor):
    if factor <= 1:
        raise ValueError("scale factor must be greater than 1")


def pyramid_reduce(image, downscale=2, sigma=None, order=1, mode="reflect", cval=0, multichannel=False, preserve_range=False):
    """Smooth (sigma = 2 * downscale / 6 by default), then `resize` to ceil(n / downscale) samples per axis
    (pyramids.py:27-97); with `multichannel` the last axis is kept."""
    _check_factor(downscale)
    image = image if isinstance(image, core.ndarray) else core.asarray(np.asarray(image))
    image = convert_to_float(image, preserve_range)
    out_shape = tuple([math.ceil(d / float(downscale)) for d in image.shape])
    if multichannel:
        out_shape = out_shape[:-1]
    if sigma is None:
        sigma = 2 * downscale / 6.0
    smoothed = _smooth(image, sigma, mode, cval, multichannel)
    return resize(smoothed, out_shape, order=order, mode=mode, cval=cval, anti_aliasing=False)


def pyramid_expand(image, upscale=2, sigma=None, order=1, mode="reflect", cval=0, multichannel=False, preserve_range=False):
    """`resize` to ceil(upscale * n) samples per axis, then smooth (sigma = 2 * upscale / 6 by default)
    (pyramids.py:100-165); with `multichannel` the last axis is kept."""
    _check_factor(upscale)
    image = image if isinstance(image, core.ndarray) else core.asarray(np.asarray(image))
    image = convert_to_float(image, preserve_range)
    out_shape = tuple([math.ceil(upscale * d) for d in image.shape])
    if multichannel:
        out_shape = out_shape[:-1]
    if sigma is None:
        sigma = 2 * upscale / 6.0
    resized = resize(image, out_shape, order=order, mode=mode, cval=cval, anti_aliasing=False)
    return _smooth(resized, sigma, mode, cval, multichannel)
