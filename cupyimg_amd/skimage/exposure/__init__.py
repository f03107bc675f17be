"""skimage.exposure subset (cupyimg/skimage/exposure/exposure.py, _adapthist.py): rescale_intensity, histogram,
cumulative_distribution, equalize_hist and equalize_adapthist (CLAHE) on HIP kernels (csrc/exposure.hip; the histograms of
`histogram` by the labelled-reduction kernel of csrc/measure.hip)."""
import ctypes
import numbers
import warnings

import numpy as np

from ... import core
from ...scipy.ndimage import _support as S
from ...scipy.ndimage import measurements as _M

__all__ = ["rescale_intensity", "histogram", "cumulative_distribution", "equalize_hist", "equalize_adapthist"]

NR_OF_GRAY = 2 ** 14                    # MI_CLAHE_GRAY
_MAX_NDIM = 4                           # MI_CLAHE_MAX_NDIM
_WORK_BYTES = 16                        # MI_CLAHE_WORK_BYTES
_MAX_KNOTS = 65536                      # MI_INTERP_MAX_KNOTS
_MAX_INT_BINS = 1 << 26                 # one bin per integer value: a 512 MiB table of counters at most

_INT_NAMES = ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64")
DTYPE_RANGE = {name: (int(np.iinfo(name).min), int(np.iinfo(name).max)) for name in _INT_NAMES}
DTYPE_RANGE.update({"float16": (-1, 1), "float32": (-1, 1), "float64": (-1, 1), "float": (-1, 1), "bool": (False, True),
                    "uint10": (0, 2 ** 10 - 1), "uint12": (0, 2 ** 12 - 1), "uint14": (0, 2 ** 14 - 1)})


def _range_key(value):
    """The DTYPE_RANGE key of a dtype name, a NumPy scalar type or a dtype; None for anything else."""
    if isinstance(value, str):
        return value if value in DTYPE_RANGE else None
    if isinstance(value, (type, np.dtype)):
        try:
            name = np.dtype(value).name
        except TypeError:
            return None
        return name if name in DTYPE_RANGE else None
    return None


def _dtype_limits(dtype):
    return DTYPE_RANGE[np.dtype(dtype).name]


def _intensity_range(image, range_values, clip_negative=False, extrema=None):
    """exposure.py:260-300; `extrema`: a callable that gives the image's (min, max), asked at most once"""
    if isinstance(range_values, str) and range_values == "dtype":
        range_values = image.dtype
    if isinstance(range_values, str) and range_values == "image":
        return extrema()
    key = _range_key(range_values)
    if key is not None:
        i_min, i_max = DTYPE_RANGE[key]
        if clip_negative:
            i_min = 0
        return i_min, i_max
    if isinstance(range_values, (str, type, np.dtype)):
        raise ValueError("Incorrect value for a range, should be 'image', 'dtype', a valid image data type or a pair of "
                         "values, got {}.".format(range_values))
    i_min, i_max = range_values
    return i_min, i_max


def _output_dtype(dtype_or_range):
    """exposure.py:303-344"""
    if type(dtype_or_range) in (list, tuple, np.ndarray):
        return np.dtype(np.float64)
    key = _range_key(dtype_or_range)
    if key is None:
        raise ValueError("Incorrect value for out_range, should be a valid image data type or a pair of values, got {}."
                         .format(dtype_or_range))
    if key in ("uint10", "uint12", "uint14"):
        return np.dtype(np.uint16)
    return np.dtype(key)


def rescale_intensity(image, in_range="image", out_range="dtype"):
    """Stretch or shrink the intensity levels of an image (exposure.py:347-463).

    `in_range` and `out_range`: 'image' (the image's min and max), 'dtype' (the range of the image's dtype), a dtype name
    ('uint8' ... 'float64', 'uint10', 'uint12', 'uint14', 'bool', 'float') or a (min, max) pair.  The result has the
    image's dtype for 'image' / 'dtype', the named dtype (uint16 for uint10 .. uint14) for a name, and float64 for a pair.
    The arithmetic is clip(image, imin, imax), then (x - imin) / (imax - imin), then * (omax - omin) + omin, each operation
    rounded on its own in float32 for float32 images and in float64 otherwise; a constant range (imin == imax) is only
    clipped to the output range.  One launch (plus the min / max reduction when a range is 'image').  float16 images are
    computed as float32.  A NaN in a floating-point image is the image's min and max, as it is to NumPy: the warning of the
    reference is given and the whole result is NaN.  A wrong `out_range` name is refused before the device is touched."""
    named = not (isinstance(out_range, str) and out_range in ("dtype", "image"))
    if named:
        out_dtype = _output_dtype(out_range)
    image = S.as_device(image)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    if not named:
        out_dtype = _output_dtype(image.dtype)
    src = core.ascontiguousarray(image)
    cache = []

    def extrema():
        if not cache:
            if src.dtype.kind == "f":
                # S.min_max skips NaN; the whole-array extrema of ndimage give NaN for both when the image holds one
                both, _, _, _, _ = _M._extrema(src, None, None, False)
                lo, hi = both.get()[0]
                cache.append((float(lo), float(hi)))
            else:
                cache.append(S.min_max(src))
        return cache[0]

    imin, imax = map(float, _intensity_range(src, in_range, extrema=extrema))
    omin, omax = map(float, _intensity_range(src, out_range, clip_negative=(imin >= 0), extrema=extrema))
    if np.any(np.isnan([imin, imax, omin, omax])):
        warnings.warn("One or more intensity levels are NaN. Rescaling will broadcast NaN to the full image. Provide "
                      "intensity levels yourself to avoid this. E.g. with np.nanmin(image), np.nanmax(image).", stacklevel=2)
    out = core.empty(src.shape, out_dtype)
    if src.size:
        a, o = src._desc(), out._desc()
        S.check(S.lib().mi_rescale_intensity(ctypes.byref(a), ctypes.byref(o), imin, imax, omin, omax, None))
    return out


# ---------------------------------------------------------------- histograms
def _float_edges(dtype, lo, hi, nbins, explicit):
    """The bin edges numpy.histogram(a, nbins, range) uses for a floating-point array: numpy.linspace in the array's
    dtype between the array's extrema (`explicit` false: NumPy scalars of that dtype, widened by 0.5 when equal) or
    between the two numbers of `range`."""
    dtype = np.dtype(dtype)
    if explicit:
        first, last = lo, hi
    else:
        first, last = dtype.type(lo), dtype.type(hi)
    if first == last:
        first, last = first - 0.5, last + 0.5
    return np.linspace(first, last, nbins + 1, endpoint=True, dtype=dtype)


def _masked(image, mask):
    image = S.as_device(image)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    labels = None
    if mask is not None:
        labels = mask if isinstance(mask, core.ndarray) else core.asarray(np.asarray(mask, dtype=bool))
        if labels.shape != image.shape:
            raise ValueError("mask must have the image's shape")
        if labels.dtype != np.bool_:
            labels = labels.astype(np.bool_)
        labels = core.ascontiguousarray(labels.astype(np.int32))
    return core.ascontiguousarray(image), labels


def _extrema(image, labels):
    if labels is None:
        return S.min_max(image)
    out, _, _, _, _ = _M._extrema(image, labels, 1, False)
    lo, hi = out.get()[0]
    return float(lo), float(hi)


def _counts(image, labels, edges):
    bins = edges.size - 1
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    out, _, _, _, _ = _M._reduce(_M._OPS["hist"], image, labels, None if labels is None else 1, hist=(edges, bins))
    return out.get()[0, :bins]


def _histogram_host(image, labels, nbins, source_range, normalize, max_bins=_MAX_INT_BINS):
    """(hist, bin_centers) as host arrays; image: contiguous device array, labels: int32 device array (1 = counted) or None.
    More than `max_bins` bins are refused before any of them is counted."""
    edge_dtype = image.dtype
    limits = _dtype_limits(image.dtype)
    if image.dtype.kind == "b":
        # not an integer dtype to the reference (numpy.issubdtype(bool, numpy.integer) is false): numpy.histogram, which
        # counts a bool image as uint8 in `nbins` bins between float64 edges
        image = image.astype(np.uint8)
        edge_dtype = np.dtype(np.float64)
    if edge_dtype.kind in "iu":
        if source_range not in ("image", "dtype"):
            raise ValueError("Incorrect value for `source_range` argument: {}".format(source_range))
        if source_range == "image":
            lo, hi = _extrema(image, labels)
            image_min, image_max = int(lo), int(hi)
        else:
            image_min, image_max = limits
        n = image_max - image_min + 1
        if n > max_bins:
            raise ValueError("histogram: one bin per integer value would need {} bins (at most {})".format(n, max_bins))
        # one bin per integer value: the edges image_min .. image_max + 1 are exact in float64
        hist = _counts(image, labels, np.arange(image_min, image_max + 2, dtype=np.float64))
        bin_centers = np.arange(image_min, image_max + 1)
    else:
        nbins = int(nbins)
        if nbins < 1:
            raise ValueError("`bins` must be positive, when an integer")
        if nbins > max_bins:
            raise ValueError("histogram: at most {} bins, got {}".format(max_bins, nbins))
        if source_range == "image":
            lo, hi = _extrema(image, labels)
            if not (np.isfinite(lo) and np.isfinite(hi)):
                raise ValueError("autodetected range of [{}, {}] is not finite".format(lo, hi))
            edges = _float_edges(edge_dtype, lo, hi, nbins, False)
        elif source_range == "dtype":
            lo, hi = limits
            edges = _float_edges(edge_dtype, lo, hi, nbins, True)
        else:
            raise ValueError("Wrong value for the `source_range` argument")
        hist = _counts(image, labels, edges)
        bin_centers = (edges[:-1] + edges[1:]) / 2.0
    if normalize:
        hist = hist / np.sum(hist)
    return hist, bin_centers


def histogram(image, nbins=256, source_range="image", normalize=False):
    """Histogram of an image and the centres of its bins, as device arrays (exposure.py:96-171).

    Integer images get one bin per integer value between the image's extrema (`source_range` 'image') or the limits of
    the dtype ('dtype'); `nbins` is ignored for them.  Floating-point images follow numpy.histogram(image, nbins, range)
    with the range of the image or (-1, 1); so do bool images, which are no integers to the reference, with the range of
    the image or (0, 1) and float64 centres.  The counts come from the histogram kernel of ndimage.histogram over explicit
    float64 edges; `normalize` divides them by their sum."""
    shape = image.shape if isinstance(image, core.ndarray) else np.shape(image)
    if len(shape) == 3 and shape[-1] < 4:
        warnings.warn("This might be a color image. The histogram will be computed on the flattened image. You can instead "
                      "apply this function to each color channel.", stacklevel=2)
    img, _ = _masked(image, None)
    hist, centers = _histogram_host(img, None, nbins, source_range, normalize)
    return core.asarray(hist), core.asarray(centers)


def _cdf_host(image, labels, nbins, max_bins=_MAX_INT_BINS):
    hist, centers = _histogram_host(image, labels, nbins, "image", False, max_bins)
    cdf = hist.cumsum()
    cdf = cdf / float(cdf[-1])
    return cdf, centers


def cumulative_distribution(image, nbins=256):
    """(cdf, bin_centers) of an image as device arrays (exposure.py:174-212): the cumulative sum of `histogram` over its
    last value."""
    img, _ = _masked(image, None)
    cdf, centers = _cdf_host(img, None, nbins)
    return core.asarray(cdf), core.asarray(centers)


_INTERP_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32), np.dtype(np.float64))


def equalize_hist(image, nbins=256, mask=None):
    """Histogram equalisation (exposure.py:215-257): numpy.interp(image, bin_centers, cdf) as a float64 device array.

    `mask` (bool, the image's shape) selects the voxels that feed the histogram; the mapping is applied to the whole
    image.  The histogram (at most 65536 bins: `nbins` for floating-point images, one per integer value otherwise; more
    raise ValueError before the histogram is built) is cumulated on the host; the interpolation is one launch that keeps the table in LDS up to 4096 knots and searches it in
    global memory above, in NumPy's slope form with its end clamping (the reference pulls the image to the host for it)."""
    img, labels = _masked(image, mask)
    out = core.empty(img.shape, np.float64)
    if img.size == 0:
        return out
    # the table's limit is checked against the image's extrema (or nbins) before a bin is counted
    cdf, centers = _cdf_host(img, labels, nbins, _MAX_KNOTS)
    # other dtypes as float64, which is what numpy.interp makes of them (exact up to 53 bits)
    src = img if img.dtype in _INTERP_DTYPES else img.astype(np.float64)
    xp = core.asarray(np.ascontiguousarray(centers, dtype=np.float64))
    fp = core.asarray(np.ascontiguousarray(cdf, dtype=np.float64))
    a, x, f, o = src._desc(), xp._desc(), fp._desc(), out._desc()
    S.check(S.lib().mi_interp_map(ctypes.byref(a), ctypes.byref(x), ctypes.byref(f), ctypes.byref(o), None))
    return out


# ---------------------------------------------------------------- CLAHE
_CLAHE_DTYPES = ("uint8", "uint16", "float32", "float64")


def _clahe_arguments(shape, dtype, kernel_size, clip_limit, nbins):
    """Everything the grey-level algorithm can refuse without a device: -> (kernel sizes, clip limit in voxels, nbins)"""
    dtype = np.dtype(dtype)
    if dtype == np.float16:
        dtype = np.dtype(np.float32)
    ndim = len(shape)
    if ndim < 1 or ndim > _MAX_NDIM:
        raise NotImplementedError("equalize_adapthist takes arrays of rank 1 to {}".format(_MAX_NDIM))
    if dtype.kind == "i":
        raise NotImplementedError("equalize_adapthist: signed integer images are not supported (uint8, uint16, float32, float64)")
    if dtype.name not in _CLAHE_DTYPES:
        raise NotImplementedError("equalize_adapthist: {} images are not supported (uint8, uint16, float32, float64)".format(dtype))
    if int(nbins) != nbins or nbins < 1:
        raise ValueError("nbins must be a positive integer")
    nbins = int(nbins)
    if nbins > NR_OF_GRAY:
        raise ValueError("nbins must be at most {} (the number of grey levels the algorithm works with)".format(NR_OF_GRAY))
    if any(s == 0 for s in shape):
        raise ValueError("equalize_adapthist: empty image")
    if kernel_size is None:
        kernel_size = tuple(s // 8 for s in shape)
    elif isinstance(kernel_size, numbers.Number):
        kernel_size = (kernel_size,) * ndim
    elif len(kernel_size) != ndim:
        raise ValueError("Incorrect value of `kernel_size`: {}".format(kernel_size))
    kernel = [int(k) for k in kernel_size]
    if any(k < 1 for k in kernel):
        raise ValueError("kernel_size must be at least 1 along every axis, got {} (the default, shape // 8, needs axes of "
                         "at least 8 samples)".format(tuple(kernel)))
    npix = int(np.prod(kernel, dtype=object))
    if npix > 1 << 30:
        raise ValueError("kernel_size: a contextual region holds at most 2**30 voxels")
    if clip_limit > 0.0:
        clim = int(max(clip_limit * npix, 1))
    else:
        clim = npix
    return kernel, min(clim, npix), nbins             # no bin can hold more than the region: a larger limit clips nothing


def _as_uint_scalar(value, dtype):
    """img_as_uint of one value of the image (util/dtype.py:300-332, 354-362): the conversion is monotone, so the extrema of
    the converted image are the converted extrema"""
    if dtype == np.uint8:
        return float(int(value) * 257)
    if dtype == np.uint16:
        return float(int(value))
    t = dtype.type(value) * dtype.type(65535)
    return float(np.clip(np.rint(t), 0, 65535))


def _clahe_plan(image, kernel_size, clip_limit, nbins):
    """-> (contiguous device image, kernel sizes, umin, umax, clip limit, nbins, regions per axis)"""
    shape = image.shape if isinstance(image, core.ndarray) else np.shape(image)
    dtype = image.dtype if isinstance(image, (core.ndarray, np.ndarray)) else np.asarray(image).dtype
    kernel, clim, nbins = _clahe_arguments(tuple(shape), dtype, kernel_size, clip_limit, nbins)
    img = S.as_device(image)
    if img.dtype == np.float16:
        img = img.astype(np.float32)
    img = core.ascontiguousarray(img)
    lo, hi = S.min_max(img)
    if img.dtype.kind == "f" and (lo < -1.0 or hi > 1.0):
        raise ValueError("Images of type float must be between -1 and 1.")
    umin, umax = _as_uint_scalar(lo, img.dtype), _as_uint_scalar(hi, img.dtype)
    regions = [-(-s // k) for s, k in zip(img.shape, kernel)]
    return img, kernel, umin, umax, clim, nbins, regions


def _clahe_maps(plan):
    """The grey-level mappings of the contextual regions: uint16 device array (regions, nbins)"""
    img, kernel, umin, umax, clim, nbins, regions = plan
    maps = core.empty((int(np.prod(regions)), nbins), np.uint16)
    a, m = img._desc(), maps._desc()
    S.check(S.lib().mi_clahe_maps(ctypes.byref(a), S.c_ints(kernel), umin, umax, nbins, clim, ctypes.byref(m), None))
    return maps


def _clahe_apply(plan, maps):
    """The blend of the mappings: (uint16 device array of the image's shape, the 16-byte block that holds its min and max)"""
    img, kernel, umin, umax, clim, nbins, regions = plan
    lib = S.lib()
    v = core.empty(img.shape, np.uint16)
    work = core.empty((_WORK_BYTES,), np.uint8)
    S.check(lib.mi_memset(work.ptr, 0xff, _WORK_BYTES, None))
    a, m, d = img._desc(), maps._desc(), v._desc()
    S.check(lib.mi_clahe_apply(ctypes.byref(a), S.c_ints(kernel), umin, umax, nbins, ctypes.byref(m), ctypes.byref(d),
                               ctypes.c_void_p(work.ptr), None))
    return v, work


def equalize_adapthist(image, kernel_size=None, clip_limit=0.01, nbins=256):
    """Contrast limited adaptive histogram equalisation (CLAHE) of an n-dimensional image (_adapthist.py:36-104): a float64
    device array of the image's shape, bit-identical to the reference.

    `kernel_size`: the shape of the contextual regions -- None (shape // 8 per axis), a number, or one value per axis;
    `clip_limit` between 0 and 1 (0 or >= 1: no clipping); `nbins` 1 .. 16384.  uint8, uint16, float32 and float64 images
    (floats within [-1, 1], converted as img_as_uint does; float16 as float32) of rank 1 to 4.

    One min / max reduction of the input, then three launches with no host round trip: the mappings of the contextual
    regions (one workgroup per region: histogram, clip and cumulative sum in LDS), the multilinear blend (ranks 2 and 3:
    the 2^ndim mappings of an interpolation cell in LDS; ranks 1 and 4, or mappings that do not fit: one thread per voxel)
    and the final rescale, whose min and max the blend left on the device.  The padded image of the reference never exists.

    Deviations, all of which raise: an (M, N, 3 or 4) array is an RGB(A) image to the reference -- NotImplementedError (no
    colour module here); a kernel size below 1 (the default on an axis shorter than 8) -- ValueError (the reference: a
    division by zero); a `kernel_size` sequence of the wrong length -- ValueError (the reference builds that error and does
    not raise it); signed integer images -- NotImplementedError; nbins above 16384 -- ValueError.

    Besides the input a call holds a uint16 volume, the float64 result and regions x nbins x 2 bytes of mappings."""
    shape = image.shape if isinstance(image, core.ndarray) else np.shape(image)
    if len(shape) == 3 and shape[-1] in (3, 4):
        raise NotImplementedError("equalize_adapthist: an (M, N, 3) or (M, N, 4) array is an RGB(A) image to skimage, which "
                                  "equalises its HSV value channel; this package has no colour module")
    return _adapthist_grey(image, kernel_size, clip_limit, nbins)


def _adapthist_grey(image, kernel_size=None, clip_limit=0.01, nbins=256):
    """equalize_adapthist without the colour dispatch of its decorator (the reference: `adapt_rgb(hsv_value)` around this
    body, _adapthist.py:35): every array is a grey-level image, an (M, N, 3) one too."""
    plan = _clahe_plan(image, kernel_size, clip_limit, nbins)
    v, work = _clahe_apply(plan, _clahe_maps(plan))
    out = core.empty(v.shape, np.float64)
    d, o = v._desc(), out._desc()
    S.check(S.lib().mi_clahe_finish(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(work.ptr), None))
    return out
