"""skimage.filters thresholding (cupyimg/skimage/filters/thresholding.py) on the kernels of csrc/threshold.hip.

The histogram methods (otsu, yen, isodata, minimum, triangle, multiotsu) make one call into the device histogram of
skimage.exposure and do their arithmetic on the few hundred bins on the host, in the reference's operation order; the window
statistics of niblack and sauvola, Li's iteration, the multi-Otsu search and the comparison `image > threshold` are HIP.

Return types (a deviation from the reference, which returns 0-d device arrays): the scalar thresholds are NumPy scalars -- of
the integer dtype of the bin centres for integer images, float64 for float images; threshold_isodata(return_all=True) and
threshold_multiotsu return host NumPy arrays; the image-sized results are float64 device arrays.  `hist=` takes counts, or
(counts, bin_centers), as host or device arrays."""
import ctypes
import math
import warnings
from collections.abc import Iterable

import numpy as np

from ... import core
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ...scipy.ndimage import measurements as _M
from .. import exposure as E

__all__ = ["try_all_threshold", "threshold_otsu", "threshold_yen", "threshold_isodata", "threshold_li", "threshold_local",
           "threshold_minimum", "threshold_mean", "threshold_niblack", "threshold_sauvola", "threshold_triangle",
           "threshold_multiotsu"]

MULTIOTSU_MAX_TUPLES = 2 ** 34


def try_all_threshold(image, figsize=(8, 5), verbose=True):
    """The reference draws a matplotlib figure of seven thresholded copies of the image (thresholding.py:95-157); this
    package has no plotting dependency."""
    raise NotImplementedError("try_all_threshold needs matplotlib, which this package does not depend on; call the "
                              "threshold_* functions and compare `image > threshold` yourself")


# ---------------------------------------------------------------- helpers
def _host(a):
    return a.get() if isinstance(a, core.ndarray) else np.asarray(a)


def _shape_of(image):
    return tuple(image.shape) if isinstance(image, (core.ndarray, np.ndarray)) else np.shape(image)


def _extrema(img):
    """(min, max) of a contiguous device image as NumPy does: a NaN anywhere makes both NaN"""
    if img.dtype.kind == "f":
        both, _, _, _, _ = _M._extrema(img, None, None, False)
        lo, hi = both.get()[0]
        return float(lo), float(hi)
    return S.min_max(img)


def _scalar_like(centers, value):
    """a threshold read from the bin centres: their integer dtype for integer images, float64 otherwise"""
    if np.asarray(centers).dtype.kind in "iu":
        return np.asarray(centers).dtype.type(value)
    return np.float64(value)


def _validate_image_histogram(image, hist, nbins=None):
    """thresholding.py:276-316 -> (counts as float64, bin centres), host arrays; one device histogram when `hist` is None"""
    if image is None and hist is None:
        raise Exception("Either image or hist must be provided.")
    if hist is not None:
        if isinstance(hist, (tuple, list)):
            counts, bin_centers = hist
            counts, bin_centers = _host(counts), _host(bin_centers)
        else:
            counts = _host(hist)
            bin_centers = np.arange(counts.size)
    else:
        img, _ = E._masked(image, None)
        counts, bin_centers = E._histogram_host(img, None, nbins, "image", False)
    return counts.astype(float), bin_centers


# ---------------------------------------------------------------- the arithmetic on the bins (host, NumPy)
def _otsu_index(counts, bin_centers):
    """thresholding.py:375-388"""
    with np.errstate(all="ignore"):
        weight1 = np.cumsum(counts)
        weight2 = np.cumsum(counts[::-1])[::-1]
        mean1 = np.cumsum(counts * bin_centers) / weight1
        mean2 = (np.cumsum((counts * bin_centers)[::-1]) / weight2[::-1])[::-1]
        variance12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    return int(np.argmax(variance12))


def _yen_index(counts):
    """thresholding.py:441-452: the probabilities in float32, as the reference's astype(float32) over a 0-d sum leaves them"""
    with np.errstate(all="ignore"):
        pmf = counts.astype(np.float32) / np.float32(counts.sum())
        P1 = np.cumsum(pmf)
        P1_sq = np.cumsum(pmf * pmf)
        P2_sq = np.cumsum(pmf[::-1] ** 2)[::-1]
        crit = np.log(((P1_sq[:-1] * P2_sq[1:]) ** -1) * (P1[:-1] * (1.0 - P1[:-1])) ** 2)
    return int(crit.argmax())


def _isodata_thresholds(counts, bin_centers):
    """thresholding.py:524-564"""
    with np.errstate(all="ignore"):
        counts = counts.astype(np.float32)
        csuml = np.cumsum(counts)
        csumh = csuml[-1] - csuml
        intensity_sum = counts * bin_centers
        csum_intensity = np.cumsum(intensity_sum)
        lower = csum_intensity[:-1] / csuml[:-1]
        higher = (csum_intensity[-1] - csum_intensity[:-1]) / csumh[:-1]
        all_mean = (lower + higher) / 2.0
        bin_width = bin_centers[1] - bin_centers[0]
        distances = all_mean - bin_centers[:-1]
        return bin_centers[:-1][(distances >= 0) & (distances < bin_width)]


def _smooth3(h):
    """scipy.ndimage.uniform_filter1d(h, 3) with its default 'reflect' border (the edge sample repeated), written out: the
    product imports no SciPy"""
    p = np.concatenate([h[:1], h, h[-1:]])
    return (p[:-2] + p[1:-1] + p[2:]) / 3.0


def _local_maxima(hist):
    """thresholding.py:821-839 without its Python loop over the bins: i is a maximum where the histogram falls after i and its
    last change before i was a rise (or there was none: the walk starts upwards), so a plateau counts once, at its last bin"""
    step = np.sign(hist[1:] - hist[:-1])
    moved = np.flatnonzero(step)
    if moved.size == 0:
        return []
    before = np.concatenate([[1.0], step[moved[:-1]]])          # the direction in force when each change is met
    return moved[(step[moved] < 0) & (before > 0)].tolist()


def _minimum_index(counts, max_iter):
    """thresholding.py:843-863"""
    smooth_hist = counts.astype(np.float64, copy=False)
    maximum_idxs = []
    counter = -1
    for counter in range(max_iter):
        smooth_hist = _smooth3(smooth_hist)
        maximum_idxs = _local_maxima(smooth_hist)
        if len(maximum_idxs) < 3:
            break
    if len(maximum_idxs) != 2:
        raise RuntimeError("Unable to find two maxima in histogram")
    elif counter == max_iter - 1:
        raise RuntimeError("Maximum iteration reached for histogramsmoothing")
    threshold_idx = np.argmin(smooth_hist[maximum_idxs[0]:maximum_idxs[1] + 1])
    return maximum_idxs[0] + int(threshold_idx)


def _triangle_index(hist):
    """thresholding.py:933-978"""
    hist = np.asarray(hist, dtype=np.float64)
    nbins = len(hist)
    arg_peak_height = int(np.argmax(hist))
    peak_height = hist[arg_peak_height]
    nz = np.where(hist > 0)[0]
    arg_low_level, arg_high_level = int(nz[0]), int(nz[-1])
    flip = arg_peak_height - arg_low_level < arg_high_level - arg_peak_height
    if flip:
        hist = hist[::-1]
        arg_low_level = nbins - arg_high_level - 1
        arg_peak_height = nbins - arg_peak_height - 1
    width = arg_peak_height - arg_low_level
    x1 = np.arange(width)
    y1 = hist[x1 + arg_low_level]
    with np.errstate(all="ignore"):
        norm = np.sqrt(peak_height ** 2 + width ** 2)
        peak_height = peak_height / norm
        width = width / norm
    length = peak_height * x1 - width * y1
    arg_level = int(np.argmax(length)) + arg_low_level
    if flip:
        arg_level = nbins - arg_level - 1
    return arg_level


# ---------------------------------------------------------------- global thresholds
def threshold_otsu(image=None, nbins=256, *, hist=None):
    """Otsu's threshold (thresholding.py:319-390).  A constant image returns its value: read from the min / max reduction,
    no `image == first` array is made."""
    if image is not None:
        shape = _shape_of(image)
        if len(shape) > 2 and shape[-1] in (3, 4):
            warnings.warn("threshold_otsu is expected to work correctly only for grayscale images; image shape {0} looks "
                          "like an RGB image".format(shape), stacklevel=2)
        img, _ = E._masked(image, None)
        if img.size:
            lo, hi = _extrema(img)
            if lo == hi:
                return img.dtype.type(lo)
    counts, bin_centers = _validate_image_histogram(image, hist, nbins)
    return _scalar_like(bin_centers, bin_centers[_otsu_index(counts, bin_centers)])


def threshold_yen(image=None, nbins=256, *, hist=None):
    """Yen's threshold (thresholding.py:393-452)"""
    counts, bin_centers = _validate_image_histogram(image, hist, nbins)
    if bin_centers.size == 1:
        return _scalar_like(bin_centers, bin_centers[0])
    return _scalar_like(bin_centers, bin_centers[_yen_index(counts)])


def threshold_isodata(image=None, nbins=256, return_all=False, *, hist=None):
    """ISODATA threshold(s) (thresholding.py:455-569); `return_all`: a host array of every valid threshold"""
    counts, bin_centers = _validate_image_histogram(image, hist, nbins)
    out_dtype = bin_centers.dtype if bin_centers.dtype.kind in "iu" else np.float64
    if len(bin_centers) == 1:
        return bin_centers.astype(out_dtype) if return_all else _scalar_like(bin_centers, bin_centers[0])
    thresholds = _isodata_thresholds(counts, bin_centers)
    if return_all:
        return thresholds.astype(out_dtype)
    return _scalar_like(bin_centers, thresholds[0])


def threshold_minimum(image=None, nbins=256, max_iter=10000, *, hist=None):
    """Minimum method (thresholding.py:768-863): the histogram is smoothed on the host with a three-bin mean until two maxima
    remain; RuntimeError when that fails or takes `max_iter` rounds."""
    counts, bin_centers = _validate_image_histogram(image, hist, nbins)
    return _scalar_like(bin_centers, bin_centers[_minimum_index(counts, max_iter)])


def threshold_mean(image):
    """Mean of the grey values (thresholding.py:866-894), float64: the strided sum reduction over the number of samples"""
    img = S.as_device(image)
    if img.dtype == np.float16:
        img = img.astype(np.float32)
    if img.size == 0:
        return np.float64(np.nan)
    total = ctypes.c_double()
    d = img._desc()
    S.check(S.lib().mi_sum(0, ctypes.byref(d), None, ctypes.byref(total), None))
    return np.float64(total.value) / np.float64(img.size)


def threshold_triangle(image, nbins=256):
    """Triangle threshold (thresholding.py:897-978)"""
    img, _ = E._masked(image, None)
    hist, bin_centers = E._histogram_host(img, None, nbins, "image", False)
    return _scalar_like(bin_centers, bin_centers[_triangle_index(hist)])


# ---------------------------------------------------------------- Li
def _li_sums(img, threshold, shift):
    """(count above, sum above, count at or below, sum at or below, min, max) over the finite samples of `img - shift`"""
    is_int = img.dtype.kind in "iu"
    buf = (ctypes.c_int64 * 6)()
    d = img._desc()
    S.check(S.lib().mi_li_sums(ctypes.byref(d), float(threshold), 0.0 if is_int else float(shift), int(shift) if is_int else 0,
                               ctypes.cast(buf, ctypes.c_void_p), None), ValueError)
    words = np.frombuffer(buf, dtype=np.int64).copy()
    if is_int:
        return tuple(int(v) for v in words)
    reals = words.view(np.float64)
    return int(words[0]), float(reals[1]), int(words[2]), float(reals[3]), float(reals[4]), float(reals[5])


def _li_tolerance(img, image_min, image_max):
    """half the smallest gap between distinct values of the shifted finite image (thresholding.py:715)"""
    if img.dtype.kind in "iu" and image_max - image_min + 1 <= E._MAX_INT_BINS:
        counts, _ = E._histogram_host(img, None, 0, "image", False)
        present = np.flatnonzero(counts)
        gap = float(np.min(np.diff(present))) if present.size > 1 else math.inf
    else:
        srt = core.sort(img.reshape(-1))
        res = ctypes.c_double()
        d = srt._desc()
        S.check(S.lib().mi_min_adjacent_diff(ctypes.byref(d), 0.0 if img.dtype.kind in "iu" else float(image_min), ctypes.byref(res), None),
                ValueError)
        gap = res.value
    if not math.isfinite(gap):
        raise ValueError("threshold_li: the finite values of the image are all equal; pass `tolerance`")
    return gap / 2


def threshold_li(image, *, tolerance=None, initial_guess=None, iter_callback=None):
    """Li's iterative minimum cross entropy threshold (thresholding.py:636-765), float64.

    One reduction launch per iteration returns the counts and sums of the finite samples above and at or below the current
    threshold; the host reads those four numbers.  No compacted or shifted copy of the image is made: NaN and +-inf are
    skipped, and the minimum is subtracted, inside the kernel.  Integer images are summed in int64 (exact; the reference's
    in-place `image -= image_min` wraps for int8 / int16 ranges above the dtype's maximum, this does not); float images in
    double, in a fixed order.  The default `tolerance`, half the smallest gap between distinct values, comes from the
    histogram for integer images and from the device sort plus one reduction otherwise.  A callable `initial_guess` receives
    the shifted finite samples as a 1-D device array (built on the host: the one path that copies the image)."""
    img = S.as_device(image)
    if img.dtype == np.float16:
        img = img.astype(np.float32)
    elif img.dtype == np.bool_:
        img = img.astype(np.uint8)
    elif img.dtype == np.uint64:
        img = img.astype(np.float64)
    img = core.ascontiguousarray(img)
    if img.size == 0:
        return np.float64(np.nan)
    lo, hi = S.min_max(img)                      # NaNs skipped
    if math.isnan(lo):
        return np.float64(np.nan)
    if lo == hi:                                  # one value (inf included), with or without NaNs beside it
        return img.dtype.type(lo)
    is_int = img.dtype.kind in "iu"
    n_hi, _, n_lo, _, image_min, image_max = _li_sums(img, math.inf, 0)
    if n_hi + n_lo == 0:
        return np.float64(0.0)                    # nothing finite: both inf and -inf are present
    if not is_int:
        image_min, image_max = img.dtype.type(image_min), img.dtype.type(image_max)
    tolerance = tolerance or _li_tolerance(img, image_min, image_max)
    shift = int(image_min) if is_int else float(image_min)
    with np.errstate(all="ignore"):
        if initial_guess is None:
            _, _, count, total, _, _ = _li_sums(img, math.inf, shift)
            t_next = np.float64(total) / np.float64(count)
        elif callable(initial_guess):
            host = img.get().reshape(-1)
            if not is_int:
                host = host[np.isfinite(host)]
            host = host - image_min
            guess = initial_guess(core.asarray(host))
            t_next = np.float64(_host(guess).reshape(-1)[0] if isinstance(guess, (core.ndarray, np.ndarray)) else guess)
        elif np.isscalar(initial_guess):
            t_next = np.float64(initial_guess - shift)
            if not 0 < t_next < float(image_max) - shift:
                raise ValueError("The initial guess for threshold_li must be within the range of the image. Got {} for image min "
                                 "{} and max {} ".format(initial_guess, image_min, image_max))
        else:
            raise TypeError("Incorrect type for `initial_guess`; should be a floating point value, or a function mapping an "
                            "array to a floating point value.")
        t_curr = -2 * tolerance
        if iter_callback is not None:
            iter_callback(t_next + shift)
        while abs(t_next - t_curr) > tolerance:
            t_curr = t_next
            n_fore, s_fore, n_back, s_back, _, _ = _li_sums(img, t_curr, shift)
            mean_fore = np.float64(s_fore) / np.float64(n_fore)
            mean_back = np.float64(s_back) / np.float64(n_back)
            t_next = (mean_back - mean_fore) / (np.log(mean_back) - np.log(mean_fore))
            if iter_callback is not None:
                iter_callback(t_next + shift)
    return np.float64(t_next + shift)


# ---------------------------------------------------------------- multi-Otsu
def _multiotsu_tuples(nbins, classes):
    return math.comb(nbins - 1, classes - 1)


def _check_multiotsu_count(nbins, classes):
    n = _multiotsu_tuples(nbins, classes)
    if n > MULTIOTSU_MAX_TUPLES:
        raise ValueError("threshold_multiotsu: {} bins in {} classes are {} threshold tuples; the exhaustive search takes at "
                         "most 2**34".format(nbins, classes, n))


def _multiotsu_tables(prob):
    """the running sums from 0 of p and of index * p the search kernel works on (nbins + 1 float64 each)"""
    prob = np.asarray(prob, dtype=np.float64)
    cum_p = np.concatenate([[0.0], np.cumsum(prob)])
    cum_s = np.concatenate([[0.0], np.cumsum(np.arange(prob.size, dtype=np.float64) * prob)])
    return np.ascontiguousarray(cum_p), np.ascontiguousarray(cum_s)


def _multiotsu_search(prob, classes):
    cum_p, cum_s = _multiotsu_tables(prob)
    idx = (ctypes.c_int64 * (classes - 1))()
    best = ctypes.c_double()
    S.check(S.lib().mi_multiotsu_search(cum_p.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        cum_s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(prob.size), int(classes), idx,
                                        ctypes.byref(best), None), ValueError)
    return np.array(list(idx), dtype=np.intp)


def threshold_multiotsu(image, classes=3, nbins=256):
    """classes - 1 thresholds that maximise the between-class variance (thresholding.py:1230-1341), as a host array.

    The reference calls a private Cython module of scikit-image; here a kernel evaluates every strictly increasing tuple of
    bin indices -- the sum over the classes of S_k^2 / P_k from the running sums of the normalised histogram -- and reduces
    to the maximum, the lexicographically smallest tuple among equals.  2 to 5 classes; more than 2**34 tuples raise
    ValueError before any is evaluated (for float images, whose bin count is `nbins`, before the device is touched).
    Deviation: the objective is evaluated in float64 where scikit-image's tables are float32, so a threshold can differ from
    scikit-image's only where two tuples' objectives agree to float32 precision."""
    classes = int(classes)
    if classes < 2 or classes > 5:
        raise ValueError("threshold_multiotsu: 2 to 5 classes, got {}".format(classes))
    shape = _shape_of(image)
    dtype = image.dtype if isinstance(image, (core.ndarray, np.ndarray)) else np.asarray(image).dtype
    if len(shape) > 2 and shape[-1] in (3, 4):
        warnings.warn("threshold_multiotsu is expected to work correctly only for grayscale images; image shape {0} looks "
                      "like an RGB image".format(shape), stacklevel=2)
    if np.dtype(dtype).kind not in "iu":
        _check_multiotsu_count(int(nbins), classes)
    img, _ = E._masked(image, None)
    prob, bin_centers = E._histogram_host(img, None, nbins, "image", True)
    nvalues = int(np.count_nonzero(prob))
    if nvalues < classes:
        raise ValueError("The input image has only {} different values. It can not be thresholded in {} classes".format(nvalues, classes))
    elif nvalues == classes:
        thresh_idx = np.where(prob > 0)[0][:-1]
    else:
        _check_multiotsu_count(prob.size, classes)
        thresh_idx = _multiotsu_search(prob, classes)
    thresh = bin_centers[thresh_idx]
    return thresh if thresh.dtype.kind in "iu" else thresh.astype(np.float64)


# ---------------------------------------------------------------- local thresholds
def threshold_local(image, block_size, method="gaussian", offset=0, mode="reflect", param=None, cval=0):
    """Threshold image from the local neighbourhood of each pixel (thresholding.py:160-273), 2-D, float64: the Gaussian,
    mean (two convolve1d) or median filter of this library into a float64 output, minus `offset` in one pointwise launch.
    The image enters the filters as float64 (what a float64 `output` makes the reference's kernels compute in)."""
    if block_size % 2 == 0:
        raise ValueError("The kwarg ``block_size`` must be odd! Given ``block_size`` {0} is even.".format(block_size))
    shape = _shape_of(image)
    if len(shape) != 2:
        raise ValueError("The parameter `image` must be a 2-dimensional array")
    if method == "generic":
        raise NotImplementedError("TODO: implement generic_filter")
    if method not in ("gaussian", "mean", "median"):
        raise ValueError("Invalid method specified. Please use `generic`, `gaussian`, `mean`, or `median`.")
    img = S.as_device(image)
    if img.dtype != np.float64:
        img = img.astype(np.float64)
    thresh_image = core.zeros(img.shape, np.float64)
    if method == "gaussian":
        sigma = (block_size - 1) / 6.0 if param is None else param
        ndi.gaussian_filter(img, sigma, output=thresh_image, mode=mode, cval=cval)
    elif method == "mean":
        mask = 1.0 / block_size * np.ones((block_size,))
        ndi.convolve1d(img, mask, axis=0, output=thresh_image, mode=mode, cval=cval)
        ndi.convolve1d(thresh_image, mask, axis=1, output=thresh_image, mode=mode, cval=cval)
    else:
        ndi.median_filter(img, block_size, output=thresh_image, mode=mode, cval=cval)
    return _minus_scalar(thresh_image, offset)


def _minus_scalar(a, value):
    """a - value for a float64 device array: one pointwise launch (x - v = 1.0 x + (-v), one rounding either way)"""
    return S.scale_shift(a, 1.0, -float(value))


def _validate_window_size(axis_sizes):
    """thresholding.py:981-1000"""
    for axis_size in axis_sizes:
        if axis_size % 2 == 0:
            raise ValueError("Window size for `threshold_sauvola` or `threshold_niblack` must not be even on any dimension. "
                             "Got {}".format(axis_sizes))


def _window_arguments(shape, w):
    if not isinstance(w, Iterable):
        w = (w,) * len(shape)
    w = tuple(w)
    _validate_window_size(w)
    if len(w) != len(shape):
        raise ValueError("the window has {} sizes, the image {} axes".format(len(w), len(shape)))
    w = tuple(int(k) for k in w)
    if any(k < 1 for k in w):
        raise ValueError("window sizes must be positive, got {}".format(w))
    if len(shape) < 1 or len(shape) > 8:
        raise ValueError("arrays of rank 1 to 8")
    if math.prod(w) >= 2 ** 31:
        raise ValueError("the window must hold fewer than 2**31 samples")
    return w


def _window_call(image, w, kind, k=0.0, r=1.0):
    w = _window_arguments(_shape_of(image), w)
    img = S.as_device(image)
    if img.dtype == np.float16:
        img = img.astype(np.float32)
    img = core.ascontiguousarray(img)
    out0 = core.empty(img.shape, np.float64)
    out1 = core.empty(img.shape, np.float64) if kind == 0 else None
    if img.size:
        a, o0 = img._desc(), out0._desc()
        o1 = out1._desc() if out1 is not None else None
        S.check(S.lib().mi_window_mean_std(ctypes.byref(a), S.c_ints(w), kind, float(k), float(r), ctypes.byref(o0),
                                           ctypes.byref(o1) if o1 is not None else None, None), ValueError)
    return out0, out1


def _mean_std(image, w):
    """(m, s): mean and standard deviation over the window of `w` samples (an odd int, or one per axis) around every sample,
    float64 device arrays (thresholding.py:1003-1056).  The reference pads, squares, builds two integral images and
    correlates each with a dense (w + 1)^ndim kernel; here the sums of x and x^2 are formed directly in one launch, borders
    by index arithmetic (numpy.pad's 'reflect').  m = S / n, s = sqrt(max(Q / n - m m, 0)), as the reference."""
    return _window_call(image, w, 0)


def threshold_niblack(image, window_size=15, k=0.2):
    """Niblack's local threshold T = m - k s (thresholding.py:1059-1119), float64, any rank; one launch, m and s never in memory"""
    return _window_call(image, window_size, 1, k)[0]


def threshold_sauvola(image, window_size=15, k=0.2, r=None):
    """Sauvola's local threshold T = m (1 + k (s / r - 1)) (thresholding.py:1122-1179), float64, any rank; `r` defaults to half
    the range of the image's dtype; one launch"""
    if r is None:
        dtype = image.dtype if isinstance(image, (core.ndarray, np.ndarray)) else np.asarray(image).dtype
        imin, imax = E._dtype_limits(dtype)
        r = 0.5 * (imax - imin)
    return _window_call(image, window_size, 2, k, r)[0]
