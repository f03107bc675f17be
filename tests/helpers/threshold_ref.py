"""NumPy references for skimage.filters thresholding, written from the behaviour of cupyimg/skimage/filters/thresholding.py:
the histogram methods on the histograms of tests/helpers/exposure_ref.py, the window statistics three ways (the integral
images of the reference, direct window sums, exactly rounded rational sums), Li's iteration with a choice of mean, a
brute-force multi-Otsu, and the readers of tests/golden/threshold_kat.json.  Nothing here imports the library."""
import itertools
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage as sndi

from helpers import exposure_ref

U = 2.0 ** -53


# ---------------------------------------------------------------- histogram methods
def _hist(image, hist, nbins):
    if image is None and hist is None:
        raise Exception("Either image or hist must be provided.")
    if hist is None:
        counts, centers = exposure_ref.histogram(np.asarray(image), nbins, "image")
    elif isinstance(hist, (tuple, list)):
        counts, centers = np.asarray(hist[0]), np.asarray(hist[1])
    else:
        counts = np.asarray(hist)
        centers = np.arange(counts.size)
    return counts.astype(np.float64), centers


def _typed(centers, value):
    return centers.dtype.type(value) if centers.dtype.kind in "iu" else np.float64(value)


def otsu(image=None, nbins=256, hist=None):
    if image is not None:
        a = np.asarray(image)
        if a.size and a.min() == a.max():
            return a.reshape(-1)[0]
    c, b = _hist(image, hist, nbins)
    with np.errstate(all="ignore"):
        w1 = np.cumsum(c)
        w2 = np.cumsum(c[::-1])[::-1]
        m1 = np.cumsum(c * b) / w1
        m2 = (np.cumsum((c * b)[::-1]) / w2[::-1])[::-1]
        var = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return _typed(b, b[np.argmax(var)])


def yen(image=None, nbins=256, hist=None):
    c, b = _hist(image, hist, nbins)
    if b.size == 1:
        return _typed(b, b[0])
    with np.errstate(all="ignore"):
        pmf = c.astype(np.float32) / np.float32(c.sum())
        p1 = np.cumsum(pmf)
        p1sq = np.cumsum(pmf * pmf)
        p2sq = np.cumsum(pmf[::-1] ** 2)[::-1]
        crit = np.log(((p1sq[:-1] * p2sq[1:]) ** -1) * (p1[:-1] * (1.0 - p1[:-1])) ** 2)
    return _typed(b, b[crit.argmax()])


def isodata(image=None, nbins=256, return_all=False, hist=None):
    c, b = _hist(image, hist, nbins)
    kind = b.dtype if b.dtype.kind in "iu" else np.float64
    if len(b) == 1:
        return b.astype(kind) if return_all else _typed(b, b[0])
    with np.errstate(all="ignore"):
        c = c.astype(np.float32)
        low_n = np.cumsum(c)
        high_n = low_n[-1] - low_n
        mass = np.cumsum(c * b)
        low = mass[:-1] / low_n[:-1]
        high = (mass[-1] - mass[:-1]) / high_n[:-1]
        mid = (low + high) / 2.0
        d = mid - b[:-1]
        t = b[:-1][(d >= 0) & (d < b[1] - b[0])]
    return t.astype(kind) if return_all else _typed(b, t[0])


def smooth3(h):
    """scipy.ndimage.uniform_filter1d(h, 3) ('reflect'), as the three-term mean"""
    p = np.concatenate([h[:1], h, h[-1:]])
    return (p[:-2] + p[1:-1] + p[2:]) / 3.0


def _maxima(h):
    """the last bin of every run of equal values that is higher than the run before it (if any) and the run after it"""
    starts = np.flatnonzero(np.concatenate([[True], h[1:] != h[:-1]]))
    c = h[starts]
    last = np.concatenate([starts[1:], [len(h)]]) - 1
    rises = np.concatenate([[True], c[1:] > c[:-1]])
    falls = np.concatenate([c[1:] < c[:-1], [False]])
    return last[rises & falls].tolist()


def minimum(image=None, nbins=256, max_iter=10000, hist=None):
    c, b = _hist(image, hist, nbins)
    h = c.astype(np.float64)
    peaks, k = [], -1
    for k in range(max_iter):
        h = smooth3(h)
        peaks = _maxima(h)
        if len(peaks) < 3:
            break
    if len(peaks) != 2:
        raise RuntimeError("Unable to find two maxima in histogram")
    if k == max_iter - 1:
        raise RuntimeError("Maximum iteration reached for histogramsmoothing")
    return _typed(b, b[peaks[0] + int(np.argmin(h[peaks[0]:peaks[1] + 1]))])


def mean(image):
    return np.float64(np.mean(np.asarray(image), dtype=np.float64))


def triangle(image, nbins=256):
    h, b = exposure_ref.histogram(np.asarray(image), nbins, "image")
    h = h.astype(np.float64)
    n = len(h)
    peak = int(np.argmax(h))
    height = h[peak]
    nz = np.flatnonzero(h > 0)
    low, high = int(nz[0]), int(nz[-1])
    flip = peak - low < high - peak
    if flip:
        h = h[::-1]
        low = n - high - 1
        peak = n - peak - 1
    width = peak - low
    x1 = np.arange(width)
    y1 = h[x1 + low]
    with np.errstate(all="ignore"):
        norm = np.sqrt(height ** 2 + width ** 2)
        height = height / norm
        width = width / norm
    level = int(np.argmax(height * x1 - width * y1)) + low
    if flip:
        level = n - level - 1
    return _typed(b, b[level])


# ---------------------------------------------------------------- Li
def fsum_mean(v):
    return np.float64(math.fsum(v.tolist()) / len(v)) if len(v) else np.float64(np.nan)


def numpy_mean(v):
    with np.errstate(all="ignore"):
        return np.float64(np.mean(v)) if len(v) else np.float64(np.nan)


def li(image, tolerance=None, initial_guess=None, iter_callback=None, mean_fn=numpy_mean, trace=None):
    """threshold_li on a host image.  Integers are shifted exactly (int64), floats in their own dtype; the means are taken
    over the shifted samples as float64 by `mean_fn` (numpy_mean: pairwise; fsum_mean: exactly rounded sum).  `trace`, a list,
    receives (t_curr, t_next) of every iteration."""
    a = np.asarray(image).reshape(-1)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype == np.float16:
        a = a.astype(np.float32)
    if a.dtype.kind == "f":
        a = a[~np.isnan(a)]
    if a.size == 0:
        return np.float64(np.nan)
    if np.all(a == a[0]):
        return a[0]
    if a.dtype.kind == "f":
        a = a[np.isfinite(a)]
    if a.size == 0:
        return np.float64(0.0)
    if a.dtype.kind in "iu":
        lo = int(a.min())
        v = a.astype(np.int64) - lo
        top = int(v.max())
    else:
        lo = a.min()
        v = a - lo
        top = float(v.max())
        lo = float(lo)
    if not tolerance:
        gaps = np.diff(np.unique(v))
        tolerance = float(gaps.min()) / 2
    x = v.astype(np.float64)
    with np.errstate(all="ignore"):
        if initial_guess is None:
            t_next = mean_fn(x)
        elif callable(initial_guess):
            t_next = np.float64(initial_guess(v))
        elif np.isscalar(initial_guess):
            t_next = np.float64(initial_guess - lo)
            if not 0 < t_next < top:
                raise ValueError("The initial guess for threshold_li must be within the range of the image.")
        else:
            raise TypeError("Incorrect type for `initial_guess`")
        t_curr = -2 * tolerance
        if iter_callback is not None:
            iter_callback(t_next + lo)
        while abs(t_next - t_curr) > tolerance:
            t_curr = t_next
            fore = x > t_curr
            mf, mb = mean_fn(x[fore]), mean_fn(x[~fore])
            t_next = (mb - mf) / (np.log(mb) - np.log(mf))
            if trace is not None:
                trace.append((float(t_curr), float(t_next)))
            if iter_callback is not None:
                iter_callback(t_next + lo)
    return np.float64(t_next + lo)


# ---------------------------------------------------------------- multi-Otsu
def multiotsu_tables(prob):
    prob = np.asarray(prob, dtype=np.float64)
    return (np.concatenate([[0.0], np.cumsum(prob)]),
            np.concatenate([[0.0], np.cumsum(np.arange(prob.size, dtype=np.float64) * prob)]))


def _term(cp, cs, lo, hi):
    """S^2 / P of the bins lo .. hi (hi may be an array)"""
    p = cp[np.asarray(hi) + 1] - cp[lo]
    s = cs[np.asarray(hi) + 1] - cs[lo]
    with np.errstate(all="ignore"):
        return np.where(p > 0.0, s * s / p, 0.0)


def multiotsu_brute(prob, classes, runner_up=False):
    """the strictly increasing tuple of classes - 1 bin indices (the last at most nbins - 2) with the largest sum over the
    classes, from the lowest, of S_k^2 / P_k in float64; among equal sums the lexicographically smallest.  With `runner_up`:
    (tuple, best, second best value)."""
    cp, cs = multiotsu_tables(prob)
    nbins = len(cp) - 1
    k = classes - 1
    best, best_t, second = -math.inf, None, -math.inf
    for prefix in itertools.combinations(range(nbins - 2), k - 1):
        base, lo = 0.0, 0
        for t in prefix:
            base = base + float(_term(cp, cs, lo, t))
            lo = t + 1
        u = np.arange(lo, nbins - 1)
        if not u.size:
            continue
        vals = base + _term(cp, cs, lo, u)
        vals = vals + _term(cp, cs, u + 1, nbins - 1)
        j = int(np.argmax(vals))
        order = np.sort(vals)
        cands = [order[-1]] + ([order[-2]] if order.size > 1 else [])
        if vals[j] > best:
            second = max(second, best, *cands[1:])
            best, best_t = float(vals[j]), tuple(prefix) + (int(u[j]),)
        else:
            second = max(second, *cands)
    return (best_t, best, second) if runner_up else best_t


def multiotsu_exact(counts, thresholds):
    """the objective of one tuple as an exact rational, from integer counts"""
    total, n = sum(counts), len(counts)
    edges = [-1] + list(thresholds) + [n - 1]
    value = Fraction(0)
    for a, b in zip(edges[:-1], edges[1:]):
        p = Fraction(sum(counts[a + 1:b + 1]), total)
        s = Fraction(sum(i * counts[i] for i in range(a + 1, b + 1)), total)
        if p > 0:
            value += s * s / p
    return value


def multiotsu_float(counts, thresholds):
    """the same in float64 from the tables, in the search's order of operations"""
    cp, cs = multiotsu_tables(np.asarray(counts, dtype=np.float64) / sum(counts))
    value, lo = 0.0, 0
    for t in list(thresholds) + [len(counts) - 1]:
        value = value + float(_term(cp, cs, lo, t))
        lo = t + 1
    return value


def multiotsu(image, classes=3, nbins=256):
    prob, centers = exposure_ref.histogram(np.asarray(image), nbins, "image", normalize=True)
    nvalues = int(np.count_nonzero(prob))
    if nvalues < classes:
        raise ValueError("The input image has only {} different values. It can not be thresholded in {} classes".format(nvalues, classes))
    if nvalues == classes:
        idx = np.flatnonzero(prob > 0)[:-1]
    else:
        idx = np.array(multiotsu_brute(prob, classes), dtype=np.intp)
    out = centers[idx]
    return out if out.dtype.kind in "iu" else out.astype(np.float64)


# ---------------------------------------------------------------- window statistics
def _window(shape, w):
    w = tuple(w) if hasattr(w, "__iter__") else (w,) * len(shape)
    if any(k % 2 == 0 for k in w):
        raise ValueError("Window size for `threshold_sauvola` or `threshold_niblack` must not be even on any dimension. Got {}".format(w))
    return w


def _finish(S, Q, n):
    m = S / n
    g2 = Q / n
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.clip(g2 - m * m, 0, None))
    return m, s


def _integral_window_sums(padded, w):
    """the window sums of a padded array from its integral image: the inclusion-exclusion over the 2^ndim corners"""
    integral = padded
    for ax in range(padded.ndim):
        integral = np.cumsum(integral, axis=ax)
    out_shape = tuple(n - k for n, k in zip(padded.shape, w))
    total = np.zeros(out_shape, np.float64)
    for corner in itertools.product((0, 1), repeat=padded.ndim):
        sl = tuple(slice(k, k + n) if c else slice(0, n) for c, k, n in zip(corner, w, out_shape))
        sign = (-1) ** (padded.ndim - sum(corner))
        total = total + sign * integral[sl]
    return total


def mean_std_integral(image, w):
    """_mean_std as the reference computes it: float64 image padded (k // 2 + 1, k // 2) by reflection, squared, two integral
    images, the corner differences"""
    image = np.asarray(image)
    w = _window(image.shape, w)
    pad = tuple((k // 2 + 1, k // 2) for k in w)
    padded = np.pad(image.astype(np.float64), pad, mode="reflect")
    n = int(np.prod(w))
    return _finish(_integral_window_sums(padded, w), _integral_window_sums(padded * padded, w), n)


def _windows(image, w):
    """(output shape + window shape) view of the image padded k // 2 either way by reflection"""
    pad = tuple((k // 2, k // 2) for k in w)
    return np.lib.stride_tricks.sliding_window_view(np.pad(image, pad, mode="reflect"), w)


def _axis_window_sum(a, k, axis):
    """sum over the k samples around every sample along one axis (reflected border), added from the lowest index, from 0"""
    p = np.pad(a, [(k // 2, k // 2) if d == axis else (0, 0) for d in range(a.ndim)], mode="reflect")
    acc = np.zeros(a.shape, a.dtype)
    for t in range(k):
        acc = acc + np.take(p, np.arange(t, t + a.shape[axis]), axis=axis)
    return acc


def mean_std_direct(image, w):
    """the same from direct window sums, formed axis by axis, the last axis first: integers in int64 (exact in any order),
    floats in float64"""
    image = np.asarray(image)
    w = _window(image.shape, w)
    n = int(np.prod(w))
    x = image.astype(np.int64 if image.dtype.kind in "biu" else np.float64)
    S, Q = x, x * x
    for axis in reversed(range(image.ndim)):
        S, Q = _axis_window_sum(S, w[axis], axis), _axis_window_sum(Q, w[axis], axis)
    return _finish(S.astype(np.float64), Q.astype(np.float64), n)


def integral_sum_bound(image, w):
    """the largest value an integral image of the reference's form holds: (sum |x|, sum x^2) over the padded image"""
    image = np.asarray(image)
    w = _window(image.shape, w)
    padded = np.pad(image.astype(np.int64), tuple((k // 2 + 1, k // 2) for k in w), mode="reflect")
    return int(np.abs(padded).sum()), int((padded * padded).sum())


def exact_window_moments(image, w):
    """per output, as exact rationals: (sum |x|, sum x, sum x^2) -- object arrays of Fractions"""
    image = np.asarray(image)
    w = _window(image.shape, w)
    v = _windows(image.astype(np.float64), w).reshape(image.shape + (-1,))
    sa = np.empty(image.shape, object)
    sx = np.empty(image.shape, object)
    sq = np.empty(image.shape, object)
    for idx in np.ndindex(*image.shape):
        fr = [Fraction(float(t)) for t in v[idx]]
        sa[idx] = sum(abs(t) for t in fr)
        sx[idx] = sum(fr)
        sq[idx] = sum(t * t for t in fr)
    return sa, sx, sq


def gamma(k):
    return Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))


def check_mean_std_bounds(image, w, m_dev, s_dev):
    """the derived bounds of the float window statistics against exactly rounded sums; returns the largest ratios error / bound
    of m and of s^2 (both at most 1, asserted)"""
    w = _window(np.shape(image), w)
    n = int(np.prod(w))
    u = Fraction(U)
    sa, sx, sq = exact_window_moments(image, w)
    worst_m = worst_s = Fraction(0)
    for idx in np.ndindex(*np.shape(image)):
        m = sx[idx] / n
        g2 = sq[idx] / n
        s2 = g2 - m * m
        bm = gamma(n) * sa[idx] / n + u * abs(m)
        bg = gamma(n + 1) * sq[idx] / n + u * g2
        md, sd = Fraction(float(m_dev[idx])), Fraction(float(s_dev[idx]))
        em = abs(md - m)
        assert em <= bm, ("mean", idx, float(em), float(bm))
        bs = bg + 2 * abs(m) * bm + 4 * u * (g2 + m * m) + 3 * u * sd * sd       # the last term: the square root's rounding
        es = abs(sd * sd - s2)
        assert es <= bs, ("deviation", idx, float(es), float(bs))
        if bm:
            worst_m = max(worst_m, em / bm)
        if bs:
            worst_s = max(worst_s, es / bs)
    return float(worst_m), float(worst_s)


def niblack_from(m, s, k=0.2):
    return m - k * s


def sauvola_from(m, s, k=0.2, r=None, dtype=None):
    if r is None:
        lo, hi = exposure_ref.DTYPE_RANGE[np.dtype(dtype).name]
        r = 0.5 * (hi - lo)
    return m * (1 + k * ((s / r) - 1))


def niblack(image, window_size=15, k=0.2):
    m, s = mean_std_integral(image, window_size)
    return niblack_from(m, s, k)


def sauvola(image, window_size=15, k=0.2, r=None):
    m, s = mean_std_integral(image, window_size)
    return sauvola_from(m, s, k, r, np.asarray(image).dtype)


def local(image, block_size, method="gaussian", offset=0, mode="reflect", param=None, cval=0):
    if block_size % 2 == 0:
        raise ValueError("The kwarg ``block_size`` must be odd! Given ``block_size`` {0} is even.".format(block_size))
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("The parameter `image` must be a 2-dimensional array")
    out = np.zeros(image.shape, np.float64)
    if method == "generic":
        raise NotImplementedError("TODO: implement generic_filter")
    if method == "gaussian":
        sndi.gaussian_filter(image, (block_size - 1) / 6.0 if param is None else param, output=out, mode=mode, cval=cval)
    elif method == "mean":
        mask = 1.0 / block_size * np.ones((block_size,))
        sndi.convolve1d(image, mask, axis=0, output=out, mode=mode, cval=cval)
        sndi.convolve1d(out, mask, axis=1, output=out, mode=mode, cval=cval)
    elif method == "median":
        sndi.median_filter(image.astype(np.float64), block_size, output=out, mode=mode, cval=cval)
    else:
        raise ValueError("Invalid method specified. Please use `generic`, `gaussian`, `mean`, or `median`.")
    return out - offset


def try_all(image, **kw):
    raise NotImplementedError("needs matplotlib")


FUNCTIONS = {"threshold_otsu": otsu, "threshold_yen": yen, "threshold_isodata": isodata, "threshold_minimum": minimum,
             "threshold_mean": mean, "threshold_triangle": triangle, "threshold_li": li, "threshold_multiotsu": multiotsu,
             "threshold_niblack": niblack, "threshold_sauvola": sauvola, "threshold_local": local}


# ---------------------------------------------------------------- the known answers of tests/golden/threshold_kat.json
def kat_image(spec):
    """the host image of a case: literal data, or one of the recipes the reference's tests build their inputs with"""
    if "data" in spec:
        return np.array(_decode(spec["data"]), dtype=spec["dtype"])
    kind = spec["recipe"]
    if kind == "full":
        return np.full(spec["shape"], _decode(spec["value"]), dtype=spec["dtype"])
    if kind == "arange":
        return np.arange(spec["n"]).astype(spec["dtype"]).reshape(spec.get("shape", [spec["n"]]))       # wraps, as arange(n, dtype=uint8) did
    if kind == "linspace":
        return np.linspace(spec["start"], spec["stop"], spec["n"])
    if kind == "legacy_rand":
        return np.random.RandomState(spec["seed"]).rand(*spec["shape"])
    if kind == "rows":                                   # rows i0 .. i1 - 1 set to a value, on top of a base recipe
        img = kat_image(spec["base"])
        for i0, i1, v in spec["set_rows"]:
            img[i0:i1] = v
        return img
    if kind == "columns":
        img = kat_image(spec["base"])
        for j0, j1, v in spec["set_columns"]:
            img[:, j0:j1] = v
        return img
    if kind == "discs":                                  # skimage.draw.disk: the pixels strictly inside the circle
        img = np.zeros(spec["shape"], dtype=spec["dtype"])
        yy, xx = np.indices(spec["shape"])
        for (r, c), rad, v in zip(spec["centers"], spec["radii"], spec["values"]):
            img[(yy - r) ** 2 + (xx - c) ** 2 < rad ** 2] = v
        return img
    if kind == "scaled":
        return spec["factor"] * kat_image(spec["base"])
    raise ValueError(kind)


def _decode(v):
    """JSON has no inf / nan: they are written as strings"""
    if isinstance(v, list):
        return [_decode(e) for e in v]
    if isinstance(v, str):
        return float(v)
    return v


def check_expectation(expect, call, image):
    """`call()` runs the case and returns a host value (scalar or array); `expect` is the JSON entry"""
    kind = expect["kind"]
    if kind == "raises":
        try:
            call()
        except Exception as exc:
            assert type(exc).__name__ == expect["error"], (type(exc).__name__, expect["error"], exc)
            return
        raise AssertionError("no {} raised".format(expect["error"]))
    got = call()
    if kind == "equals":
        assert got == _decode(expect["value"]), (got, expect["value"])
    elif kind == "between":
        lo, hi = expect["low"], expect["high"]
        assert (lo <= got if expect.get("low_closed") else lo < got) and got < hi, (got, lo, hi)
    elif kind == "below":
        assert got < expect["value"], got
    elif kind == "isnan":
        assert np.isnan(got), got
    elif kind == "finite":
        assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), got
    elif kind == "no_nan":
        assert not np.any(np.isnan(np.asarray(got))), got
    elif kind == "array_equal":
        assert np.array_equal(np.asarray(got), np.asarray(expect["value"])), (got, expect["value"])
    elif kind == "array_almost_equal":
        np.testing.assert_array_almost_equal(np.asarray(got), np.asarray(expect["value"]))
    elif kind == "all_above":
        assert np.all(np.asarray(got) > expect["value"]), got
    elif kind == "length":
        assert len(got) == expect["value"], got
    elif kind == "mask_above":                           # image > result
        assert np.array_equal(image > np.asarray(got), np.asarray(expect["value"], dtype=bool)), (image > np.asarray(got))
    else:
        raise ValueError(kind)
