"""NumPy transcription of the match_template contract (cupyimg_amd/skimage/feature/_template.py, include/mi355img.h): the image
converted to float64 and padded by numpy.pad with the template's shape on every side, the windows by sliding_window_view, the
three sums, then the formula, every operation a float64 rounded on its own.

    window of output index o, per axis: starts at image index o - t // 2 (pad_input) or o, t the template's extent
    x = sum(I * T), s1 = sum(I), s2 = sum(I * I);  mean, V, ssd of the template from NumPy in float64
    num = x - s1 * mean;  d = s2 - (s1 * s1) / V;  d = d * ssd;  d = maximum(d, 0);  den = sqrt(d)
    r = num / den where den > finfo(float64).eps, else 0.0

`match_template` sums in NumPy's order, which equals any other order where the sums are exact (integer data below 2**53).
`match_template_longdouble` forms x, s1 and s2 in numpy.longdouble and returns, next to the result, what the error bound of
`error_bound` needs."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def template_stats(template):
    """(float64 template, mean, V, ssd) in the reference's operation order"""
    t = np.asarray(template).astype(np.float64)
    mean = t.mean()
    dev = t - mean
    dev *= dev
    return t, mean, t.size, np.sum(dev)


def windows(image, tshape, pad_input, mode, constant_values=0):
    """float64 view (output shape + template shape) of the window under every output"""
    img = np.asarray(image).astype(np.float64)
    width = tuple((t, t) for t in tshape)
    padded = np.pad(img, width, mode=mode, constant_values=constant_values) if mode == "constant" else np.pad(img, width, mode=mode)
    win = sliding_window_view(padded, tshape)
    index = []
    for n, t in zip(img.shape, tshape):
        # padded index of the first sample of output 0's window, and the number of outputs
        start, count = (t - t // 2, n) if pad_input else (t, n - t + 1)
        index.append(slice(start, start + count))
    return win[tuple(index)]


def _formula(x, s1, s2, mean, volume, ssd):
    num = x - s1 * mean
    d = s1 * s1
    d = d / volume
    d = s2 - d
    d = d * ssd
    with np.errstate(invalid="ignore"):
        d = np.maximum(d, 0)
        den = np.sqrt(d)
        mask = den > np.finfo(np.float64).eps
    r = np.zeros(np.shape(x), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r[mask] = (num[mask] / den[mask]).astype(np.float64)
    return r


def match_template(image, template, pad_input=False, mode="constant", constant_values=0):
    t, mean, volume, ssd = template_stats(template)
    win = windows(image, t.shape, pad_input, mode, constant_values)
    axes = tuple(range(-t.ndim, 0))
    with np.errstate(invalid="ignore", over="ignore"):
        x = (win * t).sum(axis=axes)
        s1 = win.sum(axis=axes)
        s2 = (win * win).sum(axis=axes)
        return _formula(x, s1, s2, mean, volume, ssd)


def match_template_longdouble(image, template, pad_input=False, mode="constant", constant_values=0):
    """(r, sums): the sums in numpy.longdouble and the formula on them in numpy.longdouble, with the float64 mean and ssd of
    the contract; sums = dict(x, s1, s2, abs_it = sum|I * T|, abs_i = sum|I|, mean, volume, ssd), float64 arrays and scalars
    (the long-double sums rounded once)"""
    t, mean, volume, ssd = template_stats(template)
    win = windows(image, t.shape, pad_input, mode, constant_values).astype(np.longdouble)
    tl = t.astype(np.longdouble)
    axes = tuple(range(-t.ndim, 0))
    x = (win * tl).sum(axis=axes)
    s1 = win.sum(axis=axes)
    s2 = (win * win).sum(axis=axes)
    abs_it = np.abs(win * tl).sum(axis=axes)
    abs_i = np.abs(win).sum(axis=axes)
    ld = np.longdouble
    num = x - s1 * ld(mean)
    d = (s2 - (s1 * s1) / ld(volume)) * ld(ssd)
    den = np.sqrt(np.maximum(d, 0))
    r = np.zeros(x.shape, np.float64)
    mask = den > np.finfo(np.float64).eps
    r[mask] = (num[mask] / den[mask]).astype(np.float64)
    f = lambda a: np.asarray(a, np.float64)
    return r, dict(x=f(x), s1=f(s1), s2=f(s2), abs_it=f(abs_it), abs_i=f(abs_i), mean=float(mean), volume=int(volume), ssd=float(ssd))


def conditioning(sums):
    """(s2 - s1^2 / V) / s2 per output: below 1e-3 the window variance is lost to cancellation"""
    return (sums["s2"] - sums["s1"] * sums["s1"] / sums["volume"]) / sums["s2"]


def error_bound(r, sums):
    """Per output, a first-order bound on |r_float64 - r_exact| for sums accumulated in float64 in ANY order and the formula
    evaluated in float64.  u = 2**-53; a sum of V products carries at most gamma = (V + 2) u relative to the
    sum of the magnitudes of its terms:

        dx = gamma sum|I T|,   ds1 = gamma sum|I|,   ds2 = gamma s2
        num = x - s1 mean:       dnum = dx + |mean| ds1 + 2 u (|x| + |s1 mean|)          (the product's and the difference's rounding)
        D = s2 - s1^2 / V:       dD = ds2 + 2 |s1| ds1 / V + u (s2 + 3 s1^2 / V)         (product, quotient, difference)
        den = sqrt(D ssd):       dden = den (dD / (2 D) + 2 u)                           (product u, square root u / 2 of its own, u / 2 passed on)
        r = num / den:           dr = dnum / den + |r| dden / den + u |r|"""
    u = 2.0 ** -53
    v = sums["volume"]
    gamma = (v + 2) * u
    x, s1, s2, mean = sums["x"], sums["s1"], sums["s2"], abs(sums["mean"])
    dx, ds1, ds2 = gamma * sums["abs_it"], gamma * sums["abs_i"], gamma * s2
    dnum = dx + mean * ds1 + 2 * u * (np.abs(x) + np.abs(s1) * mean)
    sq = s1 * s1 / v
    big_d = s2 - sq
    dd = ds2 + 2 * np.abs(s1) * ds1 / v + u * (s2 + 3 * sq)
    den = np.sqrt(big_d * sums["ssd"])
    dden = den * (dd / (2 * big_d) + 2 * u)
    return dnum / den + np.abs(r) * dden / den + u * np.abs(r)
