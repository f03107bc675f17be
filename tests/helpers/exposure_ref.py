"""Host transcription (NumPy) of the skimage.exposure arithmetic the device kernels implement, written from the equations in
include/mi355img.h above mi_clahe_maps (steps 1 .. 8), mi_interp_map and mi_rescale_intensity -- not from the reference's
source.  tests/test_exposure_yardstick.py checks it against NumPy and against the reference's own test vectors and
properties; tests/test_gpu_exposure.py compares the device with it bit for bit.

The CLAHE stages are callable one by one: to_gray14, region_histograms, clip_histogram, map_histogram, blend, finish."""
import itertools

import numpy as np

GRAY = 16384

_INT_NAMES = ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64")
DTYPE_RANGE = {n: (int(np.iinfo(n).min), int(np.iinfo(n).max)) for n in _INT_NAMES}
DTYPE_RANGE.update({"float16": (-1, 1), "float32": (-1, 1), "float64": (-1, 1), "float": (-1, 1), "bool": (0, 1),
                    "uint10": (0, 1023), "uint12": (0, 4095), "uint14": (0, 16383)})


# ---------------------------------------------------------------- test volumes
def volume(shape, dtype, seed=1, flat_corner=False):
    """A sum of sines plus noise on `shape`: uint8 in [10, 210], uint16 in [100, 4100] (12 bits on an offset, as a CT or MRI
    series is stored), floats in [-0.2, 1] (the negative part is what img_as_uint clips).  flat_corner: the block of the
    first half of every axis is set to the minimum (a background corner: histograms with one full bin)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    f = np.zeros(shape)
    for a, g in enumerate(grids):
        f += np.sin(g * (0.23 + 0.11 * a) + 0.7 * a)
    f += np.sin(sum(grids) * 0.09)
    f = (f - f.min()) / max(f.max() - f.min(), 1e-12)
    f = 0.85 * f + 0.15 * rng.random(shape)
    if flat_corner:
        f[tuple(slice(0, max(1, s // 2)) for s in shape)] = f.min()
    if dtype == np.uint8:
        return np.rint(10 + f * 200).astype(np.uint8)
    if dtype == np.uint16:
        return np.rint(100 + f * 4000).astype(np.uint16)
    return (f * 1.2 - 0.2).astype(dtype)


# ---------------------------------------------------------------- CLAHE, stage by stage
def as_uint(image):
    """step 1"""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image.astype(np.uint16) * np.uint16(257)
    if image.dtype == np.uint16:
        return image.copy()
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    if image.dtype.kind != "f":
        raise NotImplementedError(str(image.dtype))
    if image.min() < -1.0 or image.max() > 1.0:
        raise ValueError("Images of type float must be between -1 and 1.")
    t = image * image.dtype.type(65535)          # in the image dtype
    t = np.rint(t)
    t = np.clip(t, image.dtype.type(0), image.dtype.type(65535))
    return t.astype(np.uint16)


def to_gray14(image):
    """steps 1 and 2: uint16 grey levels 0 .. 16383"""
    u = as_uint(image)
    umin, umax = float(u.min()), float(u.max())
    x = u.astype(np.float64)
    if umin == umax:
        return np.minimum(u, 16383).astype(np.uint16)
    x = np.clip(x, umin, umax)
    x = (x - umin) / (umax - umin)
    x = x * 16383.0 + 0.0
    return np.rint(x).astype(np.uint16)


def bins_of(gray, nbins):
    """step 3"""
    return (gray // np.uint16(1 + GRAY // nbins)).astype(np.int64)


def _reflect(i, n):
    """numpy.pad(mode="reflect") index for i >= 0: period 2 (n - 1); an axis of length 1 repeats its sample"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    r = i % p
    return np.where(r < n, r, p - r)


def region_counts(shape, kernel):
    return [-(-s // k) for s, k in zip(shape, kernel)]


def region_histograms(b, kernel, nbins):
    """step 4: int64 array (regions_0, ..., regions_(n-1), nbins)"""
    nd = b.ndim
    nr = region_counts(b.shape, kernel)
    idx = [_reflect(np.arange(n * k), s) for n, k, s in zip(nr, kernel, b.shape)]
    ext = b[np.ix_(*idx)]
    split = []
    for n, k in zip(nr, kernel):
        split += [n, k]
    ext = ext.reshape(split).transpose(tuple(range(0, 2 * nd, 2)) + tuple(range(1, 2 * nd, 2)))
    flat = ext.reshape(int(np.prod(nr)), -1)
    hist = np.stack([np.bincount(row, minlength=nbins) for row in flat]).astype(np.int64)
    assert hist.shape[1] == nbins
    return hist.reshape(tuple(nr) + (nbins,))


def clip_limit_voxels(clip_limit, kernel):
    npix = int(np.prod(kernel, dtype=object))
    return int(max(clip_limit * npix, 1)) if clip_limit > 0.0 else npix


def clip_histogram(hist, c, stats=None):
    """step 5 on one histogram (int64 vector, not modified).  stats (a dict): 'entered' = the strided loop was entered,
    'passes' = strided passes that ran, 'rounds', 'overshoot' = E ended below 0, 'idle' = left by a round that changed
    nothing."""
    h = np.array(hist, dtype=np.int64)
    nbins = h.size
    over = h > c
    E = int((h[over] - c).sum())
    h[over] = c
    incr = E // nbins
    upper = c - incr
    low = h < upper
    E -= int(low.sum()) * incr
    h[low] += incr
    mid = (h >= upper) & (h < c)
    E -= int((c - h[mid]).sum())
    h[mid] = c
    st = {"entered": E > 0, "passes": 0, "rounds": 0, "overshoot": False, "idle": False}
    while E > 0:
        E0 = E
        st["rounds"] += 1
        for index in range(nbins):
            under = h < c
            step = max(1, int(under.sum()) // E)
            sel = np.arange(index, nbins, step)
            sel = sel[under[sel]]
            h[sel] += 1
            E -= sel.size
            st["passes"] += 1
            if E <= 0:
                break
        if E == E0:
            st["idle"] = True
            break
    st["overshoot"] = E < 0
    if stats is not None:
        stats.update(st)
    return h


def map_histogram(hist, npix):
    """step 6 along the last axis: int64"""
    m = np.cumsum(hist, axis=-1).astype(np.float64)
    m = m * (16383 / npix)
    m = m + 0.0
    m = np.minimum(m, 16383.0)
    return m.astype(np.int64)


def blend(b, maps, kernel):
    """step 7: b int64 bins of the image's shape, maps (regions_0, ..., nbins) -> uint16"""
    nd = b.ndim
    nr = maps.shape[:nd]
    cell, coef = [], []
    for a in range(nd):
        p = np.arange(b.shape[a]) + kernel[a] // 2
        shp = [1] * nd
        shp[a] = -1
        cell.append((p // kernel[a]).reshape(shp))
        coef.append(((p % kernel[a]) / float(kernel[a])).reshape(shp))
    acc = np.zeros(b.shape, np.float32)
    for e in itertools.product((0, 1), repeat=nd):
        regs = tuple(np.clip(cell[a] - 1 + e[a], 0, nr[a] - 1) for a in range(nd))
        w = None
        for a in range(nd - 1, -1, -1):
            f = coef[a] if e[a] else 1.0 - coef[a]
            w = f if w is None else w * f
        mapped = maps[regs + (b,)].astype(np.float64)
        acc = acc + (mapped * w).astype(np.float32)
    return acc.astype(np.uint16)


def finish(v):
    """step 8"""
    f = v.astype(np.float64) * (1.0 / 65535)
    lo, hi = float(f.min()), float(f.max())
    if lo == hi:
        return f
    f = (f - lo) / (hi - lo)
    return f * 1.0 + 0.0


def kernel_of(shape, kernel_size):
    if kernel_size is None:
        return [s // 8 for s in shape]
    if np.ndim(kernel_size) == 0:
        return [int(kernel_size)] * len(shape)
    assert len(kernel_size) == len(shape)
    return [int(k) for k in kernel_size]


def clahe_maps(image, kernel_size=None, clip_limit=0.01, nbins=256, stats=None):
    """steps 1 .. 6: (bins b, maps (regions..., nbins) int64); stats: a list that receives one dict per region"""
    image = np.asarray(image)
    kernel = kernel_of(image.shape, kernel_size)
    b = bins_of(to_gray14(image), nbins)
    hist = region_histograms(b, kernel, nbins)
    c = clip_limit_voxels(clip_limit, kernel)
    flat = hist.reshape(-1, nbins)
    out = np.empty_like(flat)
    for r in range(flat.shape[0]):
        st = {}
        out[r] = clip_histogram(flat[r], c, st)
        if stats is not None:
            stats.append(st)
    return b, map_histogram(out.reshape(hist.shape), int(np.prod(kernel)))


def equalize_adapthist(image, kernel_size=None, clip_limit=0.01, nbins=256):
    image = np.asarray(image)
    b, maps = clahe_maps(image, kernel_size, clip_limit, nbins)
    return finish(blend(b, maps, kernel_of(image.shape, kernel_size)))


# ---------------------------------------------------------------- histogram, cdf, equalize_hist
def _float_edges(a, nbins, rng):
    if rng is None:
        first, last = a.min(), a.max()
    else:
        first, last = rng
    if first == last:
        first, last = first - 0.5, last + 0.5
    return np.linspace(first, last, nbins + 1, endpoint=True, dtype=a.dtype if a.dtype.kind == "f" else np.float64)


def histogram(image, nbins=256, source_range="image", normalize=False):
    """(hist, bin_centers): integers one bin per value from the image's minimum (or the dtype's) to its maximum, floats as
    numpy.histogram(image, nbins, range) with bins [e_k, e_(k+1)), the last one closed, against explicit edges; bool images
    (no integers to numpy.issubdtype) as floats too: their values as uint8, float64 edges, the range (0, 1) for "dtype"."""
    a = np.asarray(image).reshape(-1)
    if a.dtype == np.float16:
        a = a.astype(np.float32)
    dtype_range = (-1, 1)
    if a.dtype.kind == "b":
        a = a.astype(np.uint8)
        dtype_range = (0, 1)
    elif a.dtype.kind in "iu":
        dtype_range = None
    if dtype_range is None:
        if source_range == "image":
            lo, hi = int(a.min()), int(a.max())
        else:
            lo, hi = DTYPE_RANGE[a.dtype.name]
        hist = np.zeros(hi - lo + 1, np.int64)
        vals, cnt = np.unique(a, return_counts=True)
        hist[(vals.astype(object) - lo).astype(np.int64)] = cnt
        centers = np.arange(lo, hi + 1)
    else:
        edges = _float_edges(a, nbins, None if source_range == "image" else dtype_range)
        e = edges.astype(np.float64)
        x = a.astype(np.float64)
        x = x[(x >= e[0]) & (x <= e[-1])]
        k = np.searchsorted(e, x, side="right") - 1
        k[x == e[-1]] = nbins - 1
        hist = np.bincount(k, minlength=nbins).astype(np.int64)
        centers = (edges[:-1] + edges[1:]) / 2.0
    if normalize:
        hist = hist / np.sum(hist)
    return hist, centers


def cumulative_distribution(image, nbins=256):
    hist, centers = histogram(image, nbins)
    cdf = hist.cumsum()
    return cdf / float(cdf[-1]), centers


def interp(x, xp, fp):
    """numpy.interp written out: j = the last knot at or below x, fp[j] + slope * (x - xp[j]), ends clamped"""
    x = np.asarray(x, dtype=np.float64)
    xp = np.asarray(xp, dtype=np.float64)
    fp = np.asarray(fp, dtype=np.float64)
    n = xp.size
    if n == 1:
        return np.full(x.shape, fp[0])
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 2)
    with np.errstate(all="ignore"):
        slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
        r = slope * (x - xp[j]) + fp[j]
    r = np.where(x == xp[j], fp[j], r)
    r = np.where(x >= xp[-1], fp[-1], r)
    r = np.where(x <= xp[0], fp[0], r)
    return r


def equalize_hist(image, nbins=256, mask=None):
    image = np.asarray(image)
    src = image if mask is None else image[np.asarray(mask, dtype=bool)]
    cdf, centers = cumulative_distribution(src, nbins)
    return interp(image.reshape(-1), centers, cdf).reshape(image.shape)


# ---------------------------------------------------------------- rescale_intensity
def _range(image, value, clip_negative=False):
    if isinstance(value, str) and value == "dtype":
        value = image.dtype.name
    if isinstance(value, str) and value == "image":
        return image.min().item(), image.max().item()
    if isinstance(value, (type, np.dtype)):
        value = np.dtype(value).name
    if isinstance(value, str):
        lo, hi = DTYPE_RANGE[value]
        return (0 if clip_negative else lo), hi
    return tuple(value)


def rescale_intensity(image, in_range="image", out_range="dtype"):
    image = np.asarray(image)
    if isinstance(out_range, str) and out_range in ("dtype", "image"):
        out_dtype = image.dtype
    elif isinstance(out_range, (str, type, np.dtype)):
        name = out_range if isinstance(out_range, str) else np.dtype(out_range).name
        out_dtype = np.dtype(np.uint16 if name in ("uint10", "uint12", "uint14") else ("float64" if name == "float" else name))
    else:
        out_dtype = np.dtype(np.float64)
    imin, imax = map(float, _range(image, in_range))
    omin, omax = map(float, _range(image, out_range, clip_negative=(imin >= 0)))
    F = np.float32 if image.dtype == np.float32 else np.float64
    x = image.astype(F)
    x = np.clip(x, F(imin), F(imax))
    with np.errstate(all="ignore"):
        if imin != imax:
            x = (x - F(imin)) / F(imax - imin)
            x = x * F(omax - omin)
            x = x + F(omin)
        else:
            x = np.clip(x, F(omin), F(omax))
        if out_dtype.kind in "iu":
            return np.trunc(x.astype(np.float64)).astype(np.int64).astype(out_dtype)
        return x.astype(out_dtype)


# ---------------------------------------------------------------- the histogram vectors of tests/golden/exposure_kat.json
def check_histogram_case(case, hist, centers):
    start, stop, offset = case["centers_arange"]
    assert len(hist) == len(centers) == case["length"]
    np.testing.assert_array_equal(centers, np.arange(start, stop) + offset)
    listed = np.zeros(len(hist), bool)
    for k, v in case["counts"].items():
        assert hist[int(k)] == v
        listed[int(k)] = True
    if case["others_zero"]:
        assert not np.any(hist[~listed])
