"""Host transcription (NumPy / SciPy) of the edge family: skimage.filters' edge operators (cupyimg/skimage/filters/edges.py),
apply_hysteresis_threshold (filters/thresholding.py:1182-1227) and feature.canny (feature/_canny.py), operation by operation in
the reference's order, so that the device results can be compared bit for bit.  Written from the reference's arithmetic; the
deliberate differences are the ones the library documents: cval is honoured, float16 is computed in float32, the threshold
comparisons are made in float64, and the Canny magnitude is sqrt(a * a + b * b) (each operation rounded on its own) where the
reference calls hypot (`magnitude_fn` switches that back for the yardstick)."""
import math

import numpy as np
from scipy import ndimage as ndi

SOBEL_SMOOTH = np.array([1, 2, 1]) / 4
SCHARR_SMOOTH = np.array([3, 10, 3]) / 16
PREWITT_SMOOTH = np.full((3,), 1 / 3)
SMOOTH = {"sobel": SOBEL_SMOOTH, "scharr": SCHARR_SMOOTH, "prewitt": PREWITT_SMOOTH}
ROBERTS_PD = np.array([[1, 0], [0, -1]], dtype=np.double)
ROBERTS_ND = np.array([[0, 1], [-1, 0]], dtype=np.double)
_P = np.array([[0.0376593171958126, 0.249153396177344, 0.426374573253687, 0.249153396177344, 0.0376593171958126]])
_D1 = np.asarray([[0.109603762960254, 0.276690988455557, 0, -0.276690988455557, -0.109603762960254]])
HFARID = _D1.T * _P
VFARID = np.copy(HFARID.T)

_INT_RANGE = {np.dtype(t): (np.iinfo(t).min, np.iinfo(t).max) for t in (np.uint8, np.uint16, np.uint32, np.int8, np.int16, np.int32)}


def img_as_float(image):
    """skimage.img_as_float: floats pass (float16 -> float32, the library's convention), bool -> {0, 1}, unsigned integers
    x * (1 / max), signed (2 x + 1) / (max - min) as x * (2 / (max - min)) + 1 / (max - min) with one rounding"""
    image = np.asarray(image)
    dt = image.dtype
    if dt == np.float16:
        return image.astype(np.float32)
    if dt.kind == "f":
        return image
    if dt == np.bool_:
        return image.astype(np.float64)
    lo, hi = _INT_RANGE[dt]
    x = image.astype(np.float64)
    if dt.kind == "u":
        return x * (1.0 / hi)
    # one fused multiply-add (a single rounding), evaluated exactly per distinct sample value
    from fractions import Fraction
    p0, p1 = Fraction(2.0 / (hi - lo)), Fraction(1.0 / (hi - lo))
    values, inverse = np.unique(image, return_inverse=True)
    table = np.array([float(Fraction(int(v)) * p0 + p1) for v in values], dtype=np.float64)
    return table[inverse].reshape(image.shape)


def edge_kernel(ndim, edge_dim, smooth_weights, edge_weights=np.array([1, 0, -1])):
    """The dense kernel of one edge axis: the edge weights along `edge_dim`, times (in double, lowest axis first) the
    smoothing weights along every axis that is not `edge_dim` as given -- so a negative `edge_dim` is smoothed along the
    edge axis too, which is what the reference computes."""
    def along(weights, axis):
        return np.asarray(weights).reshape([3 if a == axis % ndim else 1 for a in range(ndim)])

    kernel = along(edge_weights, edge_dim)
    for axis in range(ndim):
        if axis != edge_dim:
            kernel = kernel * along(smooth_weights, axis)
    return kernel


def laplace_operator(ndim):
    """3^ndim zeros, 2 ndim at the centre, -1 at the centre's axis neighbours"""
    op = np.zeros((3,) * ndim)
    for index in np.ndindex(*op.shape):
        off_centre = [a for a in range(ndim) if index[a] != 1]
        if not off_centre:
            op[index] = 2.0 * ndim
        elif len(off_centre) == 1:
            op[index] = -1.0
    return op


def mask_filter_result(result, mask):
    """the result times the mask eroded with the full-connectivity structure (border value 0), as a multiplication in place"""
    if mask is None:
        return result
    mask = np.asarray(mask)
    eroded = ndi.binary_erosion(mask, ndi.generate_binary_structure(mask.ndim, mask.ndim), border_value=0)
    with np.errstate(invalid="ignore"):
        np.multiply(result, eroded, out=result)
    return result


def generic_edge_filter(image, smooth_weights, axis=None, mode="reflect", cval=0.0):
    """Per edge axis scipy.ndimage.convolve with the dense kernel, in the image dtype; a float64 accumulator that starts at
    0.0 takes the responses (one axis) or their squares (several: squared in the image dtype, then the sum is divided by
    the rank and rooted)."""
    axes = list(range(image.ndim)) if axis is None else ([axis] if np.isscalar(axis) else list(axis))
    total = np.zeros(image.shape, np.float64)
    with np.errstate(all="ignore"):
        for a in axes:
            response = ndi.convolve(image, edge_kernel(image.ndim, a, smooth_weights), mode=mode, cval=cval)
            total += response * response if len(axes) > 1 else response
        if len(axes) > 1:
            total /= image.ndim
            np.sqrt(total, out=total)
    return total


def edge(name, image, mask=None, *, axis=None, mode="reflect", cval=0.0):
    """sobel / scharr / prewitt"""
    if not isinstance(mode, str):
        mode = list(mode)[0]
    image = img_as_float(image)
    return mask_filter_result(generic_edge_filter(image, SMOOTH[name], axis, mode, cval), mask)


def convolve_masked(image, weights, mask=None):
    with np.errstate(all="ignore"):
        return mask_filter_result(ndi.convolve(img_as_float(image), weights), mask)


def pair_magnitude(a, b):
    """sqrt(a^2 + b^2) / sqrt(2) in the arrays' dtype, every operation rounded on its own, the division last"""
    with np.errstate(all="ignore"):
        out = np.sqrt(b * b + a * a)
        out /= math.sqrt(2)
    return out


def roberts_pos_diag(image, mask=None):
    return convolve_masked(image, ROBERTS_PD, mask)


def roberts_neg_diag(image, mask=None):
    return convolve_masked(image, ROBERTS_ND, mask)


def roberts(image, mask=None):
    return pair_magnitude(roberts_pos_diag(image, mask), roberts_neg_diag(image, mask))


def farid_h(image, mask=None):
    return convolve_masked(image, HFARID, mask)


def farid_v(image, mask=None):
    return convolve_masked(image, VFARID, mask)


def farid(image, mask=None):
    return pair_magnitude(farid_h(image, mask), farid_v(image, mask))


def laplace(image, ksize=3, mask=None):
    image = img_as_float(image)
    with np.errstate(all="ignore"):
        return mask_filter_result(ndi.convolve(image, laplace_operator(image.ndim)), mask)


# ------------------------------------------------------------------ hysteresis
def threshold_masks(image, low, high):
    """thresholding.py:1218-1220 with the comparisons in float64"""
    image = np.asarray(image).astype(np.float64)
    low = np.clip(np.asarray(low, dtype=np.float64), a_min=None, a_max=np.asarray(high, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return image > low, image > np.asarray(high, dtype=np.float64)


def hysteresis_by_labels(mask_low, mask_high, structure=None):
    """the components of mask_low (connectivity 1 unless a structure is given) that hold a sample of mask_high"""
    labels, _ = ndi.label(mask_low, structure)
    keep = np.unique(labels[np.asarray(mask_high, bool) & (labels > 0)])
    return np.isin(labels, keep) & (labels > 0)


def hysteresis_by_propagation(mask_low, mask_high, structure=None):
    if structure is None:
        structure = ndi.generate_binary_structure(mask_low.ndim, 1)
    return ndi.binary_propagation(mask_high, structure=structure, mask=mask_low)


def apply_hysteresis_threshold(image, low, high):
    mask_low, mask_high = threshold_masks(image, low, high)
    return hysteresis_by_labels(mask_low, mask_high)


# ------------------------------------------------------------------ canny
def plain_magnitude(isobel, jsobel):
    """sqrt(a * a + b * b), every operation rounded on its own: the library's definition"""
    with np.errstate(all="ignore"):
        return np.sqrt(isobel * isobel + jsobel * jsobel)


def dtype_max(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f" or dtype == np.bool_:
        return 1
    return np.iinfo(dtype).max


def gaussian(image, sigma, mode="constant"):
    """filters.gaussian: img_as_float first, then ndi.gaussian_filter in that dtype"""
    return ndi.gaussian_filter(img_as_float(image), sigma, mode=mode, cval=0)


def canny_smooth(image, mask, sigma):
    """Gaussian smoothing that ignores masked pixels: the smoothed masked image (a copy of the image under the mask, zero
    elsewhere) over the smoothed mask plus eps; float64, because the smoothed mask is"""
    weight = gaussian(mask.astype(np.float64), sigma)
    inside = np.where(mask, image, np.zeros((), image.dtype))
    return gaussian(inside, sigma) / (weight + np.finfo(np.float64).eps)


def _shifted(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx]; NaN where that lies outside (never consulted: the eroded mask clears the border ring)"""
    out = np.full(a.shape, np.nan)
    ny, nx = a.shape
    ys, xs = slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx))
    yd, xd = slice(max(0, dy), ny + min(0, dy)), slice(max(0, dx), nx + min(0, dx))
    out[ys, xs] = a[yd, xd]
    return out


# The four direction classes in the order the reference evaluates them (a later class overwrites an earlier one where the
# predicates overlap): (same sign of the two responses?, |isobel| dominant?, the two neighbours (dy, dx) towards "plus":
# the diagonal one (weight w) and the axial one (weight 1 - w)); the "minus" neighbours are the mirrored ones.
CANNY_CLASSES = [(True, True, (1, 1), (1, 0)), (True, False, (1, 1), (0, 1)),
                 (False, False, (-1, 1), (0, 1)), (False, True, (-1, 1), (-1, 0))]


def canny_stage(smoothed, mask, magnitude_fn=plain_magnitude, ties=None):
    """Sobel responses, magnitude and non-maximum suppression -> (isobel, jsobel, magnitude, local_maxima), written on
    shifted whole arrays.  A pixel of the eroded mask with magnitude m > 0 is a local maximum if, for the last class it
    belongs to, both interpolated neighbours `diag * w + axial * (1 - w)` are <= m, with w = smaller |response| / larger.
    `ties` (a list) collects how many of those comparisons were exact ties among the pixels of each class."""
    isobel = ndi.sobel(smoothed, axis=0)
    jsobel = ndi.sobel(smoothed, axis=1)
    ai, aj = np.abs(isobel), np.abs(jsobel)
    magnitude = magnitude_fn(isobel, jsobel)
    gate = ndi.binary_erosion(mask, np.ones((3, 3), bool), border_value=0) & (magnitude > 0)
    same = ((isobel >= 0) & (jsobel >= 0)) | ((isobel <= 0) & (jsobel <= 0))
    opposite = ((isobel <= 0) & (jsobel >= 0)) | ((isobel >= 0) & (jsobel <= 0))
    local_maxima = np.zeros(smoothed.shape, bool)
    with np.errstate(all="ignore"):
        for same_sign, i_dominant, diag, axial in CANNY_CLASSES:
            member = gate & (same if same_sign else opposite) & (ai >= aj if i_dominant else ai <= aj)
            w = aj / ai if i_dominant else ai / aj
            passed = np.ones(smoothed.shape, bool)
            for sign in (1, -1):
                value = _shifted(magnitude, sign * diag[0], sign * diag[1]) * w + _shifted(magnitude, sign * axial[0], sign * axial[1]) * (1 - w)
                if ties is not None:
                    ties.append(int(np.count_nonzero((value == magnitude) & member)))
                passed &= value <= magnitude
            local_maxima = np.where(member, passed, local_maxima)
    return isobel, jsobel, magnitude, local_maxima


def canny_thresholds(image_dtype, low_threshold, high_threshold, use_quantiles):
    """(low, high): defaults 0.1 / 0.2, quantiles checked to lie in [0, 1], absolute values divided by the dtype's maximum"""
    out = []
    for given, default in ((low_threshold, 0.1), (high_threshold, 0.2)):
        if given is None:
            out.append(default)
        elif not use_quantiles:
            out.append(given / dtype_max(image_dtype))
        elif 0.0 <= given <= 1.0:
            out.append(given)
        else:
            raise ValueError("quantile out of [0, 1]")
    return tuple(out)


def canny(image, sigma=1.0, low_threshold=None, high_threshold=None, mask=None, use_quantiles=False,
          magnitude_fn=plain_magnitude, detail=None):
    """The whole detector.  `detail` (a dict) receives the intermediate arrays and the thresholds."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("2-D images only")
    low, high = canny_thresholds(image.dtype, low_threshold, high_threshold, use_quantiles)
    if image.dtype == np.float16:
        image = image.astype(np.float32)
    mask = np.ones(image.shape, bool) if mask is None else np.asarray(mask).astype(bool)
    smoothed = canny_smooth(image, mask, sigma)
    ties = []
    isobel, jsobel, magnitude, local_maxima = canny_stage(smoothed, mask, magnitude_fn, ties)
    if use_quantiles:
        high, low = (np.percentile(magnitude, 100.0 * q) for q in (high, low))
    high_mask = local_maxima & (magnitude >= high)
    low_mask = local_maxima & (magnitude >= low)
    if detail is not None:
        detail.update(smoothed=smoothed, isobel=isobel, jsobel=jsobel, magnitude=magnitude, local_maxima=local_maxima,
                      high_mask=high_mask, low_mask=low_mask, high=float(high), low=float(low), ties=ties)
    return hysteresis_by_labels(low_mask, high_mask, np.ones((3, 3), bool))


# ------------------------------------------------------------------ test images
def circle_image(noisy, seed=0):
    """The ring of the reference's circle cases (test_canny.py:27-70): 400 x 400 pixels with coordinates -1 .. 1 (step 1 / 200),
    1 where the distance from the centre is within 0.02 of 0.5; `noisy`: half the ring plus half uniform noise (NumPy's
    generator; the reference draws on the device) -> (image, ring)"""
    axis = (np.arange(400) - 200.0) / 200
    radius = np.sqrt(axis[:, None] ** 2 + axis[None, :] ** 2)
    ring = np.abs(radius - 0.5) < 0.02
    image = ring.astype(float)
    if noisy:
        image = image * 0.5 + np.random.RandomState(seed).uniform(size=ring.shape) * 0.5
    return image, ring


def ring_band(ring, iterations):
    """where edges of the ring may lie: within `iterations` pixels of its inner and outer outline"""
    return ndi.binary_dilation(ring, iterations=iterations) & ~ndi.binary_erosion(ring, iterations=iterations)


def noise_image(shape, seed):
    return np.random.RandomState(seed).uniform(size=shape)


def _as_dtype(image, dtype):
    if np.dtype(dtype).kind == "f":
        return image.astype(dtype)
    return np.round(image * np.iinfo(dtype).max).astype(dtype)


def canny_cases():
    """(id, image, keyword arguments) of every whole-call Canny case the device tests run and the yardstick admits: the
    reference's two ring cases, two white-noise images, each as float64, float32 and uint8; masked and quantile variants"""
    ring, _ = circle_image(False)
    noisy, _ = circle_image(True)
    ones = np.ones(ring.shape, bool)
    base = [("ring", ring, dict(sigma=4, low_threshold=0, high_threshold=0, mask=ones)),
            ("noisy_ring", noisy, dict(sigma=4, low_threshold=0.1, high_threshold=0.2, mask=ones)),
            ("noise_64x70", noise_image((64, 70), 3), dict(sigma=1.0)),
            ("noise_37x131", noise_image((37, 131), 4), dict(sigma=1.4))]
    cases = []
    for name, image, kw in base:
        for dtype in ("float64", "float32", "uint8"):
            kw2 = dict(kw)
            if dtype == "uint8" and kw2.get("high_threshold"):
                kw2["low_threshold"] = kw2["low_threshold"] * 255
                kw2["high_threshold"] = kw2["high_threshold"] * 255
            cases.append(("{}-{}".format(name, dtype), _as_dtype(image, dtype), kw2))
    rng = np.random.RandomState(5)
    for name, image, kw in base[2:]:
        mask = rng.uniform(size=image.shape) > 0.08
        mask[:3, :5] = False
        cases.append((name + "-masked", image, dict(kw, mask=mask)))
        cases.append((name + "-masked-float32", image.astype(np.float32), dict(kw, mask=mask)))
        cases.append((name + "-quantiles", image, dict(kw, low_threshold=0.6, high_threshold=0.8, use_quantiles=True)))
        cases.append((name + "-quantiles-uint8", _as_dtype(image, "uint8"), dict(kw, low_threshold=0.55, high_threshold=0.9, use_quantiles=True)))
    return cases


def percentile_plan(n, q):
    """the two order statistics and the weight of numpy.percentile(a, q), linear interpolation, on n samples"""
    virtual = (n - 1) * np.true_divide(q, 100)
    if virtual >= n - 1:
        return n - 1, n - 1, 0.0
    previous = int(np.floor(virtual))
    return previous, previous + 1, float(virtual - previous)
