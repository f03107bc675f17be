"""Host transcription (NumPy / SciPy) of skimage.feature.structure_tensor and the corner detectors built on it
(cupyimg/skimage/feature/corner.py:18-138, 533-830), operation by operation in the reference's order and dtypes, so that the
device results can be compared bit for bit.  This file is the arithmetic contract of csrc/corners.hip:

  * the derivative along axis a is scipy.ndimage.sobel(image, axis=a, mode=mode, cval=cval) itself;
  * `sobel_by_passes` and `sobel_by_registers` restate that arithmetic in NumPy the two ways the device evaluates it (one 3-tap
    pass per launch; all passes from the 3^rank samples around a voxel), and tests/test_corners_yardstick.py holds both to
    SciPy's bits;
  * the products are formed in the image dtype, the Gaussian is a plug-in (SciPy's by default; the device tests plug in the
    library's own filter), the responses follow corner.py:566-590, 658-671, 728-743, 812-830 literally.

The deliberate differences from the reference are the library's: float16 is computed in float32, and corner_kitchen_rosenfeld
converts integer images like the other detectors (the reference lets them wrap inside ndi.sobel)."""
from itertools import combinations_with_replacement

import numpy as np
from scipy import ndimage as ndi

from helpers.edges_ref import img_as_float

# the library's mode names as SciPy's filters understand them (all eight exist there)
MODES = ["reflect", "constant", "nearest", "mirror", "wrap", "grid-wrap", "grid-constant", "grid-mirror"]


def _index_map(i, n, mode):
    """the position inside an axis of length n that index i (at most one axis length outside) stands for; -1: cval"""
    if 0 <= i < n:
        return i
    if mode in ("constant", "grid-constant"):
        return -1
    if mode == "nearest":
        return 0 if i < 0 else n - 1
    if mode in ("wrap", "grid-wrap"):
        return i % n
    if mode in ("reflect", "grid-mirror"):
        i = -1 - i if i < 0 else i
        i %= 2 * n
        return min(i, 2 * n - 1 - i)
    if mode == "mirror":
        if n == 1:
            return 0
        i = abs(i)
        i = 1 + (i - 1) % (2 * n - 2) if i > 0 else 0
        return min(i, 2 * n - 2 - i)
    raise ValueError(mode)


def _diff(xm, x0, xp, dtype):
    """correlate1d with [-1, 0, 1] in SciPy's antisymmetric form: a double accumulator, the centre tap first"""
    with np.errstate(all="ignore"):
        t = x0.astype(np.float64) * 0.0
        t = t + (xm.astype(np.float64) - xp.astype(np.float64)) * -1.0
        return t.astype(dtype)


def _smooth(xm, x0, xp, dtype):
    """correlate1d with [1, 2, 1] in SciPy's symmetric form"""
    with np.errstate(all="ignore"):
        t = x0.astype(np.float64) * 2.0
        t = t + (xm.astype(np.float64) + xp.astype(np.float64)) * 1.0
        return t.astype(dtype)


def _pass(x, axis, anti, mode, cval):
    """one 3-tap pass along `axis`: the line extended by one sample either way (the mode's index map, or the double cval)"""
    n = x.shape[axis]
    def neighbour(step):
        out = np.empty(x.shape, np.float64)
        for l in range(n):
            src = _index_map(l + step, n, mode)
            dst = tuple(slice(l, l + 1) if a == axis else slice(None) for a in range(x.ndim))
            if src < 0:
                out[dst] = cval
            else:
                out[dst] = x[tuple(slice(src, src + 1) if a == axis else slice(None) for a in range(x.ndim))]
        return out
    return (_diff if anti else _smooth)(neighbour(-1), x, neighbour(1), x.dtype)


def _pass_axes(ndim, axis):
    return [axis] + [b for b in range(ndim) if b != axis]


def sobel_by_passes(image, axis, mode="reflect", cval=0.0):
    """the generic route: one pass per axis, each rounded to the image dtype"""
    out = image
    for k, b in enumerate(_pass_axes(image.ndim, axis)):
        out = _pass(out, b, k == 0, mode, cval)
    return out


def neighbourhood(image, mode):
    """W[k_0, .., k_{r-1}, q] = the sample at q + k - 1 with every coordinate mapped on its own (0 where 'constant' has none:
    never used), and per axis the flags "the lower / upper neighbour lies outside the array" """
    rank = image.ndim
    w = np.zeros((3,) * rank + image.shape, image.dtype)
    for k in np.ndindex(*(3,) * rank):
        maps = [np.array([_index_map(l + k[a] - 1, image.shape[a], mode) for l in range(image.shape[a])]) for a in range(rank)]
        valid = np.ones(image.shape, bool)
        for a in range(rank):
            valid &= (maps[a] >= 0).reshape([-1 if b == a else 1 for b in range(rank)])
        gathered = image[np.ix_(*[np.maximum(m, 0) for m in maps])]
        w[k] = np.where(valid, gathered, np.zeros((), image.dtype))
    return w


def sobel_by_registers(image, axis, mode="reflect", cval=0.0, w=None):
    """the fused route: every pass from the 3^rank samples around a voxel; a pass along b folds the neighbourhood's axis b, and
    for 'constant' its outer operands are replaced by cval where the voxel's neighbour along b lies outside the array"""
    rank = image.ndim
    w = neighbourhood(image, mode) if w is None else w
    constant = mode in ("constant", "grid-constant")
    live = list(range(rank))                       # neighbourhood axes still present, in order
    for k, b in enumerate(_pass_axes(rank, axis)):
        pos = live.index(b)
        lower, centre, upper = (np.take(w, j, axis=pos).astype(np.float64) for j in range(3))
        if constant:
            coord = np.arange(image.shape[b]).reshape([-1 if a == b else 1 for a in range(rank)])
            lower = np.where(coord == 0, cval, lower)
            upper = np.where(coord == image.shape[b] - 1, cval, upper)
        w = (_diff if k == 0 else _smooth)(lower, centre, upper, image.dtype)
        live.remove(b)
    return w


def derivatives(image, mode="constant", cval=0):
    """corner.py:18-43 on an image that is already floating point"""
    with np.errstate(all="ignore"):
        return [ndi.sobel(image, axis=a, mode=mode, cval=cval) for a in range(image.ndim)]


def products(derivs, order="rc"):
    if order == "xy":
        derivs = list(reversed(derivs))
    with np.errstate(all="ignore"):
        return [d0 * d1 for d0, d1 in combinations_with_replacement(derivs, 2)]


def prepare(image):
    """the library's input conversion: img_as_float, float16 computed in float32"""
    return np.ascontiguousarray(img_as_float(np.asarray(image)))


def structure_products(image, mode="constant", cval=0, order="rc"):
    image = prepare(image)
    return products(derivatives(image, mode, cval), order)


def structure_tensor(image, sigma=1, mode="constant", cval=0, order="rc", gaussian=None):
    """corner.py:125-138; `gaussian(product, sigma, mode=, cval=)` defaults to SciPy's filter"""
    if gaussian is None:
        gaussian = ndi.gaussian_filter
    return [gaussian(p, sigma, mode=mode, cval=cval) for p in structure_products(image, mode, cval, order)]


def corner_harris(Arr, Arc, Acc, method="k", k=0.05, eps=1e-6):
    """corner.py:660-671 on the tensor's elements"""
    with np.errstate(all="ignore"):
        detA = Arr * Acc
        detA -= Arc * Arc
        traceA = Arr + Acc
        if method == "k":
            response = detA - k * traceA * traceA
        else:
            response = 2 * detA / (traceA + eps)
    return response


def corner_shi_tomasi(Arr, Arc, Acc):
    """corner.py:733-743"""
    with np.errstate(all="ignore"):
        tmp = Arr - Acc
        tmp *= tmp
        tmp2 = 4 * Arc
        tmp2 *= Arc
        tmp += tmp2
        np.sqrt(tmp, out=tmp)
        tmp /= 2
        response = Arr + Acc
        response -= tmp
    return response


def corner_foerstner(Arr, Arc, Acc):
    """corner.py:814-830"""
    with np.errstate(all="ignore"):
        detA = Arr * Acc
        detA -= Arc * Arc
        traceA = Arr + Acc
        w = np.zeros_like(Arr, dtype=np.double)
        q = np.zeros_like(Arr, dtype=np.double)
        mask = traceA != 0
        w[mask] = detA[mask] / traceA[mask]
        tsq = traceA[mask]
        tsq *= tsq
        q[mask] = 4 * detA[mask] / tsq
    return w, q


def kitchen_rosenfeld_response(imx, imy, imxx, imxy, imyy):
    """corner.py:570-590"""
    with np.errstate(all="ignore"):
        numerator = imxx * imy
        numerator *= imy
        tmp = imyy * imx
        tmp *= imx
        numerator += tmp
        tmp = 2 * imxy
        tmp *= imx
        tmp *= imy
        numerator -= tmp
        denominator = imx * imx
        denominator += imy * imy
        response = np.zeros_like(imx, dtype=np.double)
        mask = denominator != 0
        response[mask] = numerator[mask] / denominator[mask]
    return response


def corner_kitchen_rosenfeld(image, mode="constant", cval=0):
    """corner.py:566-590 (on the converted image: the library's deviation)"""
    image = prepare(image)
    imx, imy = derivatives(image, mode, cval)
    imxx, imxy = derivatives(imx, mode, cval)
    imyx, imyy = derivatives(imy, mode, cval)
    return kitchen_rosenfeld_response(imx, imy, imxx, imxy, imyy)


def detector(name, image, gaussian=None, **kw):
    """a whole detector call on an image: the tensor with the detector's defaults (mode 'constant', order 'rc')"""
    if name == "corner_kitchen_rosenfeld":
        return corner_kitchen_rosenfeld(image, **kw)
    sigma = kw.pop("sigma", 1)
    elems = structure_tensor(image, sigma, order="rc", gaussian=gaussian)
    return {"corner_harris": corner_harris, "corner_shi_tomasi": corner_shi_tomasi, "corner_foerstner": corner_foerstner}[name](*elems, **kw)
