"""Host yardstick of the Hessian family: a NumPy / SciPy transcription of the reference's skimage.feature.hessian_matrix,
hessian_matrix_eigvals and skimage.filters.meijering / sato / frangi / hessian (feature/corner.py:141-211, 260-458,
filters/ridges.py:21-635), operation by operation, oddities included:

* order "rc" enumerates the axes in REVERSE (corner.py:203-204);
* meijering's `auxiliary[-1]` is the eigenvalue of largest magnitude times its coefficients summed one by one
  (ridges.py:262-278: the comprehension multiplies eigenvalues[i] by roll(coefficients, j)[i] for every j);
* `x ** (1 / n)` as NumPy evaluates it, `_divide_nonzero` with 1e-10.

Every function keeps the dtype it is given (coefficients are cast to it), so a float32 call is float32 throughout."""
from functools import reduce
from itertools import combinations_with_replacement

import numpy as np
from scipy import ndimage as ndi


def img_as_float(image):
    image = np.asarray(image)
    dt = image.dtype
    if dt.kind == "f":
        return image
    if dt == np.bool_:
        return image.astype(np.float64)
    info = np.iinfo(dt)
    out = image.astype(np.float64)
    if dt.kind == "u":
        return out * (1.0 / info.max)
    return (out * 2.0 + 1.0) / (float(info.max) - float(info.min))


def invert(image):
    image = np.asarray(image)
    dt = image.dtype
    if dt == np.bool_:
        return ~image
    if dt.kind == "u":
        return np.subtract(np.iinfo(dt).max, image, dtype=dt)
    if dt.kind == "i":
        return np.subtract(-1, image, dtype=dt)
    return np.subtract(1, image, dtype=dt)


def hessian_from_smoothed(g, order="rc"):
    gradients = np.gradient(g)
    if g.ndim == 1:
        gradients = [gradients]
    axes = range(g.ndim)
    if order == "rc":
        axes = reversed(axes)
    return [np.gradient(gradients[a0], axis=a1) for a0, a1 in combinations_with_replacement(axes, 2)]


def hessian_matrix(image, sigma=1, mode="constant", cval=0, order="rc"):
    image = img_as_float(image)
    return hessian_from_smoothed(ndi.gaussian_filter(image, sigma=sigma, mode=mode, cval=cval), order)


def eigvals22(m00, m01, m11):
    """corner.py:260-281"""
    tmp1 = m01 * m01
    tmp1 *= 4
    tmp2 = m00 - m11
    tmp2 *= tmp2
    tmp2 += tmp1
    np.sqrt(tmp2, out=tmp2)
    tmp2 /= 2
    tmp1 = m00 + m11
    tmp1 /= 2
    return tmp1 + tmp2, tmp1 - tmp2


def symmetric_image(elems, dtype=np.float64):
    ndim = elems[0].ndim
    out = np.zeros(elems[0].shape + (ndim, ndim), dtype)
    for idx, (row, col) in enumerate(combinations_with_replacement(range(ndim), 2)):
        out[..., row, col] = elems[idx]
        out[..., col, row] = elems[idx]
    return out


def hessian_matrix_eigvals(elems, dtype=np.float64):
    """decreasing along a new leading axis; larger than 2 x 2: LAPACK in `dtype`"""
    if len(elems) == 1:
        return np.stack([np.asarray(elems[0])])
    if len(elems) == 3:
        return np.stack(eigvals22(*elems))
    eigs = np.linalg.eigvalsh(symmetric_image(elems, dtype))[..., ::-1]
    return np.moveaxis(eigs, -1, 0)


def sortbyabs(array, axis=0):
    index = list(np.ix_(*[np.arange(i) for i in array.shape]))
    index[axis] = np.abs(array).argsort(axis, kind="stable")
    return array[tuple(index)]


def order_eigenvalues(eigs, sorting):
    if sorting == "abs":
        return sortbyabs(eigs, axis=0)
    if sorting == "val":
        return np.sort(eigs, axis=0)
    return eigs


def eigenvalues_from_smoothed(g, sigma, sorting="none", eig_dtype=np.float64):
    """ridges.py:147-173 from the smoothed array on; the eigenvalues are returned in g's dtype"""
    s2 = g.dtype.type(sigma ** 2)
    elems = [s2 * e for e in hessian_from_smoothed(g, "rc")]
    eigs = hessian_matrix_eigvals(elems, eig_dtype).astype(g.dtype)
    return order_eigenvalues(eigs, sorting)


def divide_nonzero(a, b, cval=1e-10):
    den = np.array(b, copy=True)
    den[den == 0] = cval
    return np.divide(a, den)


def frangi_response(eigs, alpha=0.5, beta=0.5, gamma=15):
    """eigs: ordered by magnitude, (ndim, ...) with ndim 2 or 3 (ridges.py:500-530, one scale, background removed)"""
    dt = eigs.dtype.type
    ndim = eigs.shape[0]
    alpha_sq, beta_sq, gamma_sq = dt(2 * alpha ** 2), dt(2 * beta ** 2), dt(2 * gamma ** 2)
    lambda1, *lambdas = eigs
    with np.errstate(all="ignore"):
        r_a = dt(np.inf) if ndim == 2 else divide_nonzero(*lambdas) ** 2
        filtered_raw = np.abs(reduce(np.multiply, lambdas)) ** dt(1 / len(lambdas))
        r_b = divide_nonzero(lambda1, filtered_raw) ** 2
        r_g = sum([lambda1 ** 2] + [l ** 2 for l in lambdas])
        out = (1 - np.exp(-r_a / alpha_sq)) * np.exp(-r_b / beta_sq) * (1 - np.exp(-r_g / gamma_sq))
    out = np.array(out, dtype=eigs.dtype)
    out[np.max(np.asarray(lambdas), axis=0) > 0] = 0
    return out


def sato_response(eigs):
    """eigs: increasing (ridges.py:371-380)"""
    dt = eigs.dtype.type
    _, *lambdas = eigs
    filtered = np.abs(reduce(np.multiply, lambdas)) ** dt(1 / len(lambdas))
    return np.where(lambdas[-1] > 0, filtered, 0).astype(eigs.dtype)


def meijering_aux(eigs, alpha):
    """eigs: ordered by magnitude (ridges.py:262-278)"""
    dt = eigs.dtype.type
    ndim = eigs.shape[0]
    coefficients = [alpha] * ndim
    coefficients[0] = 1
    auxiliary = [np.sum([eigs[i] * dt(np.roll(coefficients, j)[i]) for j in range(ndim)], axis=0) for i in range(ndim)]
    return auxiliary[-1]


def meijering_response(aux):
    """ridges.py:282-285"""
    filtered = divide_nonzero(aux, np.min(aux))
    return np.where(aux < 0, filtered, 0).astype(aux.dtype)


def _filter(image, sigmas, mode, cval, sorting, response):
    out = np.zeros((len(sigmas),) + image.shape)
    for i, sigma in enumerate(sigmas):
        g = ndi.gaussian_filter(image, sigma=float(sigma), mode=mode, cval=cval)
        out[i] = response(eigenvalues_from_smoothed(g, sigma, sorting))
    return np.max(out, axis=0)


def meijering(image, sigmas=range(1, 10, 2), alpha=None, black_ridges=True, mode="reflect", cval=0):
    sigmas = np.asarray(sigmas).ravel()
    image = np.asarray(image)
    if alpha is None:
        alpha = 1.0 / image.ndim
    if black_ridges:
        image = invert(image)
    image = img_as_float(image)
    return _filter(image, sigmas, mode, cval, "abs", lambda e: meijering_response(meijering_aux(e, alpha)))


def sato(image, sigmas=range(1, 10, 2), black_ridges=True, mode="reflect", cval=0):
    sigmas = np.asarray(sigmas).ravel()
    image = np.asarray(image)
    if not black_ridges:
        image = invert(image)
    image = img_as_float(image)
    return _filter(image, sigmas, mode, cval, "val", sato_response)


def frangi(image, sigmas=range(1, 10, 2), alpha=0.5, beta=0.5, gamma=15, black_ridges=True, mode="reflect", cval=0):
    sigmas = np.asarray(sigmas).ravel()
    image = np.asarray(image)
    if black_ridges:
        image = invert(image)
    image = img_as_float(image)
    return _filter(image, sigmas, mode, cval, "abs", lambda e: frangi_response(e, alpha, beta, gamma))


def hessian(image, **kw):
    out = frangi(image, **kw)
    out[out <= 0] = 1
    return out


def volume(shape, dtype=np.float64, seed=0):
    """two crossing tubes, a blob and a plate on noise, scaled to [0, 1]; any rank >= 2"""
    rng = np.random.default_rng(seed)
    nd = len(shape)
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    c = [(n - 1) / 2.0 for n in shape]
    w = max(1.0, min(shape) / 8.0)
    v = np.zeros(shape)
    # a tube along the last axis and one along the first, through the centre
    d2 = sum((grid[a] - c[a]) ** 2 for a in range(nd - 1))
    v += np.exp(-d2 / (2 * w * w))
    d2 = sum((grid[a] - c[a]) ** 2 for a in range(1, nd))
    v += np.exp(-d2 / (2 * w * w))
    # a blob off centre
    d2 = sum((grid[a] - 0.25 * shape[a]) ** 2 for a in range(nd))
    v += 0.8 * np.exp(-d2 / (2 * (1.5 * w) ** 2))
    # a plate normal to the first axis
    v += 0.6 * np.exp(-(grid[0] - 0.8 * shape[0]) ** 2 / (2 * w * w))
    v += 0.05 * rng.standard_normal(shape)
    v -= v.min()
    if v.max() > 0:
        v /= v.max()
    return v.astype(dtype)
