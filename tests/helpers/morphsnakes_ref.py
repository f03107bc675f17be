"""Host transcription of the morphological snakes as cupyimg_amd.skimage.segmentation defines them (the stages of
include/mi355img.h, mi_snake_*; the reference: cupyimg/skimage/segmentation/morphsnakes.py), with NumPy and SciPy's binary
morphology, in the image's own dtype operation by operation:

    MorphACWE   c0 = sum(I (1 - u)) / (sum(1 - u) + 1e-8),  c1 = sum(I u) / (sum(u) + 1e-8)
                aux = |gradient(u)|_1 * (lambda1 (I - c1)^2 - lambda2 (I - c0)^2);   aux < 0: u = 1,  aux > 0: u = 0
    MorphGAC    balloon: u = dilation / erosion of u by the full 3^ndim element where double(I) > double(threshold) / |balloon|
                aux = sum_axis gradient(I)[axis] * gradient(u)[axis];   aux > 0: u = 1,  aux < 0: u = 0
    smoothing   step j of a CALL (j = 0, 1, ... through its iterations) is sup_inf(inf_sup(u)) for even j, inf_sup(sup_inf(u)) for odd j

Two things differ from the reference on purpose: the alternation of the smoothing operator starts afresh in every call (the
reference keeps one cycle per process), and the balloon mask is compared in float64 (threshold = "auto" is
numpy.percentile(float64(image), 40)).  bool and integer images are computed in float64, float16 in float32.  Also the
seeded inputs of the GPU tests."""
import functools
import zlib

import numpy as np
from scipy import ndimage as ndi


def _elements(ndim):
    """the 4 lines through the centre of a 3 x 3 square / the 9 planes through the centre of a 3 x 3 x 3 cube"""
    if ndim == 2:
        return [np.eye(3), np.array([[0, 1, 0]] * 3), np.flipud(np.eye(3)), np.rot90([[0, 1, 0]] * 3)]
    if ndim != 3:
        raise ValueError("u has an invalid number of dimensions (should be 2 or 3)")
    i = np.arange(3)
    out = [np.zeros((3, 3, 3)) for _ in range(9)]
    out[0][:, :, 1] = 1
    out[1][:, 1, :] = 1
    out[2][1, :, :] = 1
    out[3][:, i, i] = 1
    out[4][:, i, 2 - i] = 1
    out[5][i, :, i] = 1
    out[6][i, :, 2 - i] = 1
    out[7][i, i, :] = 1
    out[8][i, 2 - i, :] = 1
    return out


def sup_inf(u):
    u = np.asarray(u)
    return np.stack([ndi.binary_erosion(u, p).astype(np.int8) for p in _elements(u.ndim)]).max(0)


def inf_sup(u):
    u = np.asarray(u)
    return np.stack([ndi.binary_dilation(u, p).astype(np.int8) for p in _elements(u.ndim)]).min(0)


def curvature(u, j):
    """smoothing step number j of a call"""
    return sup_inf(inf_sup(u)) if j % 2 == 0 else inf_sup(sup_inf(u))


def disk_level_set(image_shape, center=None, radius=None):
    if center is None:
        center = tuple(i // 2 for i in image_shape)
    if radius is None:
        radius = min(image_shape) * 3.0 / 8.0
    grid = np.mgrid[tuple(slice(i) for i in image_shape)]
    grid = (grid.T - np.asarray(center)).T
    return (radius - np.sqrt(np.sum(grid ** 2, 0)) > 0).astype(np.int8)


def checkerboard_level_set(image_shape, square_size=5):
    grid = np.mgrid[tuple(slice(i) for i in image_shape)]
    grid = (grid // square_size) & 1
    return functools.reduce(np.bitwise_xor, list(grid)).astype(np.int8)


def _level_set(init, shape):
    if isinstance(init, str):
        if init == "checkerboard":
            return checkerboard_level_set(shape)
        if init in ("disk", "circle"):
            return disk_level_set(shape)
        raise ValueError("`init_level_set` not in ['checkerboard', 'circle', 'disk']")
    return np.asarray(init)


def _image(image):
    image = np.asarray(image)
    if image.dtype == np.float16:
        return image.astype(np.float32)
    if image.dtype not in (np.float32, np.float64):
        return image.astype(np.float64)
    return image


def chan_vese(image, iterations, init_level_set="checkerboard", smoothing=1, lambda1=1, lambda2=1, iter_callback=None,
              on_sums=None):
    """on_sums(image * (1 - u), image * u, 1 - u, u): the four arrays whose sums make c0 and c1, every iteration"""
    image = _image(image)
    u = (_level_set(init_level_set, image.shape) > 0).astype(np.int8)
    assert u.shape == image.shape and image.ndim in (2, 3)
    if iter_callback:
        iter_callback(u.copy())
    j = 0
    for _ in range(iterations):
        outside, inside = image * (1 - u), image * u
        if on_sums:
            on_sums(outside, inside, 1 - u, u)
        c0 = outside.sum() / float((1 - u).sum() + 1e-8)
        c1 = inside.sum() / float(u.sum() + 1e-8)
        assert np.asarray(c0).dtype == image.dtype and np.asarray(c1).dtype == image.dtype
        abs_du = np.abs(np.stack(np.gradient(u))).sum(0)
        bracket = lambda1 * (image - c1) ** 2 - lambda2 * (image - c0) ** 2
        assert bracket.dtype == image.dtype
        aux = abs_du * bracket
        u[aux < 0] = 1
        u[aux > 0] = 0
        for _ in range(smoothing):
            u = curvature(u, j)
            j += 1
        if iter_callback:
            iter_callback(u.copy())
    return u


def auto_threshold(image):
    return float(np.percentile(_image(image).astype(np.float64), 40))


def geodesic_active_contour(gimage, iterations, init_level_set="disk", smoothing=1, threshold="auto", balloon=0, iter_callback=None):
    image = _image(gimage)
    u = (_level_set(init_level_set, image.shape) > 0).astype(np.int8)
    assert u.shape == image.shape and image.ndim in (2, 3)
    if isinstance(threshold, str):
        assert threshold == "auto"
        threshold = auto_threshold(image)
    structure = np.ones((3,) * image.ndim, np.int8)
    dimage = np.gradient(image)
    assert all(g.dtype == image.dtype for g in dimage)
    if balloon != 0:
        mask = image.astype(np.float64) > float(threshold) / abs(float(balloon))
    if iter_callback:
        iter_callback(u.copy())
    j = 0
    for _ in range(iterations):
        if balloon > 0:
            aux = ndi.binary_dilation(u, structure)
        elif balloon < 0:
            aux = ndi.binary_erosion(u, structure)
        if balloon != 0:
            u[mask] = aux[mask]
        aux = np.zeros_like(image)
        for el1, el2 in zip(dimage, np.gradient(u)):
            aux += el1 * el2
        u[aux > 0] = 1
        u[aux < 0] = 0
        for _ in range(smoothing):
            u = curvature(u, j)
            j += 1
        if iter_callback:
            iter_callback(u.copy())
    return u


def inverse_gaussian_gradient(image, alpha=100.0, sigma=5.0):
    gradnorm = ndi.gaussian_gradient_magnitude(image, sigma, mode="nearest")
    return 1.0 / np.sqrt(1.0 + alpha * gradnorm)


# ---------------------------------------------------------------------------------------------------------------- inputs
def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _blob(shape):
    axes = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij", sparse=True)
    r2 = sum(((a - 0.45) / 0.3) ** 2 for a in axes)
    return np.exp(-r2)


def exact_image(shape, dtype=np.float64, seed=1):
    """A smooth blob plus seeded noise, rounded to the integers 0 .. 255 and (float dtypes) divided by 256: every sum of a
    subset is an integer multiple of 1 / 256 below 2^24 / 256 for up to 65 000 voxels, so it is exact in float32 in any
    order (tests/test_morphsnakes_yardstick.py checks exactly that on every input the GPU tests use)."""
    rng = rng_for("snake_exact", tuple(shape), seed)
    k = np.clip(np.rint(40 + 150 * _blob(shape) + 25 * rng.standard_normal(tuple(shape))), 0, 255)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (k / 256).astype(dtype)
    return k.astype(dtype)


def volume(shape, dtype=np.float64, seed=1):
    """A seeded volume for MorphGAC (no sums, so any values do): a blob with an edge plus noise, between about 0 and 1.2."""
    rng = rng_for("snake_volume", tuple(shape), seed)
    b = _blob(shape)
    return (0.2 + 0.8 * (b > 0.5) * b + 0.1 * rng.standard_normal(tuple(shape))).astype(dtype)


def mask(shape, density, seed=1):
    if density >= 1:
        return np.ones(shape, np.int8)
    if density <= 0:
        return np.zeros(shape, np.int8)
    return (rng_for("snake_mask", tuple(shape), density, seed).random(tuple(shape)) < density).astype(np.int8)


def fractional_level_set(shape, seed=1):
    """an explicit start with negative and fractional values: positive inside a blob-shaped region, plus noise"""
    rng = rng_for("snake_ls", tuple(shape), seed)
    return (_blob(shape) - 0.4 + 0.3 * rng.standard_normal(tuple(shape))).astype(np.float64)


# the MorphACWE inputs of the GPU tests: (shape, dtype, seed of `exact_image`)
ACWE_CASES = [((20, 37, 70), "float32", 1), ((20, 37, 70), "float64", 1), ((70, 96), "float64", 1), ((70, 96), "float32", 2),
              ((33, 18, 130), "float64", 1), ((20, 37, 70), "uint8", 3), ((12, 20, 70), "float32", 1), ((12, 20, 70), "float64", 2),
              ((12, 20, 70), "uint8", 1)]
