"""NumPy transcription of skimage.restoration.richardson_lucy's contract (include/mi355img.h, the docstring of
cupyimg_amd.skimage.restoration.richardson_lucy), written from the contract and not from the kernels.

    T = promote_types(image.dtype, float32);  image, psf -> T;  u = full(image.shape, T(0.5))
    repeat: c = conv(u, reversed psf taps);  r = image / c;  r = where(c < T(eps), 0, r) if eps;  u = u * conv(r, psf taps)
    clip at the end

Both sums visit the non-zero taps of their weights array in C order, form and add every product in float64 starting from
+0.0 -- a sample outside the image is a 0.0 that is multiplied and added like any other (so 0 * inf gives NaN there too) -- and
round the sum once to T.  The window of voxel i reaches from i - s // 2 to i + (s - 1) // 2 along every axis."""
import numpy as np


def float_type(dtype):
    return np.promote_types(np.dtype(dtype), np.float32)


def _window_sum(x, weights, T):
    """out[i] = T(sum over the non-zero taps t of `weights`, in C order, of float64(x[i - s // 2 + t]) * weights[t]), zero outside"""
    s = weights.shape
    pads = [(n // 2, (n - 1) // 2) for n in s]
    xp = np.pad(x.astype(np.float64), pads, mode="constant", constant_values=0.0)
    acc = np.zeros(x.shape, np.float64)
    w = weights.astype(np.float64)
    with np.errstate(all="ignore"):
        for t in np.ndindex(*s):
            if w[t] == 0.0:
                continue
            window = xp[tuple(slice(t[d], t[d] + x.shape[d]) for d in range(x.ndim))]
            acc = acc + window * w[t]
        return acc.astype(T)


def richardson_lucy(image, psf, iterations=50, clip=True, filter_epsilon=None):
    image = np.asarray(image)
    psf = np.asarray(psf)
    T = float_type(image.dtype)
    image = image.astype(T)
    psf = psf.astype(T)
    u = np.full(image.shape, 0.5, dtype=T)
    reversed_psf = np.flip(psf)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            c = _window_sum(u, reversed_psf, T)
            r = image / c
            if filter_epsilon:
                r = np.where(c < T.type(filter_epsilon), T.type(0), r)
            u = u * _window_sum(r, psf, T)
        if clip:
            u[u > 1] = 1
            u[u < -1] = -1
    return u
