"""Host transcription of Chambolle's projection algorithm as cupyimg_amd.skimage.restoration.denoise_tv_chambolle defines it
(written from the equations of include/mi355img.h, mi_tv_chambolle_step), in the image's own dtype operation by operation:

    d(q)   = -((p_0(q) + p_1(q)) + p_2(q) ...), then for a = 0, 1, ...: d += p_a(q - e_a) where q_a >= 1
    out(q) = image(q) + d(q)
    g_a(q) = out(q + e_a) - out(q) where q_a < n_a - 1, else 0
    norm   = sqrt(((g_0 g_0 + g_1 g_1) + g_2 g_2) ...)
    den    = norm * T(tau / weight) + 1
    p_a'   = (p_a - T(tau) g_a) / den
    E_i    = (sum d d + weight * sum norm) / size              here in T, as NumPy sums (the device: in double)

The loop stops at the first i >= 1 with |E_(i-1) - E_i| < eps * E_0; the result is `out` of that iteration.  Also the
seeded test volume of the GPU tests: an ellipsoid plus a half-space step plus Gaussian noise."""
import zlib

import numpy as np


def tv_chambolle(image, weight=0.1, eps=2.0e-4, n_iter_max=200):
    """-> (out, i_stop, ratios): i_stop is the loop variable at exit (n_iter_max when the loop ran out),
    ratios[i] = |E_(i-1) - E_i| / (eps * E_0) for i >= 1 (inf for i = 0 and where eps * E_0 is 0)."""
    image = np.asarray(image)
    T = image.dtype.type
    assert image.dtype in (np.float32, np.float64) and n_iter_max >= 1
    nd = image.ndim
    tau = 1.0 / (2.0 * nd)
    t_tau, t_tw, one = T(tau), T(tau / weight), T(1)
    p = np.zeros((nd,) + image.shape, image.dtype)
    ratios = [np.inf]
    e_init = e_prev = None
    i = 0
    out = image
    with np.errstate(divide="ignore", invalid="ignore"):
        while i < n_iter_max:
            s = p[0]
            for a in range(1, nd):
                s = s + p[a]
            d = -s
            for a in range(nd):
                hi = [slice(None)] * nd
                lo = [slice(None)] * nd
                hi[a] = slice(1, None)
                lo[a] = slice(0, -1)
                d[tuple(hi)] += p[(a,) + tuple(lo)]
            out = image + d
            g = np.zeros_like(p)
            for a in range(nd):
                hi = [slice(None)] * nd
                lo = [slice(None)] * nd
                hi[a] = slice(1, None)
                lo[a] = slice(0, -1)
                g[(a,) + tuple(lo)] = out[tuple(hi)] - out[tuple(lo)]
            n2 = g[0] * g[0]
            for a in range(1, nd):
                n2 = n2 + g[a] * g[a]
            norm = np.sqrt(n2)
            assert d.dtype == image.dtype and norm.dtype == image.dtype
            e = T(T((d * d).sum(dtype=image.dtype) + T(weight) * norm.sum(dtype=image.dtype)) / T(image.size))
            den = norm * t_tw + one
            for a in range(nd):
                p[a] = (p[a] - t_tau * g[a]) / den
            if i == 0:
                e_init = e_prev = e
            else:
                bound = eps * float(e_init)
                ratios.append(abs(float(e_prev) - float(e)) / bound if bound > 0 else np.inf)
                if abs(e_prev - e) < T(eps) * e_init:
                    break
                e_prev = e
            i += 1
    return out, i, ratios


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def volume(shape, dtype=np.float64, seed=1):
    """An ellipsoid of value 1 centred in the array (semi-axes 0.35 of each extent), plus 0.5 on the half-space where the
    coordinates, each scaled to [0, 1], sum to more than half the rank, plus Gaussian noise of sigma 0.2: edges and flat
    parts at any rank."""
    rng = rng_for("tv_volume", tuple(shape), seed)
    axes = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij", sparse=True)
    r2 = sum(((a - 0.5) / 0.35) ** 2 for a in axes)
    img = (r2 <= 1.0).astype(np.float64) + 0.5 * (sum(axes) > 0.5 * len(shape))
    img = img + 0.2 * rng.standard_normal(tuple(shape))
    return img.astype(dtype)


# the inputs of the GPU stopping tests: (shape, weight, seed of `volume`); tests/test_tv_yardstick.py checks that each stops
# clear of the threshold in float32 and float64 alike (seeds whose run came within 0.5 % of it were replaced)
STOP_CASES = [((12, 20, 70), 0.3, 1), ((9, 37, 64), 0.1, 2), ((9, 37, 64), 0.3, 1), ((33, 18, 130), 0.1, 3),
              ((33, 18, 130), 0.3, 1), ((40, 96), 0.1, 1), ((5, 6, 7, 8), 0.1, 2)]
