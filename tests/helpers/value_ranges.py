"""Inputs on the value ranges of real scans, and a per-voxel error bound that holds on all of them.

Test infrastructure: used by tests/test_value_range_harness.py, tests/test_gpu_value_ranges.py and
scripts/fuzz_vs_scipy.py (`--ranges`), never by the package.

Generators (seeded, generated block-wise along z so that 512^3 costs a few seconds):
  * `mr_u12`     MR magnitudes: a smooth phantom plus noise, integers 0 .. 4095 (uint16 or float32);
  * `ct_hu`      CT Hounsfield units: piecewise-constant blocks of air (-1000), soft tissue (~40) and bone (1500 .. 3071)
                 plus noise, clipped to -1024 .. 3071, with the outside of the in-plane field of view set to the padding
                 value (-32768 for int16, -1024 for float32);
  * `offset_1e4` 1e4 + N(0, 1), float32: the ill-conditioned case of derivative filters;
  * `int_extremes(dtype)` full-range integers with runs of iinfo.min / iinfo.max and values either side of 2^15.

The bound.  A float32 kernel that rounds every product and partial sum may differ from the exact (float64) result by
    |got - ref64| <= c . u . B
per voxel, where u = 2^-24 (float32; 2^-53 for float64), B is the SAME linear operation applied to |x| with |w| as
weights and |cval| as the fill value, and c counts the roundings on the way: Sum over the passes of (taps + 2) for a
separable filter (the taps' partial sums, the rounded weight and the rounded result).  The bound is independent of the
data's offset or scale: a smoothing filter on 1e4 + noise and a derivative of it are held to the same c, while a tap
in the wrong place or a wrong boundary mode breaks it by orders of magnitude.  For smoothing filters (w >= 0) on
non-negative data B = |ref|, so the bound is then a relative error of c . u.
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY = np.finfo(np.float64).tiny

PAD_I16 = -32768
PAD_F32 = -1024.0


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def _block_rng(seed, z0):
    """One generator per block of planes: the volume does not depend on how it is cut into blocks of work."""
    return np.random.default_rng([int(seed), int(z0)])


_ZB = 16          # planes per block


def _shape3(shape):
    shape = tuple(int(s) for s in shape)
    return (1,) + shape if len(shape) == 2 else shape, len(shape) == 2


def mr_u12(shape, seed=0, dtype=np.uint16):
    """A smooth phantom (an ellipsoid with a brighter core and slow in-plane shading) plus N(0, 30) noise, rounded and
    clipped to the 12-bit range 0 .. 4095; uint16 or float32 (the same integers)."""
    s3, flat = _shape3(shape)
    nz, ny, nx = s3
    out = np.empty(s3, dtype)
    zz = (np.arange(nz) - (nz - 1) / 2) / max(nz / 2, 1)
    yy = (np.arange(ny) - (ny - 1) / 2) / max(ny / 2, 1)
    xx = (np.arange(nx) - (nx - 1) / 2) / max(nx / 2, 1)
    r_yx = yy[:, None] ** 2 / 0.85 + xx[None, :] ** 2 / 0.9
    shade = 1.0 + 0.25 * np.cos(2.3 * yy)[:, None] * np.sin(1.7 * xx + 0.4)[None, :]
    for z0 in range(0, nz, _ZB):
        z1 = min(z0 + _ZB, nz)
        r = r_yx[None] + (zz[z0:z1] ** 2 / 0.8)[:, None, None]
        v = np.where(r < 1.0, 1400.0 * shade[None] * (1.0 - 0.3 * r), 120.0)
        v = v + np.where(r < 0.2, 2200.0 * (1.0 - r / 0.2), 0.0)
        v = v + 30.0 * _block_rng(seed, z0).standard_normal(v.shape)
        out[z0:z1] = np.clip(np.rint(v), 0, 4095)
    return out[0] if flat else out


def _cuts(rng, n, lo, hi):
    """Sorted segment boundaries of 0 .. n with segment lengths in [lo, hi)."""
    edges = [0]
    while edges[-1] < n:
        edges.append(edges[-1] + int(rng.integers(lo, hi)))
    return np.minimum(np.asarray(edges), n)


def ct_hu(shape, seed=0, dtype=np.int16):
    """Piecewise-constant blocks of air (-1000), soft tissue (20 .. 80) and bone (1500 .. 3071) plus N(0, 12) noise,
    clipped to -1024 .. 3071; outside the in-plane field of view (a disc touching the middle of every edge) the padding
    value: -32768 (int16) or -1024 (float32)."""
    s3, flat = _shape3(shape)
    nz, ny, nx = s3
    g = np.random.default_rng([int(seed), 1 << 20])
    cz, cy, cx = _cuts(g, nz, 3, 13), _cuts(g, ny, 3, 13), _cuts(g, nx, 3, 13)
    kind = g.choice(3, size=(len(cz) - 1, len(cy) - 1, len(cx) - 1), p=[0.3, 0.45, 0.25])
    level = np.where(kind == 0, -1000.0, np.where(kind == 1, g.uniform(20, 80, kind.shape), g.uniform(1500, 3071, kind.shape)))
    iz = np.searchsorted(cz, np.arange(nz), side="right") - 1
    iy = np.searchsorted(cy, np.arange(ny), side="right") - 1
    ix = np.searchsorted(cx, np.arange(nx), side="right") - 1
    yy = (np.arange(ny) - (ny - 1) / 2) / max((ny - 1) / 2, 0.5)
    xx = (np.arange(nx) - (nx - 1) / 2) / max((nx - 1) / 2, 0.5)
    fov = (yy[:, None] ** 2 + xx[None, :] ** 2) <= 1.0
    pad = PAD_I16 if np.dtype(dtype) == np.int16 else PAD_F32
    out = np.empty(s3, dtype)
    lev_yx = level[:, iy][:, :, ix]                 # (cells along z, ny, nx)
    for z0 in range(0, nz, _ZB):
        z1 = min(z0 + _ZB, nz)
        v = lev_yx[iz[z0:z1]] + 12.0 * _block_rng(seed, z0).standard_normal((z1 - z0, ny, nx))
        v = np.clip(np.rint(v), -1024, 3071)
        out[z0:z1] = np.where(fov[None], v, pad)
    return out[0] if flat else out


def offset_1e4(shape, seed=0):
    """1e4 + N(0, 1) in float32."""
    s3, flat = _shape3(shape)
    out = np.empty(s3, np.float32)
    for z0 in range(0, s3[0], _ZB):
        z1 = min(z0 + _ZB, s3[0])
        out[z0:z1] = 1e4 + _block_rng(seed, z0).standard_normal((z1 - z0,) + s3[1:], dtype=np.float32)
    return out[0] if flat else out


def int_extremes(shape, dtype, seed=0):
    """Uniform over the whole range of the integer dtype, with runs of iinfo.min and iinfo.max along rows and columns,
    whole blocks of each, and (uint16) a band of values 32766 .. 32769; (int16) a band of -2 .. 1."""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    s3, flat = _shape3(shape)
    nz, ny, nx = s3
    g = np.random.default_rng([int(seed), 1 << 21])
    out = g.integers(int(info.min), int(info.max) + 1, size=s3, dtype=np.int64)
    for _ in range(max(2, nz * ny // 16)):            # runs along x
        z, y = int(g.integers(nz)), int(g.integers(ny))
        a = int(g.integers(nx))
        out[z, y, a:a + int(g.integers(2, 12))] = info.min if g.random() < 0.5 else info.max
    for _ in range(max(2, nz * nx // 16)):            # runs along y
        z, x = int(g.integers(nz)), int(g.integers(nx))
        a = int(g.integers(ny))
        out[z, a:a + int(g.integers(2, 12)), x] = info.min if g.random() < 0.5 else info.max
    hz, hy, hx = max(nz // 4, 1), max(ny // 4, 1), max(nx // 4, 1)
    out[:hz, :hy, :hx] = info.min
    out[nz - hz:, ny - hy:, nx - hx:] = info.max
    mid = 1 << 15 if dtype == np.uint16 else 0
    if dtype.itemsize == 2:
        band = g.integers(mid - 2, mid + 2, size=(nz, ny, hx))
        out[:, :, nx // 2 - hx // 2:nx // 2 - hx // 2 + hx] = band
    out = out.astype(dtype)
    return out[0] if flat else out


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def bound_ratio(got, x, op, abs_op, c, u=U32):
    """(max |got - ref| / (c . u . B + tiny), the voxel where it falls) with ref = op(float64 x) and B = abs_op(|float64 x|).
    `op` is the exact operation in float64 (SciPy on a float64 copy), `abs_op` the same linear operation with |w| as
    weights and |cval| as the fill value."""
    x64 = np.asarray(x, dtype=np.float64)
    ref = np.asarray(op(x64), dtype=np.float64)
    B = np.asarray(abs_op(np.abs(x64)), dtype=np.float64)
    return ratio_of(got, ref, B, c, u)


def ratio_of(got, ref, B, c, u=U32, extra=None):
    """bound_ratio's arithmetic on a reference and a B already computed; `extra`: a per-voxel allowance added to the
    bound (coord_term)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == B.shape, (got.shape, ref.shape, B.shape)
    r = np.abs(got - ref) / (c * u * B + (0.0 if extra is None else extra) + TINY)
    r[np.isnan(got) != np.isnan(ref)] = np.inf
    r[np.isnan(got) & np.isnan(ref)] = 0.0
    k = int(np.argmax(r))
    return float(r.flat[k]), np.unravel_index(k, r.shape)


def sep_c(weights):
    """c of a separable filter: Sum over the filtered axes of (taps + 2)."""
    return float(sum(len(w) + 2 for w in weights if w is not None))


def abs_separable(weights, mode="reflect", cval=0.0, order=None):
    """B of a separable filter: correlate1d with |w| along every filtered axis, each pass padded with |cval|, in float64.
    `weights`: one 1-D array (or None) per axis; `mode`: one mode or one per axis; `order`: the axes in the order the
    filter runs its passes (default 0, 1, ...; sobel / prewitt run the derivative axis first) -- with `constant` the
    order matters, as every pass pads its own input with cval."""
    import scipy.ndimage as sndi
    modes = [mode] * len(weights) if isinstance(mode, str) else list(mode)
    axes = list(range(len(weights))) if order is None else list(order)

    def fn(a):
        out = np.asarray(a, dtype=np.float64)
        for ax in axes:
            w = weights[ax]
            if w is not None:
                out = sndi.correlate1d(out, np.abs(np.asarray(w, np.float64)), ax, output=np.float64, mode=modes[ax],
                                       cval=abs(float(cval)))
        return out
    return fn


def gauss_weights(sigma, order=0, truncate=4.0):
    """SciPy's sampled Gaussian (derivative) kernel: phi(x) = exp(-x^2 / 2 sigma^2) / sum, times q_n(x) with q_0 = 1,
    q_1 = -x / sigma^2, q_2 = x^2 / sigma^4 - 1 / sigma^2 (signs do not matter for B)."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    s2 = float(sigma) ** 2
    phi = np.exp(-0.5 * x * x / s2)
    phi /= phi.sum()
    q = {0: np.ones_like(x), 1: -x / s2, 2: x * x / (s2 * s2) - 1.0 / s2}[int(order)]
    return q * phi


def gaussian_spec(ndim, sigma, order=0, truncate=4.0):
    """Per-axis weights of gaussian_filter(sigma, order) (None where sigma is 0)."""
    sig = [sigma] * ndim if np.isscalar(sigma) else list(sigma)
    od = [order] * ndim if np.isscalar(order) else list(order)
    return [None if s <= 1e-15 else gauss_weights(s, o, truncate) for s, o in zip(sig, od)]


def box_spec(ndim, size):
    sz = [size] * ndim if np.isscalar(size) else list(size)
    return [None if n <= 1 else np.full(n, 1.0 / n) for n in sz]


def deriv_order(ndim, axis):
    """The order of the passes of sobel / prewitt: the derivative axis, then the others."""
    axis = axis % ndim
    return [axis] + [a for a in range(ndim) if a != axis]


def deriv_spec(ndim, axis, smooth):
    """sobel ([1, 2, 1]) / prewitt ([1, 1, 1]) along the other axes, [-1, 0, 1] along `axis` (passes: deriv_order)."""
    axis = axis % ndim
    return [np.array([-1.0, 0.0, 1.0]) if a == axis else np.asarray(smooth, np.float64) for a in range(ndim)]


# composite filters: the per-axis bounds combined -------------------------------------------------------------------
def ggm_bound(ndim, sigma, mode="reflect", cval=0.0, truncate=4.0):
    """(abs_op, c) of gaussian_gradient_magnitude: the error of sqrt(Sum d_a^2) is at most the 2-norm of the errors of
    the d_a plus the rounding of the squares, the sum and the root, so B = sqrt(Sum B_a^2) and c = c_pass + 3."""
    specs = [gaussian_spec(ndim, sigma, [1 if i == a else 0 for i in range(ndim)], truncate) for a in range(ndim)]
    fns = [abs_separable(s, mode, cval) for s in specs]
    return (lambda a: np.sqrt(sum(f(a) ** 2 for f in fns))), max(sep_c(s) for s in specs) + 3


def glaplace_bound(ndim, sigma, mode="reflect", cval=0.0, truncate=4.0):
    """(abs_op, c) of gaussian_laplace: Sum of ndim second derivatives, B = Sum B_a and c = c_pass + ndim - 1 adds."""
    specs = [gaussian_spec(ndim, sigma, [2 if i == a else 0 for i in range(ndim)], truncate) for a in range(ndim)]
    fns = [abs_separable(s, mode, cval) for s in specs]
    return (lambda a: sum(f(a) for f in fns)), max(sep_c(s) for s in specs) + ndim - 1


def abs_dense(weights, mode="reflect", cval=0.0):
    """B of a dense correlate: correlate with |w|, |cval|."""
    import scipy.ndimage as sndi
    w = np.abs(np.asarray(weights, np.float64))
    return lambda a: sndi.correlate(np.asarray(a, np.float64), w, output=np.float64, mode=mode, cval=abs(float(cval)))


def dense_c(weights):
    """c of a dense correlate accumulated in float32: nonzero taps + 2."""
    return float(np.count_nonzero(weights) + 2)


def interp_c(ndim, order):
    """c of a B-spline interpolation in float32: Sum over the axes of (order + 1 taps + 2) as for a separable filter,
    and for order > 1 the float32 coefficients: one rounding of their own plus a two-pole recursive prefilter per axis
    (2 taps + 2)."""
    return float(ndim * (order + 3) + (1 + 4 * ndim if order > 1 else 0))


def coord_term(coef, coords, order, mode="constant", cval=0.0, axes=None, u=U32):
    """Per-voxel allowance for sample positions held in float32: a coordinate c rounded to float32 (and its fraction
    taken there) moves the sample by up to 2u (|c| + 2), and an order-1 / order-3 spline changes by at most that times
    the largest coefficient step along the axis inside the support, |coef[i + 1] - coef[i]| (in `constant` mode the step
    to cval at the edge too).  Sum over the interpolated `axes` (default all) of 2u (|c_a| + 2) . L_a.  On smooth or
    N(0, 1) data this is a rounding; across a CT edge of 4000 HU it is what a 1e-5-voxel position error costs."""
    import scipy.ndimage as sndi
    coef = np.asarray(coef, np.float64)
    pad = order + 2
    if mode == "constant":
        P = np.pad(coef, pad, mode="constant", constant_values=float(cval))
    else:
        assert mode == "mirror", mode
        P = np.pad(coef, pad, mode="reflect")
    def fold(c, n):              # `mirror`: the sample a coordinate outside the array stands for
        if mode != "mirror" or n < 2:
            return c
        c = np.abs(c) % (2 * n - 2)
        return np.where(c > n - 1, 2 * n - 2 - c, c)
    idx = tuple(np.clip(np.rint(fold(np.asarray(coords[a], np.float64), coef.shape[a])) + pad, 0, P.shape[a] - 1).astype(np.intp)
                for a in range(coef.ndim))
    out = np.zeros(np.shape(coords[0]))
    for a in (range(coef.ndim) if axes is None else axes):
        D = np.abs(np.diff(P, axis=a, append=np.take(P, [-1], axis=a)))
        L = sndi.maximum_filter(D, size=5 if order > 1 else 3, mode="nearest")
        out += 2.0 * u * (np.abs(coords[a]) + 2.0) * L[idx]
    return out


def sobel3d():
    """The 3-D Sobel kernel along x: [-1, 0, 1] (x) [1, 2, 1] (y) [1, 2, 1] (z) -- zero-sum."""
    d, s = np.array([-1.0, 0.0, 1.0]), np.array([1.0, 2.0, 1.0])
    return s[:, None, None] * s[None, :, None] * d[None, None, :]


def log3d(n=5, sigma=1.0):
    """A sampled Laplacian of Gaussian on an n^3 grid with its mean removed (zero-sum)."""
    r = np.arange(n) - n // 2
    zz, yy, xx = np.meshgrid(r, r, r, indexing="ij")
    q = (zz ** 2 + yy ** 2 + xx ** 2) / float(sigma) ** 2
    w = (q - 3.0) * np.exp(-0.5 * q)
    return w - w.mean()


# ---------------------------------------------------------------------------------------------------------------------
# whole-volume variant: the worst ratio over z sub-slabs on the fork pool of helpers/fullsize.py
# ---------------------------------------------------------------------------------------------------------------------
def _bound_worker(job):
    from helpers import fullsize as fs
    a, b = job
    G = fs._G
    x, got, op, abs_op, lo, hi, c, u = (G[k] for k in ("x", "got", "op", "abs_op", "lo", "hi", "c", "u"))
    x64 = lambda s: np.asarray(s, np.float64)            # noqa: E731
    ref = fs.ref_on_slab(x, a, b, lo, hi, lambda s: op(x64(s)))
    B = fs.ref_on_slab(x, a, b, lo, hi, lambda s: abs_op(np.abs(x64(s))))
    r, at = ratio_of(got[a:b], ref, B, c, u)
    return r, (at[0] + a,) + tuple(at[1:])


def whole_volume_bound(x, got, lo, hi, op, abs_op, c, u=U32, planes=8, procs=None):
    """bound_ratio over EVERY plane of `got` (host result of the device call on `x`): z sub-slabs of `planes` planes with
    (lo, hi) planes of context, as fullsize.whole_volume_filter.  Returns (worst ratio, voxel)."""
    from helpers import fullsize as fs
    assert got.shape == x.shape
    fs._G.update(x=x, got=got, op=op, abs_op=abs_op, lo=lo, hi=hi, c=c, u=u)
    try:
        res = fs._run_pool(_bound_worker, fs._jobs(x.shape[0], planes), procs)
    finally:
        fs._G.clear()
    return max(res, key=lambda t: t[0])
