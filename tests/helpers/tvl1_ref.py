"""Host transcription of TV-L1 optical flow as cupyimg_amd.skimage.registration.optical_flow_tvl1 defines it (written from the
equations of include/mi355img.h, mi_tvl1_*, and the docstrings of the Python layer), in the images' own dtype T operation by
operation, sums over the component axis left to right:

    per warp      w      = clip(order-1 interpolation of moving at grid + flow, mode "nearest")
                  grad   = numpy.gradient(w);  NI = sum grad^2, 1 where 0;  rho_0 = (w - reference) - sum grad flow
    data term     rho    = rho_0 + sum grad flow
                  |rho| <= T(f0) NI:  flow_a -= (rho grad_a) / NI       else:  flow_a -= (T(f0) sign(rho)) grad_a
    component c   v = flow[c] after the data term, u = v, p = proj[c]; twice:
                  g_a = u(q + e_a) - u(q), 0 at the last index;  norm = sqrt(sum g^2) * T(f1) + 1;  p_a = (p_a - T(dt) g_a) / norm
                  d = -sum p, then axis by axis d(q) += p_a(q - e_a) where q_a >= 1;  u = v + d
    stop          sum (flow_previous - flow)^2 < tol * size, flow_previous as the docstring of optical_flow_tvl1 says

Every building block that is not the solver itself is a callable in `BLOCKS` (SciPy by default): the GPU tests run the same
transcription with the device library's interpolation and filters plugged in, so that only the new code differs."""
import math

import numpy as np
from scipy import ndimage as sndi

_PAD_TO_NDI = {"constant": "constant", "edge": "nearest", "symmetric": "reflect", "reflect": "mirror", "wrap": "wrap"}


# ---------------------------------------------------------------- building blocks (SciPy)
def warp_scipy(image, coords):
    """order-1 interpolation at `coords` (ndim, *shape), mode "nearest", clipped to the image's range"""
    out = sndi.map_coordinates(image, coords, order=1, mode="nearest", output=image.dtype)
    return np.clip(out, image.min(), image.max())


def gaussian_scipy(image, sigma, mode, cval):
    return sndi.gaussian_filter(image, sigma, mode=mode, cval=cval)


def zoom0_scipy(flow, factors):
    return sndi.zoom(flow, factors, order=0, mode="nearest", prefilter=False)


def median_scipy(flow):
    return sndi.median_filter(flow, size=[1] + (flow.ndim - 1) * [3])


def interp_scipy(image, factors, output_shape, order, mode, cval):
    """output sample i of axis a reads the input at factors[a] * (i + 0.5) - 0.5"""
    axes = [factors[a] * (np.arange(n) + 0.5) - 0.5 for a, n in enumerate(output_shape)]
    coords = np.stack(np.meshgrid(*axes, indexing="ij"))
    return sndi.map_coordinates(image, coords, order=order, mode=mode, cval=cval, output=image.dtype)


BLOCKS = {"warp": warp_scipy, "gaussian": gaussian_scipy, "zoom0": zoom0_scipy, "median": median_scipy, "interp": interp_scipy}


def blocks(**replaced):
    b = dict(BLOCKS)
    b.update(replaced)
    return b


# ---------------------------------------------------------------- resize and the pyramid
def _as_float(image):
    image = np.asarray(image)
    assert image.dtype.kind == "f", "the transcription takes float images"
    return image


def resize(image, output_shape, order=1, mode="reflect", cval=0, clip=True, anti_aliasing=True, anti_aliasing_sigma=None,
           blocks=BLOCKS):
    image = _as_float(image)
    output_shape = tuple(output_shape)
    if len(output_shape) == image.ndim - 1:
        output_shape = output_shape + (image.shape[-1],)
    elif len(output_shape) > image.ndim:
        image = image.reshape(image.shape + (1,) * (len(output_shape) - image.ndim))
    elif len(output_shape) < image.ndim - 1:
        raise ValueError("output_shape too short")
    factors = np.asarray(image.shape, dtype=float) / np.asarray(output_shape, dtype=float)
    if anti_aliasing:
        if anti_aliasing_sigma is None:
            sigma = np.maximum(0, (factors - 1) / 2)
        else:
            sigma = np.atleast_1d(anti_aliasing_sigma) * np.ones_like(factors)
            if np.any(sigma < 0):
                raise ValueError("negative sigma")
        image = blocks["gaussian"](image, [float(s) for s in sigma], _PAD_TO_NDI[mode], cval)
    out = blocks["interp"](image, factors, output_shape, order, _PAD_TO_NDI[mode], cval)
    if clip and order != 0:
        lo, hi = image.min(), image.max()
        if mode == "constant" and not (lo <= cval <= hi):
            out = np.where(out == cval, out, np.clip(out, lo, hi))
        else:
            out = np.clip(out, lo, hi)
    return out


def _smooth(image, sigma, mode, cval, multichannel, blocks):
    if multichannel:
        sigma = (sigma,) * (image.ndim - 1) + (0,)
    return blocks["gaussian"](image, sigma, mode, cval)


def pyramid_reduce(image, downscale=2, sigma=None, order=1, mode="reflect", cval=0, multichannel=False, blocks=BLOCKS):
    if downscale <= 1:
        raise ValueError("scale factor must be greater than 1")
    image = _as_float(image)
    out_shape = tuple(math.ceil(d / float(downscale)) for d in image.shape)
    if multichannel:
        out_shape = out_shape[:-1]
    if sigma is None:
        sigma = 2 * downscale / 6.0
    smoothed = _smooth(image, sigma, mode, cval, multichannel, blocks)
    return resize(smoothed, out_shape, order=order, mode=mode, cval=cval, anti_aliasing=False, blocks=blocks)


def pyramid_expand(image, upscale=2, sigma=None, order=1, mode="reflect", cval=0, multichannel=False, blocks=BLOCKS):
    if upscale <= 1:
        raise ValueError("scale factor must be greater than 1")
    image = _as_float(image)
    out_shape = tuple(math.ceil(upscale * d) for d in image.shape)
    if multichannel:
        out_shape = out_shape[:-1]
    if sigma is None:
        sigma = 2 * upscale / 6.0
    resized = resize(image, out_shape, order=order, mode=mode, cval=cval, anti_aliasing=False, blocks=blocks)
    return _smooth(resized, sigma, mode, cval, multichannel, blocks)


def get_pyramid(image, downscale=2.0, nlevel=10, min_size=16, blocks=BLOCKS):
    """coarsest level first"""
    levels = [image]
    while len(levels) < nlevel and min(levels[-1].shape) > downscale * min_size:
        levels.append(pyramid_reduce(levels[-1], downscale, blocks=blocks))
    return levels[::-1]


def resize_flow(flow, shape, blocks=BLOCKS):
    T = flow.dtype.type
    scale = [n / o for n, o in zip(shape, flow.shape[1:])]
    zoomed = blocks["zoom0"](flow, [1] + scale)
    out = np.empty_like(zoomed)
    for c, s in enumerate(scale):
        out[c] = T(s) * zoomed[c]
    return out


# ---------------------------------------------------------------- the solver's stages
def _csum(terms):
    """left to right"""
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


def prepare(warped, reference, flow):
    """-> grad (ndim, *shape), NI, rho_0"""
    grad = np.stack(np.gradient(warped)).astype(warped.dtype, copy=False)
    NI = _csum([g * g for g in grad])
    NI = np.where(NI == 0, warped.dtype.type(1), NI)
    rho_0 = (warped - reference) - _csum([g * f for g, f in zip(grad, flow)])
    return grad, NI, rho_0


def _data_step(rho_0, grad, NI, flow, f0):
    """in place on `flow`"""
    T = flow.dtype.type
    rho = rho_0 + _csum([g * f for g, f in zip(grad, flow)])
    near = np.abs(rho) <= T(f0) * NI
    with np.errstate(divide="ignore", invalid="ignore"):
        step_near = [(rho * g) / NI for g in grad]
    srho = T(f0) * np.sign(rho)
    for a in range(len(flow)):
        flow[a] = np.where(near, flow[a] - step_near[a], flow[a] - srho * grad[a])


def _dual_step(u, p, dt, f1):
    """one step of p (ndim, *shape) against u, in place; then -> d"""
    T = u.dtype.type
    nd = u.ndim
    g = np.zeros_like(p)
    for a in range(nd):
        lo = [slice(None)] * nd
        hi = [slice(None)] * nd
        lo[a] = slice(0, -1)
        hi[a] = slice(1, None)
        g[a][tuple(lo)] = u[tuple(hi)] - u[tuple(lo)]
    norm = np.sqrt(_csum([x * x for x in g]))
    norm = norm * T(f1)
    norm = norm + T(1)
    for a in range(nd):
        p[a] = (p[a] - T(dt) * g[a]) / norm
    d = -_csum(list(p))
    for a in range(nd):
        lo = [slice(None)] * nd
        hi = [slice(None)] * nd
        lo[a] = slice(0, -1)
        hi[a] = slice(1, None)
        d[tuple(hi)] += p[a][tuple(lo)]
    return d


def _fixed_point(rho_0, grad, NI, flow, proj, f0, f1, dt):
    """one fixed-point iteration: the data term in place on `flow` (which the caller keeps as flow_auxiliary), both
    regularisation steps in place on `proj`; -> the new flow (a new array)"""
    _data_step(rho_0, grad, NI, flow, f0)
    new = np.empty_like(flow)
    for c in range(len(flow)):
        u = flow[c]
        for _ in range(2):
            u = flow[c] + _dual_step(u, proj[c], dt, f1)
        new[c] = u
    return new


def constants(ndim, attachment, tightness):
    dt = 0.5 / ndim
    return attachment * tightness, dt / tightness, dt       # f0, f1, dt


def iterate(rho_0, grad, NI, flow, proj, n, attachment=15, tightness=0.3):
    """n fixed-point iterations from (flow, proj), which stay untouched -> (flow, proj)"""
    f0, f1, dt = constants(rho_0.ndim, attachment, tightness)
    flow, proj = flow.copy(), proj.copy()
    for _ in range(n):
        flow = _fixed_point(rho_0, grad, NI, flow, proj, f0, f1, dt)
    return flow, proj


def tvl1(reference, moving, flow0, attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4, prefilter=False, blocks=BLOCKS,
         record=None):
    """The solver on one level.  `record` (a list) receives per warp sum / (tol * size), the sum taken in double."""
    T = reference.dtype.type
    nd = reference.ndim
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=reference.dtype) for n in reference.shape], indexing="ij"))
    f0, f1, dt = constants(nd, attachment, tightness)
    limit = tol * reference.size
    current = previous = flow0.copy()
    proj = np.zeros((nd, nd) + reference.shape, reference.dtype)
    ratios = []
    for _ in range(num_warp):
        if prefilter:
            current = blocks["median"](current)             # a new array: `previous` stays the flow from before the median
        warped = blocks["warp"](moving, grid + current)
        grad, NI, rho_0 = prepare(warped, reference, current)
        for _ in range(num_iter):
            # the data term works in place: on the first iteration of a warp without prefilter that is `previous` too
            current = _fixed_point(rho_0, grad, NI, current, proj, f0, f1, dt)
        diff = previous - current
        sq = diff * diff
        ratios.append(float(sq.sum(dtype=np.float64)) / limit)
        if sq.sum() < limit:
            break
        previous = current
    if record is not None:
        record.append({"shape": reference.shape, "warps": len(ratios), "ratios": ratios})
    assert current.dtype.type is T
    return current


def coarse_to_fine(reference, moving, solver, downscale=2, nlevel=10, min_size=16, blocks=BLOCKS):
    levels = list(zip(get_pyramid(reference, downscale, nlevel, min_size, blocks), get_pyramid(moving, downscale, nlevel, min_size, blocks)))
    flow = np.zeros((reference.ndim,) + levels[0][0].shape, reference.dtype)
    flow = solver(levels[0][0], levels[0][1], flow)
    for r, m in levels[1:]:
        flow = solver(r, m, resize_flow(flow, r.shape, blocks))
    return flow


def optical_flow_tvl1(reference, moving, attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4, prefilter=False,
                      dtype=np.float32, blocks=BLOCKS, record=None):
    reference = np.asarray(reference).astype(dtype)
    moving = np.asarray(moving).astype(dtype)

    def solver(r, m, f):
        return tvl1(r, m, f, attachment, tightness, num_warp, num_iter, tol, prefilter, blocks, record)
    return coarse_to_fine(reference, moving, solver, blocks=blocks)


# ---------------------------------------------------------------- test inputs
def smooth_noise(shape, seed, sigma=2.0):
    """Gaussian-smoothed noise of unit standard deviation, float64"""
    x = sndi.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    return x / x.std()


def shifted_pair(shape, seed, shift, sigma=2.0):
    """(reference, moving): moving is the reference displaced by `shift` voxels along axis 0 (order-3 interpolation)"""
    ref = smooth_noise(shape, seed, sigma)
    mov = sndi.shift(ref, [shift] + [0] * (len(shape) - 1), order=3, mode="nearest")
    return ref, mov


def stage_inputs(shape, dtype, seed=3):
    """(warped, reference, flow, proj) for the stage tests: smooth images with a constant patch (NI == 0 there), a flow and
    a dual field of moderate size, so that both branches of the data term occur"""
    rng = np.random.default_rng(seed)
    ref = smooth_noise(shape, seed, 1.0)
    warped = ref + 0.3 * smooth_noise(shape, seed + 1, 1.0)
    patch = tuple(slice(0, max(2, n // 2)) for n in shape)
    warped[patch] = 0.25
    flow = 0.2 * rng.standard_normal((len(shape),) + tuple(shape))
    proj = 0.1 * rng.standard_normal((len(shape), len(shape)) + tuple(shape))
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (warped, ref, flow, proj))


def sin_case(shape=(256, 256), max_motion=4.5, npics=5):
    """(reference, moving, true flow), float64: white noise displaced along axis 0 by a sinusoid of axis 0 (the case of
    skimage's own test_tvl1.py)"""
    image0 = np.random.RandomState(0).normal(size=shape)
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")).astype(np.float64)
    flow = np.zeros_like(grid)
    flow[0] = max_motion * np.sin(grid[0] / grid[0].max() * npics * np.pi)
    return image0, warp_scipy(image0, grid - flow), flow


# (name, shape, seed, shift along axis 0, keyword arguments): the cases whose stopping decisions the GPU tests compare; the
# yardstick test admits them (every sum / (tol * size) outside [0.5, 2] in both dtypes at every level and warp)
STOP_CASES = [
    ("runs_out", (20, 24, 28), 11, 1.0, dict(prefilter=True)),
    ("stops_mid", (20, 24, 28), 11, 1.0, dict(prefilter=True, tol=0.3)),
    ("stops_mid_2d", (30, 32), 12, 1.0, dict(tol=0.2)),
    ("two_levels_2d", (40, 52), 13, 1.5, dict()),
    ("two_levels_3d", (40, 36, 44), 14, 1.5, dict(prefilter=True, tol=0.2)),
]


def stop_case(name, dtype):
    for n, shape, seed, shift, kw in STOP_CASES:
        if n == name:
            ref, mov = shifted_pair(shape, seed, shift)
            return ref.astype(dtype), mov.astype(dtype), dict(kw)
    raise KeyError(name)
