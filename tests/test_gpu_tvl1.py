"""skimage.registration.optical_flow_tvl1 on the device (csrc/tvl1.hip: mi_tvl1_*) against the host transcription of
tests/helpers/tvl1_ref.py, bit for bit: the stage kernels on shapes with ragged rows, rows longer than a tile, axes of
length 2 and 3 and seams on every axis, under the planner's tiles, forced small tiles and the forced per-voxel kernels; the
whole solver and the whole call against the transcription with this library's existing interpolation and filters plugged
in, stopping decisions and the prefilter path included, on the cases tests/test_tvl1_yardstick.py admitted; resize and the
pyramid steps against SciPy; dtypes, host and integer inputs, views, repeatability and the error cases."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import tvl1_ref as R

pytestmark = pytest.mark.gpu

# (small tiles, per-voxel kernels): the planner's tiles, tiles of 3 x 8 voxels in chunks of 3 planes, the per-voxel route
SETTINGS = [(0, 0), (1, 0), (0, 1)]


@pytest.fixture(scope="module")
def reg(gpu):
    from cupyimg_amd.skimage import registration
    return registration


@pytest.fixture(scope="module")
def tf(gpu):
    from cupyimg_amd.skimage import transform
    return transform


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_tvl1
    fn.argtypes = [ctypes.c_int] * 2
    yield fn
    fn(0, 0)


def _route(name, shape, dtype, setting):
    if setting[1] or len(shape) not in (2, 3):
        return "tvl1_step_kernels<{}>".format(dtype) in name and "rank {}".format(len(shape)) in name
    kind = "volume" if len(shape) == 3 else "image"
    return "tvl1_reg_fused_kernel<{},{}>".format(dtype, kind) in name and ("x8 chunk" in name) == bool(setting[0])


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---------------------------------------------------------------- stage kernels, bit for bit
SHAPES = [(12, 20, 70), (9, 37, 64), (33, 18, 257), (3, 3, 3), (2, 5, 1040), (70, 96), (5, 1040), (2, 2), (5, 6, 7, 8)]


@functools.lru_cache(maxsize=None)
def _stage(shape, dtype):
    """inputs and the transcription's results, computed once"""
    warped, ref, flow, proj = R.stage_inputs(shape, np.dtype(dtype).type)
    grad, NI, rho_0 = R.prepare(warped, ref, flow)
    want = {n: R.iterate(rho_0, grad, NI, flow, proj, n) for n in (1, 2, 7)}
    for a in (warped, ref, flow, proj, grad, NI, rho_0):
        a.setflags(write=False)
    return warped, ref, flow, proj, np.ascontiguousarray(grad), NI, rho_0, want


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_prepare_matches_host_bit_for_bit(gpu, reg, shape, dtype):
    warped, ref, flow, proj, grad, NI, rho_0, _ = _stage(shape, dtype)
    g, n, r = reg._prepare(gpu.asarray(warped), gpu.asarray(ref), gpu.asarray(flow))
    assert "tvl1_prepare_kernel<{}>".format(dtype) in gpu.last_kernel()
    assert np.array_equal(g.get(), grad)
    assert np.array_equal(n.get(), NI)
    assert np.array_equal(r.get(), rho_0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_fixed_point_iterations_match_host_bit_for_bit(gpu, reg, knob, shape, dtype):
    warped, ref, flow, proj, grad, NI, rho_0, want = _stage(shape, dtype)
    dev = [gpu.asarray(a) for a in (rho_0, grad, NI, flow, proj)]
    for n in (1, 2, 7):
        for setting in SETTINGS:
            knob(*setting)
            f, p, launches = reg._iterate(*dev, n)
            name = gpu.last_kernel()
            assert _route(name, shape, dtype, setting), (setting, name)
            fused = "fused" in name
            assert launches == (2 if fused else 5) * n
            assert np.array_equal(f.get(), want[n][0]), (n, setting, name)
            assert np.array_equal(p.get(), want[n][1]), (n, setting, name)
    # the inputs are left alone
    assert np.array_equal(dev[3].get(), flow) and np.array_equal(dev[4].get(), proj)


def test_axis_of_length_one_raises(gpu, reg):
    """numpy.gradient's rule (the reference raises there too)"""
    for shape in [(1, 8, 8), (8, 1), (4, 4, 1)]:
        x = gpu.asarray(np.zeros(shape, np.float32))
        f = gpu.asarray(np.zeros((len(shape),) + shape, np.float32))
        with pytest.raises(ValueError):
            reg._prepare(x, x, f)
        with pytest.raises(ValueError):
            reg.optical_flow_tvl1(x, x)


# ---------------------------------------------------------------- the whole solver and the whole call
def _device_blocks(gpu):
    """the transcription's building blocks as this library's existing public functions, called as the product calls them"""
    from cupyimg_amd.scipy import ndimage as ndi

    def warp(image, coords):
        out = ndi.map_coordinates(gpu.asarray(image), gpu.asarray(np.ascontiguousarray(coords)), order=1, mode="nearest").get()
        return np.clip(out, image.min(), image.max())

    def gaussian(image, sigma, mode, cval):
        d = gpu.asarray(image)
        out = gpu.empty_like(d)
        ndi.gaussian_filter(d, sigma, output=out, mode=mode, cval=cval)
        return out.get()

    def zoom0(flow, factors):
        return ndi.zoom(gpu.asarray(flow), factors, order=0, mode="nearest", prefilter=False).get()

    def median(flow):
        return np.stack([ndi.median_filter(gpu.asarray(np.ascontiguousarray(c)), size=3).get() for c in flow])

    def interp(image, factors, output_shape, order, mode, cval):
        return ndi.affine_transform(gpu.asarray(image), np.diag(factors), offset=0.5 * factors - 0.5, output_shape=output_shape,
                                    order=order, mode=mode, cval=cval).get()

    return R.blocks(warp=warp, gaussian=gaussian, zoom0=zoom0, median=median, interp=interp)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", [c[0] for c in R.STOP_CASES])
def test_whole_call_matches_transcription_bit_for_bit(gpu, reg, knob, case, dtype):
    T = np.dtype(dtype).type
    ref, mov, kw = R.stop_case(case, T)
    rec = []
    want = R.optical_flow_tvl1(ref, mov, dtype=T, blocks=_device_blocks(gpu), record=rec, **kw)
    print(case, dtype, rec)
    for setting in SETTINGS:
        knob(*setting)
        got = reg.optical_flow_tvl1(gpu.asarray(ref), gpu.asarray(mov), dtype=T, **kw)
        stats = reg.last_tvl1_stats()
        assert got.dtype == np.dtype(dtype) and got.shape == want.shape
        assert [(s["shape"], s["warps"]) for s in stats] == [(r["shape"], r["warps"]) for r in rec], (setting, stats)
        for s in stats:
            assert s["iterations"] == 10 * s["warps"]
            assert s["launches"] == (5 if setting[1] else 2) * s["iterations"], (setting, s)
        assert np.array_equal(got.get(), want), (case, setting)


@pytest.mark.parametrize("prefilter", [False, True])
def test_solver_on_one_level_matches_transcription(gpu, reg, prefilter):
    """`_tvl1` from a non-zero initial flow, few iterations: flow_previous with and without the median"""
    ref, mov, _ = R.stop_case("runs_out", np.float32)
    flow0 = (0.3 * np.random.default_rng(5).standard_normal((3,) + ref.shape)).astype(np.float32)
    args = dict(attachment=15, tightness=0.3, num_warp=3, num_iter=2, tol=1e-4, prefilter=prefilter)
    rec = []
    want = R.tvl1(ref, mov, flow0, blocks=_device_blocks(gpu), record=rec, **args)
    got = reg._tvl1(gpu.asarray(ref), gpu.asarray(mov), gpu.asarray(flow0), **args)
    assert reg.last_tvl1_stats()[-1]["warps"] == rec[0]["warps"]
    assert np.array_equal(got.get(), want)


# ---------------------------------------------------------------- resize and the pyramid steps against SciPy
def _relerr(got, want):
    return np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()


RESIZE = [((37, 52), (19, 26)), ((36, 50), (18, 25)), ((21, 30), (40, 61)), ((13, 18, 22), (7, 9, 11)), ((12, 9, 10), (24, 17, 21)),
          ((5, 6, 7, 8), (3, 3, 4, 4))]


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-6)])
@pytest.mark.parametrize("shapes", RESIZE, ids=["{}to{}".format("x".join(map(str, a)), "x".join(map(str, b))) for a, b in RESIZE])
def test_resize_matches_scipy(gpu, tf, shapes, dtype, tol):
    src, dst = shapes
    x = R.smooth_noise(src, 21, 1.0).astype(dtype)
    for aa in (False, True):
        got = tf.resize(gpu.asarray(x), dst, anti_aliasing=aa)
        want = R.resize(x.astype(np.float64), dst, anti_aliasing=aa)
        assert got.shape == dst and got.dtype == np.dtype(dtype)
        err = _relerr(got.get(), want)
        print(shapes, dtype, aa, err)
        assert err <= tol


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-6)])
def test_resize_multichannel_and_options(gpu, tf, dtype, tol):
    x = R.smooth_noise((20, 31, 3), 22, 1.0).astype(dtype)
    got = tf.resize(gpu.asarray(x), (11, 15))
    want = R.resize(x.astype(np.float64), (11, 15))
    assert got.shape == (11, 15, 3)
    assert _relerr(got.get(), want) <= tol
    # every channel is resized on its own
    one = tf.resize(gpu.asarray(np.ascontiguousarray(x[..., 1])), (11, 15)).get()
    assert _relerr(got.get()[..., 1], one.astype(np.float64)) <= tol
    # appended axes, an explicit sigma, other modes, order 0, no clipping
    y = x[..., 0]
    assert tf.resize(gpu.asarray(y), (10, 16, 1)).shape == (10, 16, 1)
    for kw in (dict(anti_aliasing_sigma=1.5), dict(mode="edge"), dict(mode="constant", cval=9.0), dict(order=0, anti_aliasing=False),
               dict(clip=False)):
        got = tf.resize(gpu.asarray(y), (9, 14), **kw)
        rkw = dict(kw)
        want = R.resize(y.astype(np.float64), (9, 14), **dict(dict(order=1), **rkw))
        assert _relerr(got.get(), want) <= tol, kw


def test_resize_errors(gpu, tf):
    x = gpu.asarray(np.zeros((8, 9, 3), np.float32))
    with pytest.raises(ValueError):
        tf.resize(x, (4,))
    with pytest.raises(ValueError):
        tf.resize(x, (4, 4), mode="nearest")
    with pytest.raises(ValueError):
        tf.resize(x, (4, 4), anti_aliasing_sigma=-1.0)
    with pytest.raises(ValueError):
        tf.resize(x, (4, 4), order=6)
    with pytest.raises(ValueError):
        tf.pyramid_reduce(x, downscale=1)
    with pytest.raises(ValueError):
        tf.pyramid_expand(x, upscale=0.5)


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-6)])
@pytest.mark.parametrize("shape", [(37, 52), (36, 50), (13, 18, 22)], ids=_ids([(37, 52), (36, 50), (13, 18, 22)]))
def test_pyramid_steps_match_scipy(gpu, tf, shape, dtype, tol):
    x = R.smooth_noise(shape, 23, 1.0).astype(dtype)
    got = tf.pyramid_reduce(gpu.asarray(x))
    want = R.pyramid_reduce(x.astype(np.float64))
    assert got.shape == tuple(-(-n // 2) for n in shape) and got.dtype == np.dtype(dtype)
    assert _relerr(got.get(), want) <= tol
    got = tf.pyramid_expand(gpu.asarray(x))
    want = R.pyramid_expand(x.astype(np.float64))
    assert got.shape == tuple(2 * n for n in shape)
    assert _relerr(got.get(), want) <= tol
    if len(shape) == 3:
        got = tf.pyramid_reduce(gpu.asarray(x), multichannel=True)
        want = R.pyramid_reduce(x.astype(np.float64), multichannel=True)
        assert got.shape == want.shape == (7, 9, 22)
        assert _relerr(got.get(), want) <= tol


# ---------------------------------------------------------------- public behaviour
@pytest.mark.parametrize("shape", [(40, 44), (24, 20, 28), (5, 6, 7, 8)], ids=["2d", "3d", "4d"])
def test_identical_images_give_zeros(gpu, reg, shape):
    x = gpu.asarray(np.random.RandomState(0).normal(size=shape))
    for dtype in (np.float32, np.float64):
        flow = reg.optical_flow_tvl1(x, x, dtype=dtype)
        assert flow.shape == (len(shape),) + shape and flow.dtype == dtype
        assert np.all(flow.get() == 0)


def test_sinusoidal_case_meets_skimage_criterion(gpu, reg):
    ref, mov, truth = R.sin_case()
    f32 = reg.optical_flow_tvl1(gpu.asarray(ref), gpu.asarray(mov), attachment=5).get()
    f64 = reg.optical_flow_tvl1(gpu.asarray(ref), gpu.asarray(mov), attachment=5, dtype=np.float64).get()
    assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.shape == (2, 256, 256)
    print(np.abs(f32 - truth).mean(), np.abs(f64 - truth).mean(), np.abs(f64 - f32).mean())
    assert np.abs(f32 - truth).mean() < 0.5
    assert np.abs(f64 - truth).mean() < 0.5
    assert np.abs(f64 - f32).mean() < 1e-3


def test_inputs_of_every_kind(gpu, reg):
    ref, mov, kw = R.stop_case("stops_mid_2d", np.float32)
    want = reg.optical_flow_tvl1(gpu.asarray(ref), gpu.asarray(mov), **kw).get()
    # host arrays, and the same call again: identical bits
    assert np.array_equal(reg.optical_flow_tvl1(ref, mov, **kw).get(), want)
    # float64 input, float32 result: the conversion is a cast
    assert np.array_equal(reg.optical_flow_tvl1(ref.astype(np.float64), mov, **kw).get(), want)
    # non-contiguous views; the caller's arrays stay as they are
    big = np.zeros((60, 64), np.float32)
    big[::2, ::2] = ref
    bigd = gpu.asarray(big)
    movd = gpu.asarray(mov)
    got = reg.optical_flow_tvl1(bigd[::2, ::2], movd, **kw)
    assert np.array_equal(got.get(), want)
    assert np.array_equal(bigd.get(), big) and np.array_equal(movd.get(), mov)
    # integer images are scaled as skimage's _convert scales them
    lo, hi = min(ref.min(), mov.min()), max(ref.max(), mov.max())
    for idt in (np.uint8, np.int16, np.uint16, np.int32):
        info = np.iinfo(idt)
        q = [np.round((a - lo) / (hi - lo) * 200).astype(idt) for a in (ref, mov)]
        for dtype in (np.float32, np.float64):
            comp = dtype if np.dtype(dtype).itemsize >= np.dtype(idt).itemsize else np.float64
            if info.min == 0:
                conv = [np.multiply(a, 1.0 / info.max, dtype=comp).astype(dtype) for a in q]
            else:
                conv = []
                for a in q:
                    c = np.add(a, 0.5, dtype=comp)
                    c *= 2 / (int(info.max) - int(info.min))
                    conv.append(c.astype(dtype))
            got = reg.optical_flow_tvl1(q[0], q[1], dtype=dtype, num_warp=2, num_iter=3).get()
            ref_flow = reg.optical_flow_tvl1(conv[0], conv[1], dtype=dtype, num_warp=2, num_iter=3).get()
            assert got.dtype == dtype and np.array_equal(got, ref_flow), (idt, dtype)


def test_error_cases(gpu, reg):
    x = np.zeros((20, 24), np.float32)
    with pytest.raises(ValueError):
        reg.optical_flow_tvl1(x, np.zeros((20, 25), np.float32))
    for bad in (np.float16, np.longdouble, np.int32):
        with pytest.raises(ValueError):
            reg.optical_flow_tvl1(x, x, dtype=bad)
    with pytest.raises(ValueError):
        reg.optical_flow_tvl1(np.zeros(30, np.float32), np.zeros(30, np.float32))
    with pytest.raises(ValueError):
        reg.optical_flow_tvl1(np.zeros((3,) * 5, np.float32), np.zeros((3,) * 5, np.float32))
    with pytest.raises(ValueError):
        reg.optical_flow_tvl1(x, x, num_warp=0)
    with pytest.raises(ValueError):
        reg.optical_flow_tvl1(x, x, num_iter=0)
    with pytest.raises(TypeError):
        reg.optical_flow_tvl1(x.astype(np.complex64), x)
