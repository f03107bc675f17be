"""skimage.restoration.denoise_tv_chambolle on the device (csrc/tv_chambolle.hip: mi_tv_chambolle_step / _output) against the
host transcription of tests/helpers/tv_ref.py, bit for bit: fixed iteration counts on shapes with ragged rows, rows longer
than a tile, axes of length 1 to 3 and seams on every axis, under the planner's tiles, forced small tiles and the forced
per-voxel kernel; the iteration at which the loop stops on the inputs tests/test_tv_yardstick.py admitted; repeatability;
dtypes, channels, views, host inputs and the error cases."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import tv_ref as tv

pytestmark = pytest.mark.gpu

# (tile rows, planes per chunk, 8-column tiles, generic kernel): the planner's tiles, small tiles (many seams), the generic kernel
SETTINGS = [(0, 0, 0, 0), (3, 2, 1, 0), (0, 0, 0, 1)]


@pytest.fixture(scope="module")
def rest(gpu):
    from cupyimg_amd.skimage import restoration
    return restoration


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_tv_chambolle
    fn.argtypes = [ctypes.c_int] * 4
    yield fn
    fn(0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def _image(shape, dtype, seed=1):
    x = tv.volume(shape, np.dtype(dtype), seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(shape, dtype, seed, weight, eps, n_iter_max):
    out, i, _ = tv.tv_chambolle(_image(shape, dtype, seed), weight=weight, eps=eps, n_iter_max=n_iter_max)
    out.setflags(write=False)
    return out, i


def _route(name, shape, dtype, setting):
    if setting[3] or len(shape) not in (2, 3):
        return "tv_generic_kernel<{}>".format(dtype) in name and "rank {}".format(len(shape)) in name
    kind = "volume" if len(shape) == 3 else "image"
    return "tv_fused_kernel<{},{}>".format(dtype, kind) in name and ("x8 " in name) == bool(setting[2])


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---------------------------------------------------------------- fixed iteration count, bit for bit
SHAPES = [(12, 20, 70), (9, 37, 64), (33, 18, 257), (3, 3, 3), (1, 1, 7), (2, 5, 1040), (70, 96), (5, 1040)]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_fixed_iterations_match_host_bit_for_bit(gpu, rest, knob, shape, dtype):
    from cupyimg_amd import last_kernel
    x = _image(shape, dtype)
    xd = gpu.asarray(x)
    for n in (1, 2, 7):
        want, i = _want(shape, dtype, 1, 0.2, 0.0, n)
        assert i == n
        for setting in SETTINGS:
            knob(*setting)
            got = rest.denoise_tv_chambolle(xd, weight=0.2, eps=0, n_iter_max=n)
            name = last_kernel()
            assert _route(name, shape, dtype, setting), (setting, name)
            assert got.dtype == np.dtype(dtype) and got.shape == shape
            assert np.array_equal(got.get(), want), (n, setting, name)
            assert rest.last_tv_iterations() == n


RANKS = [(50,), (5, 6, 7, 8), (3, 4, 3, 4, 5)]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", RANKS, ids=_ids(RANKS))
def test_other_ranks_take_the_generic_kernel(gpu, rest, shape, dtype):
    from cupyimg_amd import last_kernel
    xd = gpu.asarray(_image(shape, dtype))
    for n in (1, 2, 7):
        want, _ = _want(shape, dtype, 1, 0.2, 0.0, n)
        got = rest.denoise_tv_chambolle(xd, weight=0.2, eps=0, n_iter_max=n)
        assert _route(last_kernel(), shape, dtype, (0, 0, 0, 0)), last_kernel()
        assert np.array_equal(got.get(), want), n


# ---------------------------------------------------------------- stopping
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", tv.STOP_CASES, ids=lambda c: "{}-w{}".format("x".join(map(str, c[0])), c[1]))
def test_loop_stops_where_the_host_loop_stops(gpu, rest, knob, case, dtype):
    from cupyimg_amd import last_kernel
    shape, weight, seed = case
    want, i_stop = _want(shape, dtype, seed, weight, 2.0e-4, 200)
    assert 2 <= i_stop < 199
    xd = gpu.asarray(_image(shape, dtype, seed))
    for setting in SETTINGS:
        knob(*setting)
        got = rest.denoise_tv_chambolle(xd, weight=weight)
        assert _route(last_kernel(), shape, dtype, setting), (setting, last_kernel())
        assert rest.last_tv_iterations() == i_stop, setting
        assert np.array_equal(got.get(), want), setting


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_loop_runs_out_before_the_natural_stop(gpu, rest, knob, dtype):
    shape, weight, seed = tv.STOP_CASES[0]
    assert _want(shape, dtype, seed, weight, 2.0e-4, 200)[1] > 20
    xd = gpu.asarray(_image(shape, dtype, seed))
    for n in (10, 17):                                  # inside the first batch of queued iterations, and one past it
        want, i = _want(shape, dtype, seed, weight, 2.0e-4, n)
        assert i == n
        for setting in SETTINGS:
            knob(*setting)
            got = rest.denoise_tv_chambolle(xd, weight=weight, n_iter_max=n)
            assert rest.last_tv_iterations() == n
            assert np.array_equal(got.get(), want), (n, setting)


@pytest.mark.parametrize("shape", [(33, 18, 130), (40, 96), (5, 6, 7, 8)], ids=_ids([(33, 18, 130), (40, 96), (5, 6, 7, 8)]))
def test_same_call_twice_gives_the_same_bits(gpu, rest, shape):
    xd = gpu.asarray(_image(shape, "float32"))
    a = rest.denoise_tv_chambolle(xd, weight=0.15)
    ia = rest.last_tv_iterations()
    b = rest.denoise_tv_chambolle(xd, weight=0.15)
    assert rest.last_tv_iterations() == ia and 1 <= ia < 200
    assert np.array_equal(a.get(), b.get())
    assert not gpu.shares_memory(a, b)


# ---------------------------------------------------------------- dtypes
def _integer_image(shape, dtype):
    x = np.clip(tv.volume(shape) / 1.6, 0.0, 1.0)
    if dtype == "bool":
        return x > 0.5
    if dtype == "uint8":
        return np.round(x * 255).astype(np.uint8)
    return np.round((x * 2 - 1) * 30000).astype(np.int16)


@pytest.mark.parametrize("dtype", ["uint8", "int16", "bool"])
def test_integer_images_go_through_img_as_float(gpu, rest, dtype):
    from cupyimg_amd.skimage.filters import _img_as_float
    x = _integer_image((9, 20, 70), dtype)
    xd = gpu.asarray(x)
    scaled = _img_as_float(xd).get()
    assert scaled.dtype == np.float64
    ideal = {"uint8": lambda v: v / 255.0, "int16": lambda v: (2.0 * v + 1.0) / 65535.0, "bool": lambda v: v}[dtype](x.astype(np.float64))
    assert np.allclose(scaled, ideal, rtol=0, atol=1e-15)
    want, i_stop, _ = tv.tv_chambolle(scaled, weight=0.1, n_iter_max=12)
    got = rest.denoise_tv_chambolle(xd, weight=0.1, n_iter_max=12)
    assert got.dtype == np.float64
    assert np.array_equal(got.get(), want)
    assert np.array_equal(xd.get(), x)


def test_float16_is_computed_in_float32(gpu, rest):
    x = tv.volume((9, 20, 70)).astype(np.float16)
    want = tv.tv_chambolle(x.astype(np.float32), weight=0.1, n_iter_max=12)[0].astype(np.float16)
    for src in (gpu.asarray(x), x):
        got = rest.denoise_tv_chambolle(src, weight=0.1, n_iter_max=12)
        assert got.dtype == np.float16
        assert np.array_equal(got.get(), want)


def test_complex_is_refused(gpu, rest):
    with pytest.raises(TypeError):
        rest.denoise_tv_chambolle(np.ones((4, 5), np.complex64))
    with pytest.raises(TypeError):
        rest.denoise_tv_chambolle(np.ones((4, 5), np.complex128), multichannel=True)


# ---------------------------------------------------------------- channels, views, host inputs
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_multichannel_is_every_channel_on_its_own(gpu, rest, dtype):
    x = _image((20, 33, 3), dtype)
    xd = gpu.asarray(x)
    whole = rest.denoise_tv_chambolle(xd, weight=0.1, multichannel=True)
    its = rest.last_tv_iterations()
    assert isinstance(its, list) and len(its) == 3
    assert whole.shape == x.shape and whole.dtype == x.dtype
    whole = whole.get()
    for c in range(3):
        own = rest.denoise_tv_chambolle(gpu.asarray(np.ascontiguousarray(x[..., c])), weight=0.1)
        assert rest.last_tv_iterations() == its[c]
        assert np.array_equal(whole[..., c], own.get())
        want, i, _ = tv.tv_chambolle(np.ascontiguousarray(x[..., c]), weight=0.1, n_iter_max=9)
        got = rest.denoise_tv_chambolle(xd[..., c], weight=0.1, n_iter_max=9)
        assert np.array_equal(got.get(), want)
    fixed = rest.denoise_tv_chambolle(xd, weight=0.1, n_iter_max=9, multichannel=True).get()
    assert rest.last_tv_iterations() == [9, 9, 9]
    for c in range(3):
        assert np.array_equal(fixed[..., c], tv.tv_chambolle(np.ascontiguousarray(x[..., c]), weight=0.1, n_iter_max=9)[0])


def test_views_and_host_arrays(gpu, rest):
    base = _image((24, 20, 70), "float32")
    bd = gpu.asarray(base)
    view = bd[::2, :, 3:67]
    hv = np.ascontiguousarray(base[::2, :, 3:67])
    want = tv.tv_chambolle(hv, weight=0.2, n_iter_max=9)[0]
    got = rest.denoise_tv_chambolle(view, weight=0.2, n_iter_max=9)
    assert got.shape == (12, 20, 64)
    assert np.array_equal(got.get(), want)
    assert not gpu.shares_memory(got, bd)
    assert np.array_equal(bd.get(), base)

    img = _image((40, 96), "float64")
    idv = gpu.asarray(img)
    want_t = tv.tv_chambolle(np.ascontiguousarray(img.T), weight=0.2, n_iter_max=9)[0]
    got_t = rest.denoise_tv_chambolle(idv.T, weight=0.2, n_iter_max=9)
    assert got_t.shape == (96, 40)
    assert np.array_equal(got_t.get(), want_t)
    assert np.array_equal(idv.get(), img)

    want_h = tv.tv_chambolle(img, weight=0.2, n_iter_max=9)[0]
    got_h = rest.denoise_tv_chambolle(np.array(img), weight=0.2, n_iter_max=9)
    assert isinstance(got_h, gpu.ndarray)
    assert np.array_equal(got_h.get(), want_h)
    got_l = rest.denoise_tv_chambolle(img.tolist(), weight=0.2, n_iter_max=9)
    assert np.array_equal(got_l.get(), want_h)

    # a contiguous device input is used in place, never written and never returned
    same = rest.denoise_tv_chambolle(idv, weight=0.2, n_iter_max=1)
    assert np.array_equal(same.get(), img) and not gpu.shares_memory(same, idv)
    assert np.array_equal(idv.get(), img)


# ---------------------------------------------------------------- errors
def test_errors_and_empty_arrays(gpu, rest):
    x = gpu.asarray(_image((6, 7), "float32"))
    for n in (0, -3):
        with pytest.raises(ValueError):
            rest.denoise_tv_chambolle(x, n_iter_max=n)
    with pytest.raises(ValueError):
        rest.denoise_tv_chambolle(gpu.asarray(np.ones(5, np.float32)), multichannel=True)
    for dtype, res in (("float32", "float32"), ("float64", "float64"), ("uint8", "float64"), ("float16", "float16")):
        out = rest.denoise_tv_chambolle(gpu.asarray(np.zeros((0, 5), dtype)))
        assert out.shape == (0, 5) and out.dtype == np.dtype(res)
    out = rest.denoise_tv_chambolle(np.zeros((4, 0, 3), np.float32), multichannel=True)
    assert out.shape == (4, 0, 3) and rest.last_tv_iterations() == [0, 0, 0]
