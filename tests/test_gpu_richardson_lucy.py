"""skimage.restoration.richardson_lucy on the device (csrc/richardson_lucy.hip) against the NumPy transcription of
tests/helpers/rl_ref.py under the three settings of mi_debug_set_richardson_lucy: the planner, the split route (rl_ratio_kernel +
rl_update_kernel) and the fused kernel on tiles of 3 x 5 outputs in chunks of 3 planes with a 16 KiB staging budget (seams along
every tiled axis, several chunks, rings that wrap).  The route is read back from last_kernel().

Every result must equal the transcription in bits; where the transcription is NaN, the result is NaN at the same positions."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from helpers import dirty_pool
from helpers import rl_ref as R

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rl_kat.json")))

ROUTES = {"planner": 0, "split": 1, "small": 2}
# x crossing a 64-lane wave with ragged rows, even and odd PSF lengths, a PSF larger than the image, PSF == image, fewer planes than
# the ring, unit PSF axes, rank 1 and rank 4 (split route only)
CASES = [((5, 7), (2, 3)), ((2, 9), (1, 4)), ((13, 67), (3, 5)), ((37, 70), (4, 5)), ((6, 6), (9, 9)), ((12, 12), (12, 12)),
         ((3, 5, 7), (2, 2, 3)), ((9, 21, 67), (3, 4, 5)), ((2, 18, 19), (5, 1, 4)), ((17, 18, 19), (9, 1, 8)),
         ((17,), (4,)), ((3, 4, 5, 6), (2, 1, 3, 2))]
CASE_IDS = ["x".join(map(str, i)) + "-" + "x".join(map(str, p)) for i, p in CASES]
SETTING_CASES = [2, 7, 8, 10]          # (13, 67), (9, 21, 67), (2, 18, 19), (17,): the cases every setting runs on


def planner_takes_fused(rank, T, pshape):
    """csrc/richardson_lucy.hip rl_planner_takes_fused: where the fused kernel was measured faster (profiles/richardson_lucy.txt)"""
    return rank in (2, 3)


@pytest.fixture(scope="module")
def rl(gpu):
    from cupyimg_amd.skimage.restoration import richardson_lucy
    return richardson_lucy


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_richardson_lucy
    fn.argtypes = [ctypes.c_int]
    yield lambda route: fn(ROUTES[route])
    fn(0)


def same(got, want):
    """equal bits, except that a NaN of the transcription only asks for a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(bits)[~nan], want.view(bits)[~nan]))


def check_route(gpu, route, ishape, pshape, T):
    name = gpu.last_kernel()
    rank, tname = len(ishape), np.dtype(T).name
    fused = rank in (2, 3) and (route == "small" or (route == "planner" and planner_takes_fused(rank, T, pshape)))
    if fused:
        assert "rl_fused_kernel<{},{}>".format(tname, rank) in name and "one launch" in name, (route, name)
        assert " ring={} ".format(pshape[0] if rank == 3 else 1) in name, (route, name)
        if route == "small":
            assert " tile=3x5 chunk=3 " in name, (route, name)
    else:
        nd = 3 if rank <= 3 else 8
        assert "rl_ratio_kernel<{0},{1}> + mi::rl_update_kernel<{0},{1}>".format(tname, nd) in name and "two launches" in name, (route, name)


def run(gpu, rl, knob, route, image, psf, iterations, clip=True, filter_epsilon=None, T=None):
    knob(route)
    out = rl(image, psf, iterations=iterations, clip=clip, filter_epsilon=filter_epsilon)
    if T is not None and iterations > 0:
        check_route(gpu, route, tuple(image.shape), tuple(psf.shape), T)
    assert out._is_c_contiguous()
    return out.get()


# ------------------------------------------------------------------ inputs and references, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def inputs(case, dtype, zero_taps=False):
    ishape, pshape = CASES[case]
    rng = np.random.default_rng(3000 + case)
    psf = rng.random(pshape) + 0.05
    if zero_taps:
        psf[rng.random(pshape) < 0.4] = 0.0
        psf.flat[-1] = 0.25
    psf /= psf.sum()
    image = rng.random(ishape) * 1.5 + 0.05                               # bright enough that results exceed 1
    image[tuple(slice(0, max(1, n // 3)) for n in ishape)] *= 1e-4        # a dark corner: some c fall below filter_epsilon
    if np.dtype(dtype).kind in "ui":
        image = np.round(image * 40)
    elif np.dtype(dtype).kind == "b":
        image = image > 0.6
    image, psf = image.astype(dtype), psf.astype(dtype if np.dtype(dtype).kind == "f" else np.float64)
    image.setflags(write=False)
    psf.setflags(write=False)
    return image, psf


@functools.lru_cache(maxsize=None)
def want(case, dtype, iterations, clip=True, filter_epsilon=None, zero_taps=False):
    image, psf = inputs(case, dtype, zero_taps)
    out = R.richardson_lucy(image, psf, iterations, clip, filter_epsilon)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ every case, route and float dtype
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_cases_equal_the_transcription(gpu, rl, knob, case, dtype, route):
    image, psf = inputs(case, dtype)
    got = run(gpu, rl, knob, route, gpu.asarray(image), psf, 3, True, 1e-3, T=dtype)
    assert got.dtype == np.dtype(dtype)
    assert same(got, want(case, dtype, 3, True, 1e-3))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("iterations", [0, 1, 2, 7])
@pytest.mark.parametrize("case", SETTING_CASES, ids=[CASE_IDS[c] for c in SETTING_CASES])
def test_iterations_hit_both_parities(gpu, rl, knob, case, iterations, route):
    image, psf = inputs(case, "float32")
    got = run(gpu, rl, knob, route, gpu.asarray(image), psf, iterations, T="float32")
    assert same(got, want(case, "float32", iterations))
    if iterations == 0:
        assert np.array_equal(got, np.full(image.shape, 0.5, np.float32))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("filter_epsilon", [None, 0, 1e-3, 0.2])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", SETTING_CASES, ids=[CASE_IDS[c] for c in SETTING_CASES])
def test_clip_and_filter_epsilon(gpu, rl, knob, case, dtype, clip, filter_epsilon, route):
    image, psf = inputs(case, dtype)
    free = want(case, dtype, 4, False, None)
    assert free.max() > 1.0                                               # the clip has something to clip
    if filter_epsilon == 0.2 or (filter_epsilon and case != 8):
        # the filter has something to filter (on two planes under a PSF of five, no c is as small as 1e-3, and all are below 0.2)
        assert not np.array_equal(want(case, dtype, 4, False, filter_epsilon), free)
    elif not filter_epsilon:
        assert same(want(case, dtype, 4, False, filter_epsilon), free)    # 0 is falsy, as in the reference
    got = run(gpu, rl, knob, route, gpu.asarray(image), psf, 4, clip, filter_epsilon, T=dtype)
    assert same(got, want(case, dtype, 4, clip, filter_epsilon))
    if clip:
        assert got.max() <= 1.0


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", [3, 9], ids=[CASE_IDS[3], CASE_IDS[9]])
@pytest.mark.parametrize("dtype, T", [("uint8", "float32"), ("uint16", "float32"), ("int32", "float64"), ("bool", "float32"), ("float16", "float32")])
def test_other_input_dtypes(gpu, rl, knob, dtype, T, case, route):
    image, psf = inputs(case, dtype)
    got = run(gpu, rl, knob, route, gpu.asarray(image), psf, 2, False, 1e-3, T=T)
    assert got.dtype == np.dtype(T)
    assert same(got, want(case, dtype, 2, False, 1e-3))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", [2, 7, 11], ids=[CASE_IDS[2], CASE_IDS[7], CASE_IDS[11]])
def test_psf_with_zero_taps(gpu, rl, knob, case, dtype, route):
    image, psf = inputs(case, dtype, True)
    assert (psf == 0).sum() >= 2
    got = run(gpu, rl, knob, route, gpu.asarray(image), psf, 3, T=dtype)
    assert same(got, want(case, dtype, 3, zero_taps=True))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", [2, 7, 10], ids=[CASE_IDS[2], CASE_IDS[7], CASE_IDS[10]])
def test_non_finite_data_and_an_all_zero_psf(gpu, rl, knob, case, dtype, route):
    image, psf = inputs(case, dtype)
    image = image.copy()
    image.flat[1], image.flat[image.size // 2], image.flat[-2] = np.nan, np.inf, -np.inf
    ref = R.richardson_lucy(image, psf, 2, True, None)
    assert not np.isfinite(ref).all()
    assert same(run(gpu, rl, knob, route, gpu.asarray(image), psf, 2, T=dtype), ref)
    for clip in (True, False):
        zero = np.zeros_like(psf)
        assert same(run(gpu, rl, knob, route, gpu.asarray(image), zero, 2, clip, T=dtype), R.richardson_lucy(image, zero, 2, clip))
        assert same(run(gpu, rl, knob, route, gpu.asarray(image), zero, 1, clip, 0.2, T=dtype), R.richardson_lucy(image, zero, 1, clip, 0.2))


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_psf_the_fused_kernel_refuses_takes_the_split_route(gpu, rl, knob, route):
    """float64 rings of a 31 x 31 PSF need 84 KiB with one output row of 64 columns (40 KiB with 5): more than either budget"""
    rng = np.random.default_rng(77)
    image, psf = rng.random((20, 21)) + 0.1, rng.random((31, 31))
    knob(route)
    got = rl(gpu.asarray(image), psf, iterations=2).get()
    assert "rl_ratio_kernel<float64,3>" in gpu.last_kernel(), gpu.last_kernel()
    assert same(got, R.richardson_lucy(image, psf, 2))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("k", range(len(KAT)))
def test_known_answers_bit_for_bit(gpu, rl, knob, k, route):
    image = np.array(KAT[k]["image"], np.float64).reshape(KAT[k]["shape"])
    psf = np.array(KAT[k]["psf"], np.float64).reshape(KAT[k]["psf_shape"])
    known = np.array(KAT[k]["want"], np.float64).reshape(KAT[k]["shape"])
    got = run(gpu, rl, knob, route, gpu.asarray(image), psf, KAT[k]["iterations"], KAT[k]["clip"], KAT[k]["filter_epsilon"], T="float64")
    assert np.array_equal(got.view(np.uint64), known.view(np.uint64))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", [2, 7], ids=[CASE_IDS[2], CASE_IDS[7]])
def test_placements_and_untouched_inputs(gpu, rl, knob, case, route):
    """device and host PSF, a non-contiguous view, an image at an offset in its allocation; the inputs stay as they were"""
    image, psf = inputs(case, "float32")
    ref = want(case, "float32", 3)
    dimage, dpsf = gpu.asarray(image), gpu.asarray(psf)
    assert same(run(gpu, rl, knob, route, dimage, dpsf, 3, T="float32"), ref)
    assert same(run(gpu, rl, knob, route, image, psf, 3), ref)                          # both on the host
    assert np.array_equal(dimage.get(), image) and np.array_equal(dpsf.get(), psf)
    wide = np.full(tuple(2 * n + 1 for n in image.shape), 7.0, np.float32)
    wide[tuple(slice(1, None, 2) for _ in image.shape)] = image
    dwide = gpu.asarray(wide)
    view = dwide[tuple(slice(1, None, 2) for _ in image.shape)]
    assert not view._is_c_contiguous()
    assert same(run(gpu, rl, knob, route, view, dpsf, 3), ref)
    assert np.array_equal(dwide.get(), wide)
    flat = np.full(image.size + 3, 7.0, np.float32)
    flat[3:] = image.ravel()
    dflat = gpu.asarray(flat)
    assert same(run(gpu, rl, knob, route, dflat[3:].reshape(image.shape), dpsf, 3, T="float32"), ref)
    assert np.array_equal(dflat.get(), flat)


@pytest.mark.parametrize("route", list(ROUTES))
def test_poisoned_pool_memory(gpu, rl, knob, route):
    image, psf = inputs(7, "float32")
    dimage = gpu.asarray(image)
    gpu.synchronize()
    for byte in dirty_pool.FILLS:
        with dirty_pool.pool_fill(gpu, byte):
            got = run(gpu, rl, knob, route, dimage, psf, 3, True, 1e-3, T="float32")
        assert same(got, want(7, "float32", 3, True, 1e-3)), hex(byte)


def test_empty_image(gpu, rl):
    out = rl(gpu.asarray(np.ones((0, 5), np.uint8)), np.ones((3, 3)))
    assert out.shape == (0, 5) and out.dtype == np.float32


@pytest.mark.parametrize("case", [3, 7], ids=[CASE_IDS[3], CASE_IDS[7]])
def test_burst_of_three_calls(gpu, rl, knob, case):
    image, psf = inputs(case, "float32")
    dimage = gpu.asarray(image)
    knob("planner")
    outs = [rl(dimage, psf, iterations=7) for _ in range(3)]
    first, last = outs[0].get(), outs[2].get()
    assert same(last, first) and same(first, want(case, "float32", 7))
