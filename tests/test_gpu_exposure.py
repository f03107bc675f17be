"""skimage.exposure on the device (csrc/exposure.hip) against the host transcription of tests/helpers/exposure_ref.py, which
tests/test_exposure_yardstick.py checks: equalize_adapthist bit for bit under the planner's route, the forced per-voxel
kernel and the forced shared histogram, on shapes that are ragged on every axis, with regions of one voxel, pads longer than
the axis, ranks 1 to 4, every dtype, views and host inputs; the mappings alone region by region; equalize_hist, histogram,
cumulative_distribution and rescale_intensity."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from helpers import exposure_ref as er

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exposure_kat.json")))

# (force_generic, force_shared_hist)
SETTINGS = [(0, 0), (1, 0), (0, 1)]


@pytest.fixture(scope="module")
def exposure(gpu):
    from cupyimg_amd.skimage import exposure
    return exposure


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_clahe
    fn.argtypes = [ctypes.c_int] * 2
    yield fn
    fn(0, 0)


@functools.lru_cache(maxsize=None)
def _image(shape, dtype, seed=1, flat_corner=False):
    x = er.volume(shape, np.dtype(dtype), seed, flat_corner)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(shape, dtype, seed, flat_corner, kernel, clip_limit, nbins):
    out = er.equalize_adapthist(_image(shape, dtype, seed, flat_corner), kernel, clip_limit, nbins)
    out.setflags(write=False)
    return out


def _apply_route(name, shape, kernel, nbins, dtype, setting):
    """the route mi_clahe_apply documents: ranks 2 and 3 with at most 64 KiB of mappings per cell and sum(kernel) <= 1024"""
    nd = len(shape)
    k = er.kernel_of(shape, kernel)
    fast = not setting[0] and nd in (2, 3) and (nbins << nd) * 2 <= 65536 and sum(k) <= 1024
    if not fast:
        return "clahe_generic_kernel<{},{}>".format(dtype, nd) in name
    slabs = SLABS.get((shape, kernel), 1)
    return "clahe_apply_kernel<{},{}>".format(dtype, nd) in name and " slabs={} ".format(slabs) in name


def _maps_route(name, nbins, dtype, setting):
    private = nbins <= 1024 and not setting[1]
    return "clahe_maps_kernel<{}>".format(dtype) in name and ("per-wave histograms" if private else "shared histogram") in name


# (shape, kernel_size, clip_limit, nbins, dtype)
CASES = [
    ((20, 33, 70), (5, 8, 16), 0.01, 256, "uint16"),
    ((9, 37, 64), (4, 9, 8), 0.02, 128, "float32"),          # ragged on every axis
    ((33, 18, 257), (8, 8, 64), 0.01, 256, "uint16"),
    ((33, 18, 257), (8, 8, 64), 0.01, 16384, "uint16"),      # one shared histogram; mappings too large to stage
    ((16, 16, 16), 2, 0.01, 256, "uint8"),
    ((3, 3, 3), 1, 0.01, 256, "uint16"),
    ((2, 5, 1040), (1, 2, 130), 0.01, 256, "float64"),
    ((1, 1, 7), 1, 0.01, 256, "uint16"),
    ((9, 8), 8, 0.01, 256, "uint8"),                         # the pad exceeds the axis: reflection bounces more than once
    ((17, 19), (4, 5), 0.01, 256, "uint16"),
    ((40, 70), (8, 16), 0.05, 64, "float32"),
    ((64, 64), None, 0.01, 256, "uint16"),
    ((30, 50), 7, 0, 256, "uint8"),
    ((50,), 7, 0.1, 16, "uint16"),
    ((5, 6, 7, 8), (2, 3, 3, 4), 0.01, 32, "float64"),
    ((30, 40), 10, 0.01, 16, "uint8"),                       # clip limit 1: the loop ends by the round that changes nothing
    # regions of more than 4096 voxels in few cells: the blend splits every cell into slabs along axis 0 (SLABS below)
    ((34, 40, 70), (17, 16, 32), 0.01, 256, "uint16"),       # 6 + 6 + 5 planes
    ((11, 60, 100), (5, 56, 56), 0.01, 256, "float32"),      # 4 slabs wanted, 2 + 2 + 1 planes made
    ((96, 200), (48, 100), 0.01, 256, "uint8"),
    ((90, 500), (40, 400), 0.02, 128, "float64"),
]

# slabs per interpolation cell that mi_clahe_apply plans, by hand from its rule: want = min(ceil(8192 / cells),
# ceil(prod(kernel) / 4096), kernel[0]) slabs of ceil(kernel[0] / want) planes, cells = prod(regions + 1); every other case
# has regions of at most 4096 voxels and one slab
SLABS = {
    ((34, 40, 70), (17, 16, 32)): 3,       # 48 cells, 8704 voxels: 3 wanted, 6 planes each
    ((11, 60, 100), (5, 56, 56)): 3,       # 36 cells, 15680 voxels: 4 wanted, 2 planes each, which makes 3
    ((96, 200), (48, 100)): 2,             # 9 cells, 4800 voxels: 2 wanted, 24 rows each
    ((90, 500), (40, 400)): 4,             # 12 cells, 16000 voxels: 4 wanted, 10 rows each
}


def _case_id(c):
    return "{}-k{}-c{}-b{}-{}".format("x".join(map(str, c[0])), c[1] if not isinstance(c[1], tuple) else "x".join(map(str, c[1])),
                                      c[2], c[3], c[4])


def _clahe(exposure, shape):
    """The public function; for the one case whose shape, (3, 3, 3), the public function takes for an RGB image and refuses
    (the documented deviation, asserted in test_rgb_shaped_volume_is_refused_in_public), the grey-level body behind it, as the
    reference has it behind its adapt_rgb decorator."""
    if len(shape) == 3 and shape[-1] in (3, 4):
        return exposure._adapthist_grey
    return exposure.equalize_adapthist


def test_rgb_shaped_volume_is_refused_in_public(gpu, exposure):
    with pytest.raises(NotImplementedError, match="colour"):
        exposure.equalize_adapthist(gpu.asarray(_image((3, 3, 3), "uint16")), kernel_size=1)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_equalize_adapthist_matches_host_bit_for_bit(gpu, exposure, knob, case):
    from cupyimg_amd import last_kernel
    shape, kernel, clip_limit, nbins, dtype = case
    seed = 2 if shape == (30, 40) else 1
    xd = gpu.asarray(_image(shape, dtype, seed))
    want = _want(shape, dtype, seed, False, kernel, clip_limit, nbins)
    for setting in SETTINGS:
        knob(*setting)
        got = _clahe(exposure, shape)(xd, kernel_size=kernel, clip_limit=clip_limit, nbins=nbins)
        assert got.dtype == np.float64 and got.shape == shape
        assert_array_equal(got.get(), want, err_msg=str(setting))
        # the route of the maps launch
        exposure._clahe_maps(exposure._clahe_plan(xd, kernel, clip_limit, nbins))
        assert _maps_route(last_kernel(), nbins, dtype, setting), (setting, last_kernel())


@pytest.mark.parametrize("flat_corner", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_all_dtypes_on_both_volume_variants(gpu, exposure, knob, dtype, flat_corner):
    shape, kernel = (20, 33, 70), (5, 8, 16)
    xd = gpu.asarray(_image(shape, dtype, 1, flat_corner))
    want = _want(shape, dtype, 1, flat_corner, kernel, 0.01, 256)
    for setting in SETTINGS:
        knob(*setting)
        assert_array_equal(exposure.equalize_adapthist(xd, kernel_size=kernel).get(), want, err_msg=str(setting))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ((20, 33, 70), (33, 18, 257), (17, 19), (50,), (5, 6, 7, 8))
                                  or (c[0], c[1]) in SLABS], ids=_case_id)
def test_apply_route_names(gpu, exposure, knob, case):
    """the blend launched on its own, so that the note is that of mi_clahe_apply whatever the launches around it do; the
    slab cases must split their cells (and are held to the host bit for bit above, under the same planner)"""
    from cupyimg_amd import last_kernel
    shape, kernel, clip_limit, nbins, dtype = case
    xd = gpu.asarray(_image(shape, dtype))
    for setting in SETTINGS:
        knob(*setting)
        plan = exposure._clahe_plan(xd, kernel, clip_limit, nbins)
        maps = exposure._clahe_maps(plan)
        exposure._clahe_apply(plan, maps)
        assert _apply_route(last_kernel(), shape, kernel, nbins, dtype, setting), (setting, last_kernel())


@pytest.mark.parametrize("case", [c for c in CASES if (c[0], c[1]) in SLABS], ids=_case_id)
def test_blend_in_slabs_alone(gpu, exposure, knob, case):
    """the uint16 result of the blend before the final rescale, and the min and max it leaves on the device, with every
    cell in more than one slab: a voxel missed or written twice at a slab edge shows here as itself"""
    from cupyimg_amd import last_kernel
    shape, kernel, clip_limit, nbins, dtype = case
    x = _image(shape, dtype)
    b, maps = er.clahe_maps(x, kernel, clip_limit, nbins)
    want = er.blend(b, maps, er.kernel_of(shape, kernel))
    plan = exposure._clahe_plan(gpu.asarray(x), kernel, clip_limit, nbins)
    v, work = exposure._clahe_apply(plan, exposure._clahe_maps(plan))
    assert " slabs={} ".format(SLABS[(shape, kernel)]) in last_kernel(), last_kernel()
    assert v.dtype == np.uint16
    assert_array_equal(v.get(), want)
    lo, inv_hi = work.get().view(np.uint32)[:2]
    assert (int(lo), 65535 - int(inv_hi)) == (int(want.min()), int(want.max()))


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3], CASES[8], CASES[15]], ids=_case_id)
def test_maps_alone_region_by_region(gpu, exposure, knob, case):
    shape, kernel, clip_limit, nbins, dtype = case
    seed = 2 if shape == (30, 40) else 1
    x = _image(shape, dtype, seed)
    _, want = er.clahe_maps(x, kernel, clip_limit, nbins)
    want = want.reshape(-1, nbins)
    for setting in SETTINGS:
        knob(*setting)
        got = exposure._clahe_maps(exposure._clahe_plan(gpu.asarray(x), kernel, clip_limit, nbins)).get()
        assert got.dtype == np.uint16 and got.shape == want.shape
        for r in range(want.shape[0]):
            assert_array_equal(got[r], want[r], err_msg="region {} under {}".format(r, setting))


@pytest.mark.parametrize("dtype", ["uint16", "float64", "float32"])
def test_constant_image(gpu, exposure, knob, dtype):
    x = np.zeros((24, 40), dtype) + (1 if dtype != "uint16" else 0)
    want = er.equalize_adapthist(x, 3)
    assert want.min() == want.max()
    for setting in SETTINGS:
        knob(*setting)
        assert_array_equal(exposure.equalize_adapthist(gpu.asarray(x), kernel_size=3).get(), want)


def test_clip_limit_zero_and_one_agree(gpu, exposure):
    xd = gpu.asarray(_image((40, 70), "float32"))
    assert_array_equal(exposure.equalize_adapthist(xd, clip_limit=0).get(), exposure.equalize_adapthist(xd, clip_limit=1).get())


def test_views_host_inputs_and_repeat_calls(gpu, exposure):
    x = _image((20, 33, 70), "uint16")
    kernel = (5, 8, 16)
    want = _want((20, 33, 70), "uint16", 1, False, kernel, 0.01, 256)
    xd = gpu.asarray(x)
    first = exposure.equalize_adapthist(xd, kernel_size=kernel).get()
    assert_array_equal(first, want)
    assert_array_equal(exposure.equalize_adapthist(xd, kernel_size=kernel).get(), first)             # two calls in a row
    assert_array_equal(exposure.equalize_adapthist(x, kernel_size=kernel).get(), want)               # a host array
    view = xd[::2, 1:, ::3]                                                                          # a non-contiguous view
    hv = np.ascontiguousarray(x[::2, 1:, ::3])
    assert_array_equal(exposure.equalize_adapthist(view, kernel_size=(3, 4, 5)).get(), er.equalize_adapthist(hv, (3, 4, 5)))
    assert_array_equal(xd.get(), x)                                                                  # the input is left alone


def test_float_images_outside_the_unit_range_are_refused(gpu, exposure):
    x = np.linspace(-0.5, 1.5, 64 * 64, dtype=np.float32).reshape(64, 64)
    with pytest.raises(ValueError, match="between -1 and 1"):
        exposure.equalize_adapthist(gpu.asarray(x))


# ---------------------------------------------------------------- equalize_hist and the small functions
EH_SHAPES = [(9, 37, 64), (70, 96)]


@pytest.mark.parametrize("nbins", [2, 256])
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
@pytest.mark.parametrize("shape", EH_SHAPES, ids=["9x37x64", "70x96"])
def test_equalize_hist_matches_host(gpu, exposure, shape, dtype, nbins):
    from cupyimg_amd import last_kernel
    x = _image(shape, dtype)
    mask = np.zeros(shape, bool)
    mask[tuple(slice(s // 4, s - s // 5) for s in shape)] = True
    for m in (None, mask):
        got = exposure.equalize_hist(gpu.asarray(x), nbins=nbins, mask=None if m is None else gpu.asarray(m))
        assert got.dtype == np.float64
        assert_array_equal(got.get(), er.equalize_hist(x, nbins, m))
        assert "interp_map_kernel<{},LDS>".format(dtype) in last_kernel(), last_kernel()
    cdf, centers = exposure.cumulative_distribution(gpu.asarray(x), nbins)
    wc, wcen = er.cumulative_distribution(x, nbins)
    assert_array_equal(cdf.get(), wc)
    assert_array_equal(centers.get(), wcen)
    assert centers.dtype == wcen.dtype


def test_equalize_hist_table_in_global_memory(gpu, exposure):
    """more than 4096 knots: a 16-bit image that spans its range"""
    from cupyimg_amd import last_kernel
    rng = np.random.default_rng(7)
    x = rng.integers(0, 65536, size=(70, 96)).astype(np.uint16)
    x[0, 0], x[0, 1] = 0, 65535
    got = exposure.equalize_hist(gpu.asarray(x))
    assert "interp_map_kernel<uint16,global>" in last_kernel(), last_kernel()
    assert_array_equal(got.get(), er.equalize_hist(x))


def test_equalize_hist_value_on_the_top_edge(gpu, exposure):
    x = np.array([[0.0, 0.25, 0.5, 1.0], [1.0, 0.75, 0.125, 1.0]], np.float64)
    for nbins in (2, 4, 256):
        assert_array_equal(exposure.equalize_hist(gpu.asarray(x), nbins=nbins).get(), er.equalize_hist(x, nbins))
        hist, centers = exposure.histogram(gpu.asarray(x), nbins)
        assert_array_equal(hist.get(), np.histogram(x, nbins)[0])


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32", "float64"])
def test_histogram_normalize_and_dtype_range(gpu, exposure, dtype):
    x = _image((9, 37, 64), dtype) if dtype != "int16" else (_image((9, 37, 64), "uint16").astype(np.int16) - 2000)
    xd = gpu.asarray(x)
    for kw in ({}, {"normalize": True}, {"source_range": "dtype"}, {"source_range": "dtype", "normalize": True, "nbins": 7}):
        hist, centers = exposure.histogram(xd, **kw)
        wh, wc = er.histogram(x, **kw)
        assert_array_equal(hist.get(), wh)
        assert_array_equal(centers.get(), wc)
        assert hist.dtype == wh.dtype and centers.dtype == wc.dtype


@pytest.mark.parametrize("case", KAT["histogram"], ids=lambda c: c["name"])
def test_histogram_vectors(gpu, exposure, case):
    hist, centers = exposure.histogram(gpu.asarray(np.asarray(case["image"], dtype=case["dtype"])), **case["kwargs"])
    er.check_histogram_case(case, hist.get(), centers.get())


def test_histogram_warns_on_a_colour_shaped_array(gpu, exposure):
    with pytest.warns(UserWarning, match="color image"):
        exposure.histogram(gpu.asarray(np.zeros((4, 5, 3), np.uint8)))
    with pytest.raises(ValueError):
        exposure.histogram(gpu.asarray(np.array([-1, 100], np.int8)), source_range="foobar")


@pytest.mark.parametrize("case", KAT["rescale_intensity"], ids=lambda c: c["name"])
def test_rescale_intensity_vectors(gpu, exposure, case):
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in case["kwargs"].items()}
    x = np.asarray(case["image"], dtype=case["dtype"])
    out = exposure.rescale_intensity(gpu.asarray(x), **kw)
    want = er.rescale_intensity(x, **kw)
    assert out.dtype == want.dtype
    assert_array_equal(out.get(), want)
    if case["compare"] == "almost":
        np.testing.assert_array_almost_equal(out.get(), case["expected"])
    elif case["compare"] == "equal":
        assert_array_equal(out.get(), case["expected"])


@pytest.mark.parametrize("in_range,out_range", [("image", "dtype"), ("dtype", "image")])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_rescale_nan_warning(gpu, exposure, dtype, in_range, out_range):
    """test_rescale_nan_warning of the reference (test_exposure.py:302): a NaN in the image is its min and max, the
    warning is given and the NaN is broadcast to the whole result"""
    x = np.arange(12, dtype=dtype).reshape(3, 4)
    x[1, 1] = np.nan
    with pytest.warns(UserWarning, match=r"One or more intensity levels are NaN\. Rescaling will broadcast NaN to the full image\."):
        out = exposure.rescale_intensity(gpu.asarray(x), in_range, out_range)
    assert out.dtype == x.dtype
    assert np.isnan(out.get()).all()
    with np.errstate(all="ignore"):
        assert_array_equal(out.get(), er.rescale_intensity(x, in_range, out_range))


@pytest.mark.parametrize("nbins", [2, 5])
def test_bool_images_are_counted_as_numpy_histogram_counts_them(gpu, exposure, nbins):
    """bool is no integer dtype to the reference: `nbins` bins between float64 edges, not one bin per value"""
    x = _image((17, 19), "uint8") > 100
    for kw, rng in (({}, None), ({"source_range": "dtype"}, (0, 1)), ({"normalize": True}, None)):
        hist, centers = exposure.histogram(gpu.asarray(x), nbins, **kw)
        wh, edges = np.histogram(x.astype(np.uint8), nbins, range=rng)
        if kw.get("normalize"):
            wh = wh / wh.sum()
        assert_array_equal(hist.get(), wh)
        assert_array_equal(centers.get(), (edges[:-1] + edges[1:]) / 2.0)
        assert centers.dtype == np.float64 and len(hist) == nbins
    const = np.ones((4, 5), bool)
    hist, centers = exposure.histogram(gpu.asarray(const), nbins)
    wh, edges = np.histogram(const.astype(np.uint8), nbins)
    assert_array_equal(hist.get(), wh)
    assert_array_equal(centers.get(), (edges[:-1] + edges[1:]) / 2.0)
    assert_array_equal(exposure.equalize_hist(gpu.asarray(x), nbins).get(), er.equalize_hist(x, nbins))


def test_equalize_hist_refuses_a_table_beyond_its_limit_before_counting(gpu, exposure):
    x = np.array([[0, 1], [65536, 7]], np.uint32)                                # 65537 knots
    with pytest.raises(ValueError, match="at most 65536"):
        exposure.equalize_hist(gpu.asarray(x))
    with pytest.raises(ValueError, match="at most 65536"):
        exposure.equalize_hist(gpu.asarray(x.astype(np.float32) / 65536), nbins=65537)
    wide = np.array([[-2 ** 62, 5], [2 ** 62, 7]], np.int64)                     # 2^63 bins: refused, not allocated
    with pytest.raises(ValueError, match="at most 65536"):
        exposure.equalize_hist(gpu.asarray(wide))
    ok = np.array([[3, 1], [65536, 7]], np.uint32)                               # 65536 knots, searched in global memory
    assert_array_equal(exposure.equalize_hist(gpu.asarray(ok)).get(), er.equalize_hist(ok))


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_rescale_intensity_on_an_image(gpu, exposure, dtype):
    x = _image((70, 96), dtype)
    lo, hi = float(np.percentile(x, 2)), float(np.percentile(x, 98))
    combos = [{}, {"in_range": (lo, hi)}, {"in_range": (lo, hi), "out_range": (0, 255)}, {"out_range": "uint8"},
              {"in_range": "dtype", "out_range": (0.0, 1.0)}, {"in_range": "image", "out_range": "image"},
              {"in_range": np.float32 if dtype.startswith("float") else np.uint16, "out_range": "uint14"}]
    for kw in combos:
        out = exposure.rescale_intensity(gpu.asarray(x), **kw)
        want = er.rescale_intensity(x, **kw)
        assert out.dtype == want.dtype, kw
        assert_array_equal(out.get(), want, err_msg=str(kw))
    with pytest.raises(ValueError):
        exposure.rescale_intensity(gpu.asarray(x), out_range="flat")
