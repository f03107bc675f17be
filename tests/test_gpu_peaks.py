"""peak_local_max, corner_peaks and the greedy spacing on the device against the host transcription of the reference
(tests/helpers/peak_ref.py): coordinates AND order, exact; every known answer of tests/golden/peak_kat.json."""
import warnings

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import dirty_pool, peak_ref
from test_peaks_yardstick import KAT, SQUARED_DOT_CORNER_KWARGS, SQUARED_DOT_CORNERS, SQUARED_DOT_KWARGS

pytestmark = pytest.mark.gpu

SHAPES = ((20, 20), (33, 70), (9, 10, 11), (4, 5, 6, 7))
DTYPES = ("float32", "float64", "uint8", "int16")
CROSS = {n: np.abs(np.indices((3,) * n) - 1).sum(0) <= 1 for n in (2, 3, 4)}


def _feature():
    from cupyimg_amd.skimage import feature
    return feature


def make_image(kind, shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    smooth = sndi.gaussian_filter(rng.standard_normal(shape), 1.0)
    smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min())
    if kind == "smooth":
        x = smooth * 200 if dtype.kind in "iu" else smooth
    elif kind == "ties":                      # a quantised image: many equal values, many equal maxima
        x = np.round(smooth * 6)
    elif kind == "plateaus":                  # flat tops, two of them touching the border
        x = np.round(smooth * 3)
        x[:3, :4] = 9
        x[-2:, ...] = 9
        x[tuple(s // 2 for s in shape)] = 11
    elif kind == "constant":
        x = np.full(shape, 7.0)
    elif kind == "negative":
        x = -1 - np.round(smooth * 50)
    else:
        raise ValueError(kind)
    return x.astype(dtype)


def _run(gpu, fn, image, **kw):
    """(device result as a host array, the transcription's); the image must come back untouched"""
    d = gpu.asarray(image)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        warnings.simplefilter("ignore", RuntimeWarning)
        got = getattr(_feature(), fn)(d, **kw)
    want = getattr(peak_ref, fn)(image, **kw)
    assert np.array_equal(d.get(), image)
    return got, want


def _same(got, want, image):
    if want.dtype == bool:
        assert got.dtype == np.bool_ and got.shape == image.shape and np.array_equal(got.get(), want)
    else:
        assert got.dtype == np.int64 and got.shape == (len(want), image.ndim), (got.shape, want.shape)
        assert np.array_equal(got.get(), want.reshape(-1, image.ndim)), (got.get().tolist()[:8], want.tolist()[:8])


# an unsigned image has no negative values
KINDS_DTYPES = [(kind, dtype) for kind in ("smooth", "ties", "plateaus", "constant", "negative") for dtype in DTYPES
                if not (kind == "negative" and dtype == "uint8")]


@pytest.mark.parametrize("fn", ("peak_local_max", "corner_peaks"))
@pytest.mark.parametrize("kind,dtype", KINDS_DTYPES)
def test_images_shapes_and_distances(gpu, fn, kind, dtype):
    for k, shape in enumerate(SHAPES):
        image = make_image(kind, shape, dtype, seed=k)
        for min_distance in (1, 2, 5):
            got, want = _run(gpu, fn, image, min_distance=min_distance, exclude_border=min_distance == 2)
            _same(got, want, image)


@pytest.mark.parametrize("fn", ("peak_local_max", "corner_peaks"))
def test_footprint_border_thresholds_num_peaks_norms_and_masks(gpu, fn):
    for k, shape in enumerate(SHAPES):
        n = len(shape)
        image = make_image("ties", shape, "float32", seed=10 + k)
        cases = [dict(footprint=CROSS[n]), dict(footprint=CROSS[n], min_distance=2, exclude_border=False),
                 dict(footprint=np.ones((1,) * n, bool), threshold_abs=2.5),
                 dict(exclude_border=False), dict(exclude_border=0), dict(exclude_border=True, min_distance=3), dict(exclude_border=2),
                 dict(exclude_border=tuple(range(n))), dict(exclude_border=(40,) + (0,) * (n - 1)),
                 dict(threshold_abs=3.0), dict(threshold_rel=0.6), dict(threshold_abs=2.0, threshold_rel=0.9), dict(threshold_abs=-5, threshold_rel=0.0),
                 dict(num_peaks=1), dict(num_peaks=3, exclude_border=False), dict(num_peaks=10 ** 6),
                 dict(indices=False), dict(indices=False, min_distance=2, exclude_border=False), dict(indices=False, threshold_abs=1e9)]
        cases += [dict(p_norm=p, min_distance=d, exclude_border=False) for p in (1, 2, np.inf) for d in (2, 3)]
        for kw in cases:
            got, want = _run(gpu, fn, image, **kw)
            _same(got, want, image)
    # an integer image against a fractional threshold: compared in float64, as NumPy does
    image = make_image("ties", (33, 70), "uint8", seed=3)
    for kw in (dict(threshold_abs=2.5), dict(threshold_rel=0.55), dict(threshold_abs=-0.5, exclude_border=False)):
        got, want = _run(gpu, fn, image, **kw)
        _same(got, want, image)


def test_min_distance_below_one_and_single_voxels(gpu):
    image = make_image("ties", (9, 10, 11), "float32", seed=5)
    for kw in (dict(min_distance=0), dict(min_distance=0, threshold_rel=0.5, exclude_border=2)):
        got, want = _run(gpu, "peak_local_max", image, **kw)
        _same(got, want, image)
    with pytest.warns(RuntimeWarning, match="When min_distance < 1"):
        _feature().peak_local_max(gpu.asarray(image), min_distance=0)
    one = np.array([[3.0]], np.float32)
    for kw in (dict(exclude_border=False), dict(exclude_border=False, threshold_abs=2.0), dict()):
        got, want = _run(gpu, "peak_local_max", one, **kw)
        _same(got, want, one)
    host = _feature().peak_local_max(image, min_distance=2)                    # a host image is uploaded
    _same(host, peak_ref.peak_local_max(image, min_distance=2), image)


def test_empty_images(gpu):
    f = _feature()
    for shape in ((0,), (0, 5), (3, 0, 4)):
        image = gpu.asarray(np.zeros(shape, np.float32))
        for fn in (f.peak_local_max, f.corner_peaks):
            got = fn(image)
            assert got.shape == (0, len(shape)) and got.dtype == np.int64
            assert fn(image, exclude_border=False, min_distance=2).shape == (0, len(shape))
        with pytest.warns(FutureWarning):
            assert f.peak_local_max(image, indices=False).shape == shape
    empty = gpu.asarray(np.zeros((0, 2), np.int64))
    assert f._ensure_spacing(empty, (5, 5), 3).shape == (0, 2)


@pytest.mark.parametrize("spacing", (3, 5))
def test_ensure_spacing_on_a_full_plateau(gpu, spacing):
    f = _feature()
    pts = np.argwhere(np.ones((48, 48), bool)).astype(np.int64)
    d = gpu.asarray(pts)
    for inclusive, want in ((False, peak_ref.ensure_spacing(pts, spacing)), (True, peak_ref.corner_spacing(pts, spacing))):
        got = f._ensure_spacing(d, (48, 48), spacing, inclusive=inclusive)
        assert got.dtype == np.int64 and np.array_equal(got.get(), want)
        rounds = peak_ref.greedy_rounds(pts, spacing, np.inf, inclusive)[1]
        # two launches a round, batches of at most 64 rounds beyond the last live one, the init launch and the compaction
        assert 2 * rounds < f.last_peak_launches() <= 2 * (rounds + 64) + 16, (rounds, f.last_peak_launches())
        assert "sel_write_kernel<nonzero,uint8>" in gpu.last_kernel() or "take_kernel" in gpu.last_kernel()
    assert np.array_equal(d.get(), pts)


@pytest.mark.parametrize("p_norm", (1, 2, np.inf))
def test_ensure_spacing_on_tie_rich_sets(gpu, p_norm):
    from test_peaks_yardstick import SETS, tie_rich_points
    f = _feature()
    for rank, seed in SETS:
        pts, shape = tie_rich_points(rank, seed)
        d = gpu.asarray(pts)
        for spacing in (1, 2, 3, 4):
            assert np.array_equal(f._ensure_spacing(d, shape, spacing, p_norm).get(), peak_ref.ensure_spacing(pts, spacing, p_norm))
            assert np.array_equal(f._ensure_spacing(d, shape, spacing, p_norm, inclusive=True).get(), peak_ref.corner_spacing(pts, spacing, p_norm))
            assert 0 < f.last_peak_launches() <= 2 * (len(pts) + 64) + 16
    with pytest.raises(ValueError, match="outside"):
        f._ensure_spacing(gpu.asarray(np.array([[1, 1], [5, 2]], np.int64)), (5, 5), 2)
    with pytest.raises(ValueError, match="outside"):
        f._ensure_spacing(gpu.asarray(np.array([[1, 1], [-1, 2]], np.int64)), (5, 5), 2)


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_known_answers(gpu, case):
    f = _feature()
    image = peak_ref.kat_image(case["image"])
    d = gpu.asarray(image)
    if case.get("detector"):
        d = getattr(f, case["detector"])(d, **dict(case["detector_kwargs"]))
        image = d.get()
    kwargs = peak_ref.kat_kwargs(case["kwargs"])
    expect = case["expect"]
    if "raises" in expect:
        with pytest.raises({"ValueError": ValueError, "TypeError": TypeError}[expect["raises"]]):
            f.peak_local_max(d, **kwargs)
        return
    if "warns" in expect:
        category = FutureWarning if "indices" in expect["warns"] else RuntimeWarning
        with pytest.warns(category, match=expect["warns"]):
            got = f.peak_local_max(d, **kwargs)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = f.peak_local_max(d, **kwargs)
    peak_ref.kat_check(got.get(), expect, image)
    want = peak_ref.peak_local_max(image, **kwargs)
    assert np.array_equal(got.get(), want.reshape(got.shape))


def test_corner_pipeline_on_the_squared_dot(gpu):
    f = _feature()
    response = f.corner_harris(gpu.asarray(peak_ref.squared_dot_image()))
    host = response.get()
    peaks = f.peak_local_max(response, **SQUARED_DOT_KWARGS)
    corners = f.corner_peaks(response, **SQUARED_DOT_KWARGS)
    assert np.array_equal(peaks.get(), peak_ref.peak_local_max(host, **SQUARED_DOT_KWARGS))
    assert np.array_equal(corners.get(), peak_ref.corner_peaks(host, **SQUARED_DOT_KWARGS))
    four = f.peak_local_max(response, **SQUARED_DOT_CORNER_KWARGS)
    assert np.array_equal(four.get(), peak_ref.peak_local_max(host, **SQUARED_DOT_CORNER_KWARGS))
    assert sorted(four.get().tolist()) == SQUARED_DOT_CORNERS
    assert corners.shape == (1, 2) and corners.get().tolist()[0] in SQUARED_DOT_CORNERS
    assert np.array_equal(f.corner_peaks(response, indices=False, **SQUARED_DOT_KWARGS).get(),
                          peak_ref.corner_peaks(host, indices=False, **SQUARED_DOT_KWARGS))
    assert np.array_equal(response.get(), host)
    # the example of the reference's docstring (corner.py:891-906)
    example = np.zeros((5, 5))
    example[2:4, 2:4] = 1
    assert f.peak_local_max(gpu.asarray(example)).get().tolist() == [[2, 2], [2, 3], [3, 2], [3, 3]]
    assert f.corner_peaks(gpu.asarray(example)).get().tolist() == [[2, 2]]
    assert f.last_peak_launches() > 0


@pytest.mark.parametrize("small", (0, 1), ids=["planner-tiles", "small-tiles"])
def test_small_tiles_give_the_same_peaks(gpu, small):
    import ctypes
    from cupyimg_amd import _lib
    lib = _lib.load()
    image = make_image("ties", (33, 70), "float32", seed=21)
    assert lib.mi_debug_set_select(ctypes.c_int(small)) == 0
    try:
        for fn in ("peak_local_max", "corner_peaks"):
            got, want = _run(gpu, fn, image, min_distance=2, exclude_border=False)
            _same(got, want, image)
    finally:
        lib.mi_debug_set_select(ctypes.c_int(0))


@pytest.mark.parametrize("byte", dirty_pool.FILLS)
def test_public_functions_on_a_poisoned_pool(gpu, byte):
    """the filtered maximum, the work block, the pair buffers, the map and the status array come from the pool uninitialised"""
    f = _feature()
    image = make_image("plateaus", (33, 70), "float32", seed=22)
    d = gpu.asarray(image)
    gpu.synchronize()
    with dirty_pool.pool_fill(gpu, byte):
        got = f.peak_local_max(d, min_distance=2, exclude_border=False)
        cor = f.corner_peaks(d, min_distance=2, exclude_border=False)
        with pytest.warns(FutureWarning):
            mask = f.peak_local_max(d, min_distance=2, indices=False)
    assert np.array_equal(got.get(), peak_ref.peak_local_max(image, min_distance=2, exclude_border=False))
    assert np.array_equal(cor.get(), peak_ref.corner_peaks(image, min_distance=2, exclude_border=False))
    assert np.array_equal(mask.get(), peak_ref.peak_local_max(image, min_distance=2, indices=False))
    assert np.array_equal(d.get(), image)
