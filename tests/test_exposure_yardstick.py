"""The host transcription tests/helpers/exposure_ref.py is what tests/test_gpu_exposure.py holds the device to, bit for bit,
so it is checked here without being trusted: against NumPy directly (histogram, bincount, interp), against the literal
vectors of the reference's own tests (tests/golden/exposure_kat.json), against the CLAHE properties the reference's tests
assert, on hand-built histograms for the redistribution loop, and for the admission of the GPU test inputs (the loop must be
entered, and run more than one pass, on the volume the GPU tests use).  No device is needed."""
import json
import os

import numpy as np
import pytest

from helpers import exposure_ref as er

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exposure_kat.json")))


# ---------------------------------------------------------------- against NumPy
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nbins", [2, 7, 256])
def test_float_histogram_is_numpy_histogram(dtype, nbins):
    x = er.volume((9, 37, 64), dtype)
    for source_range, rng in (("image", None), ("dtype", (-1, 1))):
        hist, centers = er.histogram(x, nbins, source_range)
        want, edges = np.histogram(x.reshape(-1), bins=nbins, range=rng)
        np.testing.assert_array_equal(hist, want)
        np.testing.assert_array_equal(centers, (edges[:-1] + edges[1:]) / 2.0)
        assert centers.dtype == ((edges[:-1] + edges[1:]) / 2.0).dtype


def test_float_histogram_of_a_constant_image_and_top_edge():
    x = np.full((5, 6), 0.25, np.float32)
    hist, centers = er.histogram(x, 4)
    want, edges = np.histogram(x.reshape(-1), bins=4)
    np.testing.assert_array_equal(hist, want)
    np.testing.assert_array_equal(centers, (edges[:-1] + edges[1:]) / 2.0)
    y = np.array([0.0, 0.5, 1.0, 1.0, 0.999], np.float64)          # values on the top edge belong to the last bin
    hist, _ = er.histogram(y, 2)
    np.testing.assert_array_equal(hist, np.histogram(y, 2)[0])


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int8", "int16"])
def test_integer_histogram_is_bincount(dtype):
    rng = np.random.default_rng(3)
    info = np.iinfo(dtype)
    x = rng.integers(max(info.min, -90), min(info.max, 700), size=(40, 50)).astype(dtype)
    hist, centers = er.histogram(x)
    lo, hi = int(x.min()), int(x.max())
    np.testing.assert_array_equal(centers, np.arange(lo, hi + 1))
    np.testing.assert_array_equal(hist, np.bincount((x.astype(np.int64) - lo).reshape(-1), minlength=hi - lo + 1))
    hist, centers = er.histogram(x, source_range="dtype")
    np.testing.assert_array_equal(centers, np.arange(info.min, info.max + 1))
    np.testing.assert_array_equal(hist, np.bincount((x.astype(np.int64) - info.min).reshape(-1), minlength=info.max - info.min + 1))
    cdf, c2 = er.cumulative_distribution(x)
    np.testing.assert_array_equal(cdf, np.cumsum(er.histogram(x)[0]) / float(x.size))
    np.testing.assert_array_equal(c2, np.arange(lo, hi + 1))


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
@pytest.mark.parametrize("nbins", [2, 256])
def test_equalize_hist_is_numpy_interp(dtype, nbins):
    x = er.volume((70, 96), dtype)
    mask = np.zeros(x.shape, bool)
    mask[10:50, 20:80] = True
    for m in (None, mask):
        src = x if m is None else x[m]
        hist, centers = er.histogram(src, nbins)
        cdf = hist.cumsum() / float(hist.sum())
        want = np.interp(x.reshape(-1), centers, cdf).reshape(x.shape)
        got = er.equalize_hist(x, nbins, m)
        np.testing.assert_array_equal(got, want)
        assert got.dtype == np.float64 and got.min() >= 0.0 and got.max() == 1.0


def test_interp_on_knots_and_beyond_the_ends():
    xp = np.array([0.5, 1.5, 2.5, 4.0])
    fp = np.array([0.1, 0.4, 0.7, 1.0])
    x = np.array([-3.0, 0.5, 0.75, 1.5, 2.0, 2.5, 3.999, 4.0, 9.0])
    np.testing.assert_array_equal(er.interp(x, xp, fp), np.interp(x, xp, fp))
    np.testing.assert_array_equal(er.interp(x, xp[:1], fp[:1]), np.interp(x, xp[:1], fp[:1]))


# ---------------------------------------------------------------- the reference's literal vectors
@pytest.mark.parametrize("case", KAT["rescale_intensity"], ids=lambda c: c["name"])
def test_rescale_intensity_vectors(case):
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in case["kwargs"].items()}
    out = er.rescale_intensity(np.asarray(case["image"], dtype=case["dtype"]), **kw)
    if case["expected_dtype"]:
        assert out.dtype == np.dtype(case["expected_dtype"])
    if case["compare"] == "equal":
        np.testing.assert_array_equal(out, case["expected"])
    elif case["compare"] == "almost":
        np.testing.assert_array_almost_equal(out, case["expected"])


@pytest.mark.parametrize("case", KAT["histogram"], ids=lambda c: c["name"])
def test_histogram_vectors(case):
    hist, centers = er.histogram(np.asarray(case["image"], dtype=case["dtype"]), **case["kwargs"])
    er.check_histogram_case(case, hist, centers)


# ---------------------------------------------------------------- the reference's CLAHE properties
@pytest.mark.parametrize("dtype", ["uint16", "float64"])
def test_adapthist_constant(dtype):
    """test_exposure.py:436-448"""
    image = np.zeros((200, 200), dtype) + (1 if dtype == "float64" else 0)
    out = er.equalize_adapthist(image, 3)
    assert out.min() == out.max()


def test_adapthist_clip_limit():
    """test_exposure.py:475-484"""
    x = er.volume((48, 64), "float64")
    x = (x - x.min()) / (x.max() - x.min())
    a = er.equalize_adapthist(x, clip_limit=0)
    b = er.equalize_adapthist(x, clip_limit=1)
    np.testing.assert_array_equal(a, b)
    c = er.equalize_adapthist(x, clip_limit=0.01)
    assert not np.array_equal(a, c)


def test_adapthist_stacked_image_matches_2d():
    """test_exposure.py:404-433: a 2-D image stacked along a third axis; the middle slice stays within 0.02 mean absolute
    difference of the 2-D result (the bound of the reference's test), kernel 5, clip limit 0.05"""
    img = er.volume((40, 50), "float64", seed=4)
    img = (img - img.min()) / (img.max() - img.min())
    a = 15
    vol = np.stack([img] * a, axis=0)
    out2 = er.equalize_adapthist(img, kernel_size=5, clip_limit=0.05)
    out3 = er.equalize_adapthist(vol, kernel_size=5, clip_limit=0.05)
    assert out3.shape == vol.shape and out3.dtype == np.float64
    assert np.mean(np.abs(out2 - out3[a // 2])) < 0.02


def test_no_bin_exceeds_the_limit_after_clipping():
    x = er.volume((20, 33, 70), "uint16")
    kernel = (5, 8, 16)
    b = er.bins_of(er.to_gray14(x), 256)
    hist = er.region_histograms(b, kernel, 256).reshape(-1, 256)
    c = er.clip_limit_voxels(0.01, kernel)
    assert c == 6
    assert (hist.sum(axis=1) == 5 * 8 * 16).all()
    assert hist.max() > c
    for h in hist:
        out = er.clip_histogram(h, c)
        assert out.max() <= c and out.min() >= 0
        assert np.all(out >= np.minimum(h, c))


def test_region_histograms_are_those_of_the_padded_image():
    """step 4 against numpy.pad itself, also where the pad is longer than the axis (more than one bounce)"""
    for shape, kernel in (((9, 8), (8, 8)), ((17, 19), (4, 5)), ((1, 1, 7), (1, 1, 1)), ((5, 3), (4, 7))):
        rng = np.random.default_rng(5)
        b = rng.integers(0, 16, size=shape)
        hist = er.region_histograms(b, kernel, 16)
        # the reference's padding: k // 2 before, (k - s % k) % k + ceil(k / 2) after
        pads = [(k // 2, (k - s % k) % k + -(-k // 2)) for s, k in zip(shape, kernel)]
        padded = np.pad(b, pads, mode="reflect")
        nr = [int(s / k) - 1 for s, k in zip(padded.shape, kernel)]
        assert tuple(nr) == hist.shape[:-1]
        for r in np.ndindex(*nr):
            block = padded[tuple(slice(k // 2 + i * k, k // 2 + (i + 1) * k) for i, k in zip(r, kernel))]
            np.testing.assert_array_equal(hist[r], np.bincount(block.reshape(-1), minlength=16))


# ---------------------------------------------------------------- hand-built histograms for the redistribution loop
def test_clip_overshoots():
    """E = 3 after the first two stages, bins 0 .. 9 under the limit: step = 3, the pass at index 0 raises bins 0, 3, 6 and 9 and
    E ends at -1"""
    h = np.array([0] * 10 + [13] + [10] * 5)
    st = {}
    out = er.clip_histogram(h, 10, st)
    assert st["entered"] and st["overshoot"] and st["passes"] == 1 and not st["idle"]
    np.testing.assert_array_equal(out, [1, 0, 0, 1, 0, 0, 1, 0, 0, 1] + [10] * 6)
    assert out.sum() == h.sum() + 1


def test_clip_needs_two_strided_passes():
    """E = 5 with two bins under the limit: step = 1, the pass at index 0 raises both (E = 3), the pass at index 1 the
    second one again (E = 2), and so on"""
    h = np.array([25, 0, 0, 10, 10, 10, 10, 10])
    st = {}
    out = er.clip_histogram(h, 10, st)
    # E = 15, incr = 1, upper = 9: bins 1 and 2 gain 1 (E = 13) ... the loop then adds 1 to every bin under the limit per pass
    assert st["entered"] and st["passes"] >= 2
    assert out.max() <= 10
    np.testing.assert_array_equal(out[3:], 10)
    assert out[0] == 10


def test_clip_leaves_by_the_idle_round():
    """clip_limit * nbins < 1: the limit is 1 and every bin reaches it; E stays positive with no bin under the limit, and the
    loop ends after a round that changes nothing (nbins 16, clip_limit 0.01, a 10 x 10 region)"""
    c = er.clip_limit_voxels(0.01, (10, 10))
    assert c == 1
    h = np.array([7] * 14 + [1, 1])
    assert h.sum() == 100
    st = {}
    out = er.clip_histogram(h, c, st)
    np.testing.assert_array_equal(out, 1)
    assert st["entered"] and st["idle"] and st["rounds"] == 1 and st["passes"] == 16


# ---------------------------------------------------------------- admission of the GPU test inputs
@pytest.mark.parametrize("flat_corner", [False, True])
def test_gpu_test_volume_exercises_the_strided_loop(flat_corner):
    x = er.volume((20, 33, 70), "uint16", flat_corner=flat_corner)
    stats = []
    er.clahe_maps(x, (5, 8, 16), 0.01, 256, stats)
    assert len(stats) == 100
    entered = sum(s["entered"] for s in stats)
    passes = max(s["passes"] for s in stats)
    print("regions that enter the strided loop: {} of {}; most passes: {}; overshoots: {}".format(
        entered, len(stats), passes, sum(s["overshoot"] for s in stats)))
    assert 2 * entered >= len(stats)
    assert passes >= 2


def test_idle_round_case_of_the_gpu_tests():
    x = er.volume((30, 40), "uint8", seed=2)
    stats = []
    er.clahe_maps(x, (10, 10), 0.01, 16, stats)
    assert any(s["idle"] for s in stats)


# ---------------------------------------------------------------- the test_rescale_* items that state no vector
@pytest.mark.parametrize("in_range,out_range", [("image", "dtype"), ("dtype", "image")])
def test_rescale_nan_is_broadcast(in_range, out_range):
    """test_rescale_nan_warning (test_exposure.py:302): NumPy's min and max of an image with a NaN are NaN, and the three
    operations of rescale_intensity then give NaN everywhere (the warning itself is the device function's, checked in
    tests/test_gpu_exposure.py)"""
    x = np.arange(12, dtype=float).reshape(3, 4)
    x[1, 1] = np.nan
    with np.errstate(all="ignore"):
        out = er.rescale_intensity(x, in_range, out_range)
        lo, hi = x.min(), x.max()
        direct = (np.clip(x, lo, hi) - lo) / (hi - lo) if in_range == "image" else (np.clip(x, -1, 1) + 1) / 2 * (hi - lo) + lo
    assert out.dtype == np.float64 and np.isnan(out).all() and np.isnan(direct).all()


@pytest.mark.parametrize("nbins", [2, 5, 256])
def test_bool_histogram_is_numpy_histogram(nbins):
    """bool is no integer dtype to the reference (numpy.issubdtype(bool, numpy.integer) is false): numpy.histogram"""
    x = er.volume((17, 19), np.uint8) > 100
    for kw, rng in (({}, None), ({"source_range": "dtype"}, (0, 1))):
        hist, centers = er.histogram(x, nbins, **kw)
        wh, edges = np.histogram(x.astype(np.uint8), nbins, range=rng)
        np.testing.assert_array_equal(hist, wh)
        np.testing.assert_array_equal(centers, (edges[:-1] + edges[1:]) / 2.0)
    hist, centers = er.histogram(np.ones((3, 4), bool), nbins)
    wh, edges = np.histogram(np.ones(12, np.uint8), nbins)
    np.testing.assert_array_equal(hist, wh)
    np.testing.assert_array_equal(centers, (edges[:-1] + edges[1:]) / 2.0)
