"""The yardstick of the edge family, on the CPU: the host transcription (tests/helpers/edges_ref.py) meets every known answer
of the reference's tests (tests/golden/edges_kat.json); hysteresis by propagation is the label-based formulation; and every
Canny case the device tests use is admitted only if the transcription's edge map with numpy.hypot substituted for
sqrt(a * a + b * b) is identical, no non-maximum-suppression comparison is an exact tie, and (quantile cases) both thresholds
lie strictly between two distinct order statistics.  A case that fails is to be replaced, not tolerated."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

from helpers import edges_ref as R

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edges_kat.json")))
FUNCS = {"sobel": lambda im, m=None, **k: R.edge("sobel", im, m, **k), "scharr": lambda im, m=None, **k: R.edge("scharr", im, m, **k),
         "prewitt": lambda im, m=None, **k: R.edge("prewitt", im, m, **k),
         "roberts": R.roberts, "farid": R.farid, "laplace": lambda im, m=None: R.laplace(im, 3, m),
         "roberts_pos_diag": R.roberts_pos_diag, "roberts_neg_diag": R.roberts_neg_diag, "farid_h": R.farid_h, "farid_v": R.farid_v}
for _n in ("sobel", "scharr", "prewitt"):
    FUNCS[_n + "_h"] = (lambda n: lambda im, m=None: R.edge(n, im, m, axis=0))(_n)
    FUNCS[_n + "_v"] = (lambda n: lambda im, m=None: R.edge(n, im, m, axis=1))(_n)


def kat_image(case):
    if "image" in case:
        return np.asarray(case["image"], dtype=float)
    return np.random.RandomState(case["image_seed"]).uniform(size=case["image_shape"])


def check_edge_case(case, funcs):
    """the stated expectation of one known-answer case, for every function it names; shared with the device tests"""
    expect = case["expect"]
    if expect == "the_centre_response_of_the_cube_is_the_maximum_over_binary_volumes":
        rng = np.random.RandomState(7)
        volumes = (rng.uniform(size=(40, 3, 3, 3)) > 0.5).astype(float)
        for name, cube, axis in case["pairs"]:
            kw = {} if axis is None else {"axis": axis}
            top = np.asarray(funcs[name](np.asarray(case["cubes"][cube], dtype=float), **kw))[1, 1, 1]
            assert 0 < top <= 1 + 1e-12                     # (three roundings of 1 / 3 in prewitt)
            for v in volumes:
                assert np.asarray(funcs[name](v, **kw))[1, 1, 1] <= top * (1 + 1e-12)
        return
    image = kat_image(case)
    mask = np.asarray(case["mask"], dtype=bool) if "mask" in case else None
    for name in case["funcs"]:
        result = np.asarray(funcs[name](image) if mask is None else funcs[name](image, mask))
        if expect == "all_zero":
            np.testing.assert_allclose(result, 0, atol=case.get("atol", 0))
        elif expect == "allclose":
            np.testing.assert_allclose(result, np.asarray(case["expected"], dtype=float), rtol=case["rtol"], atol=1e-12)
        elif expect == "nonzero_pattern":
            assert np.array_equal(result.astype(bool), np.asarray(case["expected"], dtype=bool))
        elif expect == "within_0_1":
            assert result.min() >= 0 and result.max() <= 1
        else:
            grid = np.mgrid[-5:6, -5:6][case["step_axis"]]
            if expect == "times_sqrt2_is_1_on_the_step_and_0_beyond_one_pixel":
                np.testing.assert_allclose((result * np.sqrt(2))[grid == 0], 1, rtol=case["rtol"])
                np.testing.assert_allclose(result[np.abs(grid) > 1], 0, atol=1e-12)
            elif expect == "abs_is_1_on_the_step_and_0_beyond_one_pixel":
                np.testing.assert_allclose(np.abs(result[grid == 0]), 1, rtol=case["rtol"])
                np.testing.assert_allclose(result[np.abs(grid) > 1], 0, atol=case["atol"])
            elif expect == "constant_on_the_step_and_0_beyond_two_pixels":
                assert np.all(result[grid == 0] == result[grid == 0][0]) and result[grid == 0][0] != 0
                np.testing.assert_allclose(result[np.abs(grid) > 2], 0, atol=case["atol"])
            else:
                raise AssertionError("unknown expectation " + expect)


def canny_kat_image(case):
    if case["image"] == "zeros":
        return np.zeros(case["shape"])
    if case["image"] == "uniform":
        return np.random.RandomState(case["image_seed"]).uniform(size=case["shape"])
    return R.circle_image(case["image"] == "noisy_ring", case.get("image_seed", 0))[0]


def check_canny_case(case, canny):
    """shared with the device tests: `canny` takes (image, sigma, low, high[, mask]) and returns a host bool array"""
    if case["expect"] == "ValueError":
        if "thresholds" in case:
            image = np.random.RandomState(0).uniform(size=case["shape"])
            for low, high in case["thresholds"]:
                with pytest.raises(ValueError):
                    canny(image, use_quantiles=True, low_threshold=low, high_threshold=high)
        else:
            with pytest.raises(ValueError):
                canny(np.zeros(case["shape"]), *case["args"])
        return
    image = canny_kat_image(case)
    masks = {"ones": np.ones(image.shape, bool), "zeros": np.zeros(image.shape, bool)}
    if case["expect"] == "equals_the_all_ones_mask":
        assert np.array_equal(canny(image, *case["args"]), canny(image, *case["args"], masks["ones"]))
        return
    result = np.asarray(canny(image, *case["args"], masks[case["mask"]]))
    if case["expect"] == "no_edges":
        assert not result.any()
        return
    ring = R.circle_image(False)[1]
    assert np.all(R.ring_band(ring, case["band_iterations"])[result])
    assert case["count_above"] < result.sum() < case["count_below"]


@pytest.mark.parametrize("case", KAT["edges"], ids=[c["name"] for c in KAT["edges"]])
def test_transcription_meets_the_edge_known_answers(case):
    check_edge_case(case, FUNCS)


@pytest.mark.parametrize("case", KAT["canny"], ids=[c["name"] for c in KAT["canny"]])
def test_transcription_meets_the_canny_known_answers(case):
    check_canny_case(case, R.canny)


def test_single_axis_and_magnitude_conventions():
    """edges.py:180-199: float64 result for a float32 image, division by the rank for a 2-tuple of axes on a volume, and a
    negative axis that is smoothed along the edge axis too (it is not removed from the smoothing axes)"""
    x = np.random.RandomState(0).uniform(size=(5, 6, 7)).astype(np.float32)
    assert R.edge("sobel", x).dtype == np.float64 and R.edge("sobel", x, axis=1).dtype == np.float64
    two = R.edge("sobel", x, axis=(0, 2))
    a, b = R.edge("sobel", x, axis=0), R.edge("sobel", x, axis=2)
    np.testing.assert_allclose(two, np.sqrt((a * a + b * b) / 3), rtol=1e-6)
    assert not np.allclose(R.edge("sobel", x, axis=-1), R.edge("sobel", x, axis=2))
    assert np.array_equal(R.edge_kernel(2, -1, R.SOBEL_SMOOTH), np.array([[1, 0, -1]] * 3) * R.SOBEL_SMOOTH.reshape(3, 1) * R.SOBEL_SMOOTH.reshape(1, 3))


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_hysteresis_by_propagation_is_the_label_formulation(ndim):
    rng = np.random.RandomState(10 + ndim)
    shape = {1: (200,), 2: (40, 50), 3: (12, 14, 16)}[ndim]
    for trial in range(20):
        image = ndi.gaussian_filter(rng.uniform(size=shape), 1.0)
        low, high = np.quantile(image, [0.4 + 0.02 * trial, 0.7])
        mask_low, mask_high = R.threshold_masks(image, low, high)
        assert np.array_equal(R.hysteresis_by_propagation(mask_low, mask_high), R.hysteresis_by_labels(mask_low, mask_high))
    # 8-connectivity, the Canny linking
    full = np.ones((3,) * ndim, bool)
    assert np.array_equal(R.hysteresis_by_propagation(mask_low, mask_high, full), R.hysteresis_by_labels(mask_low, mask_high, full))


def _ulps(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return int(np.abs(ia - ib).max()), int(np.count_nonzero(ia != ib))


CASES = R.canny_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_canny_case_is_admitted(case):
    name, image, kw = case
    plain, hyp = {}, {}
    edges = R.canny(image, detail=plain, **kw)
    edges_hypot = R.canny(image, magnitude_fn=np.hypot, detail=hyp, **kw)
    worst, differing = _ulps(plain["magnitude"], hyp["magnitude"])
    print("{}: {} edge pixels; sqrt(a*a+b*b) vs hypot: at most {} ulp at {} pixels".format(name, int(edges.sum()), worst, differing))
    assert np.array_equal(edges, edges_hypot)
    assert worst <= 1
    assert sum(plain["ties"]) == 0 and sum(hyp["ties"]) == 0
    assert 0 < edges.sum() < edges.size
    if kw.get("use_quantiles"):
        ordered = np.sort(plain["magnitude"].ravel())
        for q, value in ((kw["high_threshold"], plain["high"]), (kw["low_threshold"], plain["low"])):
            k0, k1, gamma = R.percentile_plan(ordered.size, 100.0 * q)
            assert ordered[k0] < value < ordered[k1] and 0 < gamma < 1
