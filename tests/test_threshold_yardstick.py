"""The yardsticks of the thresholding tests, on the host: the NumPy references of tests/helpers/threshold_ref.py meet every
known answer of tests/golden/threshold_kat.json (the literal cases of the reference's test_thresholding.py), the JSON is what
its generator writes, the integral-image form of _mean_std equals direct window sums bit for bit on integer images whose
sums stay below 2^53, and the brute-force multi-Otsu agrees with Otsu for two classes.  The inputs and case tables the GPU
tests share live here."""
import importlib.util
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from helpers import threshold_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_PATH = os.path.join(HERE, "golden", "threshold_kat.json")
with open(KAT_PATH) as _f:
    KAT = json.load(_f)
KAT_CASES = KAT["cases"]
KAT_IDS = [c["name"] for c in KAT_CASES]


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def seeded(shape, dtype, seed, lo=None, hi=None):
    """seeded image: integers over [lo, hi) (default: a range with negative values for signed dtypes), bool half set, floats
    in [0, 1000)"""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return rng.random(shape) < 0.5
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        lo = max(info.min, -3000 if dtype.kind == "i" else 0) if lo is None else lo
        hi = min(info.max + 1, 3000 if dtype.itemsize > 1 else 256) if hi is None else hi
        return rng.integers(lo, hi, size=shape).astype(dtype)
    return (rng.random(shape) * 1000).astype(dtype)


# (shape, window) of the window-statistics tests; ranks 2 and 3 run fused, fused with small tiles, and generic
WINDOW_CASES = [((37, 41), 15), ((37, 41), 3), ((37, 41), (3, 5)), ((9, 7), 15), ((1, 23), (1, 9)), ((11, 12, 13), (5, 3, 7)),
                ((11, 12, 13), (1, 5, 5)), ((50,), 7), ((5, 6, 7, 8), 3),
                ((6, 67), (3, 5))]            # rows of 67 bytes / 134 bytes: no multiple of 16
WINDOW_IDS = ["x".join(map(str, s)) + "-w" + (str(w) if isinstance(w, int) else "x".join(map(str, w))) for s, w in WINDOW_CASES]
INT_DTYPES = ["uint8", "uint16", "int16", "bool"]

# the cases of the issue on which the two host forms were found identical
EXACT_CASES = [("uint8", (37, 41), 15), ("uint8", (9, 7), 15), ("uint16", (9, 13), (3, 5)), ("uint16", (11, 12, 13), (5, 3, 7)),
               ("int16", (20, 20, 20), 15)]


def full_range(shape, dtype, seed):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, info.max + 1, size=shape).astype(dtype)


@pytest.mark.parametrize("case", KAT_CASES, ids=KAT_IDS)
def test_references_meet_the_known_answers(case):
    image = R.kat_image(case["image"])
    fn = R.FUNCTIONS[case["function"]]
    R.check_expectation(case["expect"], lambda: fn(image, **case["kwargs"]), image)


def test_json_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("make_threshold_kat", os.path.join(HERE, "golden", "make_threshold_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(KAT_PATH) as f:
        assert f.read() == mod.dumps()
    assert len(KAT_CASES) >= 50 and len(set(KAT_IDS)) == len(KAT_IDS)


@pytest.mark.parametrize("dtype,shape,w", EXACT_CASES, ids=["{}-{}".format(d, "x".join(map(str, s))) for d, s, _ in EXACT_CASES])
def test_integral_image_form_equals_direct_sums_on_integers(dtype, shape, w):
    image = full_range(shape, dtype, 7)
    sum_abs, sum_sq = R.integral_sum_bound(image, w)
    assert sum_abs < 2 ** 53 and sum_sq < 2 ** 53          # every entry of both integral images is an exact float64
    mi, si = R.mean_std_integral(image, w)
    md, sd = R.mean_std_direct(image, w)
    assert same_bits(mi, md) and same_bits(si, sd)


@pytest.mark.parametrize("shape,w", WINDOW_CASES, ids=WINDOW_IDS)
def test_window_cases_stay_exact(shape, w):
    """the shapes the GPU test compares bit for bit keep every integral-image entry below 2^53 for every integer dtype"""
    for dtype in ("uint16", "int16"):
        sum_abs, sum_sq = R.integral_sum_bound(np.full(shape, np.iinfo(dtype).min if dtype == "int16" else np.iinfo(dtype).max, dtype), w)
        assert sum_abs < 2 ** 53 and sum_sq < 2 ** 53


def test_direct_sums_on_floats_meet_the_derived_bounds():
    """the direct float64 form is itself inside the bounds the device is held to"""
    image = seeded((9, 11), "float32", 3)
    m, s = R.mean_std_direct(image, (3, 5))
    worst = R.check_mean_std_bounds(image, (3, 5), m, s)
    assert max(worst) <= 1.0


@pytest.mark.parametrize("seed", range(6))
def test_brute_force_multiotsu_is_otsu_for_two_classes(seed):
    rng = np.random.default_rng(seed)
    nbins = int(rng.integers(8, 80))
    counts = rng.integers(0, 500, size=nbins)
    counts[0] = counts[-1] = 1 + counts[0]                   # a histogram of an image spans its extrema
    want = R.otsu(hist=counts)
    got = R.multiotsu_brute(counts / counts.sum(), 2)
    assert got == (int(want),)


# symmetric histograms whose optimum is attained by exactly two tuples, mirror images of each other: (counts, classes, the two)
TIE_CASES = [([4, 0, 4, 0, 4, 0, 4], 2, [(2,), (3,)]), ([1, 1, 4, 4, 4, 1, 1], 3, [(1, 3), (2, 4)]),
             ([6, 3, 6, 1, 1, 6, 3, 6], 3, [(1, 4), (2, 5)])]


def tie_image(counts):
    return np.repeat(np.arange(len(counts)), counts).astype(np.uint8)


@pytest.mark.parametrize("counts,classes,pair", TIE_CASES, ids=["tie-{}bins-{}classes".format(len(c), k) for c, k, _ in TIE_CASES])
def test_tie_cases_are_exact_ties(counts, classes, pair):
    import itertools
    total = sum(counts)
    assert total & (total - 1) == 0                          # a power of two: the probabilities are exact
    values = {t: R.multiotsu_exact(counts, t) for t in itertools.combinations(range(len(counts) - 1), classes - 1)}
    best = max(values.values())
    assert sorted(t for t, v in values.items() if v == best) == sorted(pair)
    for t in pair:
        assert Fraction(R.multiotsu_float(counts, t)) == best            # evaluated without a rounding error
    assert R.multiotsu_brute(np.asarray(counts) / total, classes) == min(pair)
    assert np.array_equal(R.multiotsu(tie_image(counts), classes), np.asarray(min(pair)))
