"""The references the device's peak functions are held to (tests/helpers/peak_ref.py) are checked themselves, on the host:
the transcription of peak_local_max meets every known answer of tests/golden/peak_kat.json, the round-based greedy equals
the reference's sequential loops, and the exact integer distance rule equals SciPy's Minkowski distance comparison."""
import itertools
import json
import os

import numpy as np
import pytest
from scipy.spatial import distance

from helpers import corner_ref, peak_ref

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "peak_kat.json")))
# what tests/test_gpu_peaks.py demands of the squared dot's Harris response: with min_distance 1 peak_local_max finds the
# square's four corners, three pixels apart; with min_distance 3 corner_peaks, whose greedy pass rejects at a distance of
# min_distance or less, keeps exactly one of them.  The four responses are equal in exact arithmetic; which one is the largest
# in floating point rests on the last bits of the Gaussian (on the host they come out equal and the first in raster order
# wins), so the place of the survivor is held to the transcription on the same response, not to a literal.
SQUARED_DOT_CORNER_KWARGS = dict(min_distance=1, threshold_rel=0.5)
SQUARED_DOT_KWARGS = dict(min_distance=3, threshold_rel=0.1)
SQUARED_DOT_CORNERS = [[4, 4], [4, 7], [7, 4], [7, 7]]


def _case_image(case):
    image = peak_ref.kat_image(case["image"])
    if case.get("detector"):
        image = corner_ref.detector(case["detector"], image, **dict(case["detector_kwargs"]))
    return image


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_transcription_meets_the_known_answers(case):
    image = _case_image(case)
    kwargs = peak_ref.kat_kwargs(case["kwargs"])
    if "raises" in case["expect"]:
        with pytest.raises({"ValueError": ValueError, "TypeError": TypeError}[case["expect"]["raises"]]):
            peak_ref.peak_local_max(image, **kwargs)
        return
    peak_ref.kat_check(peak_ref.peak_local_max(image, **kwargs), case["expect"], image)


def test_known_answers_are_the_generators():
    """peak_kat.json is what make_peak_kat.py writes"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("make_peak_kat", os.path.join(HERE, "golden", "make_peak_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as tmp:
        mod.HERE = tmp
        mod.main()
        assert json.load(open(os.path.join(tmp, "peak_kat.json"))) == KAT
    names = [c["name"] for c in KAT["cases"]]
    assert len(set(names)) == len(names) and all(c["ref"] for c in KAT["cases"])


def tie_rich_points(rank, seed):
    """distinct integer points on a small grid, in a seeded order: many equal distances at the spacings tested"""
    rng = np.random.default_rng(seed)
    side = (40, 9, 5)[rank - 1]
    cells = np.array(list(itertools.product(range(side), repeat=rank)), dtype=np.int64)
    k = int(rng.integers(1, min(len(cells), 60) + 1))
    return cells[rng.permutation(len(cells))[:k]], (side,) * rank


SETS = [(rank, seed) for rank in (1, 2, 3) for seed in range(6)]


@pytest.mark.parametrize("p_norm", (1, 2, np.inf))
@pytest.mark.parametrize("spacing", (1, 2, 3, 4))
def test_round_based_greedy_equals_the_sequential_loops(p_norm, spacing):
    for rank, seed in SETS:
        pts, _ = tie_rich_points(rank, seed)
        got, rounds = peak_ref.greedy_rounds(pts, spacing, p_norm, inclusive=False)
        assert np.array_equal(got, peak_ref.ensure_spacing(pts, spacing, p_norm)), (rank, seed)
        assert rounds <= len(pts)
        got, rounds = peak_ref.greedy_rounds(pts, spacing, p_norm, inclusive=True)
        assert np.array_equal(got, peak_ref.corner_spacing(pts, spacing, p_norm)), (rank, seed)
        assert rounds <= len(pts)


@pytest.mark.parametrize("p_norm", (1, 2, np.inf))
def test_integer_distance_rule_equals_minkowski(p_norm):
    for rank, seed in SETS:
        pts, _ = tie_rich_points(rank, seed)
        d = distance.cdist(pts, pts, distance.minkowski, p=p_norm)
        for spacing in (1, 2, 3, 4):
            off = ~np.eye(len(pts), dtype=bool)
            assert np.array_equal(peak_ref.conflicts(pts, spacing, p_norm, False), (d < spacing) & off)
            assert np.array_equal(peak_ref.conflicts(pts, spacing, p_norm, True), (d <= spacing) & off)


def test_full_plateau_takes_many_rounds_but_never_more_than_points():
    pts = np.argwhere(np.ones((24, 24), bool))
    for spacing in (3, 5):
        got, rounds = peak_ref.greedy_rounds(pts, spacing)
        assert np.array_equal(got, peak_ref.ensure_spacing(pts, spacing))
        assert 4 < rounds <= len(pts)


def test_squared_dot_corner_peaks_is_the_fixed_point():
    response = corner_ref.detector("corner_harris", peak_ref.squared_dot_image())
    assert sorted(peak_ref.peak_local_max(response, **SQUARED_DOT_CORNER_KWARGS).tolist()) == SQUARED_DOT_CORNERS
    got = peak_ref.corner_peaks(response, **SQUARED_DOT_KWARGS).tolist()
    assert len(got) == 1 and got[0] in SQUARED_DOT_CORNERS
    assert got == [[4, 4]]                    # the four responses are equal bit for bit here: the first in raster order
    assert peak_ref.corner_peaks(response, indices=False, **SQUARED_DOT_KWARGS).sum() == 1
    # and the example of the reference's docstring (corner.py:891-906)
    response = np.zeros((5, 5))
    response[2:4, 2:4] = 1
    assert peak_ref.peak_local_max(response).tolist() == [[2, 2], [2, 3], [3, 2], [3, 3]]
    assert peak_ref.corner_peaks(response).tolist() == [[2, 2]]
