"""The yardstick of the region measurements, vetted on the host: the NumPy transcription (tests/helpers/regionprops_ref.py)
against the reference's known answers (tests/golden/regionprops_kat.json), its find_objects against SciPy's, its central
tables against the rational evaluator within the bound the device is held to, and the premise of the bit-for-bit columns:
every case the GPU test runs keeps its unweighted raw moments below 2**53.  Apart from the first test, which holds the
library's column tables to the transcription's, this file vets the yardstick and not the library."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as sndi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from helpers import regionprops_cases as cases
from helpers import regionprops_ref as ref


def test_the_feature_exports_what_the_yardstick_measures():
    from cupyimg_amd.skimage import measure, morphology
    from cupyimg_amd.scipy import ndimage as ndi
    assert set(ref.COL_DTYPES) <= set(measure.COL_DTYPES)
    for name, dt in ref.COL_DTYPES.items():
        assert measure.COL_DTYPES[name] is dt, name
    assert ref.OBJECT_COLUMNS <= measure.OBJECT_COLUMNS
    assert callable(ndi.find_objects) and callable(morphology.remove_small_objects) and callable(morphology.remove_small_holes)


KAT = cases.kat()


@pytest.mark.parametrize("case", KAT["props"], ids=[c["name"] for c in KAT["props"]])
def test_transcription_meets_the_known_answers(case):
    from make_regionprops_kat import check_props
    lab = cases.kat_array(KAT, case["labels"])
    inten = None if case["intensity"] is None else cases.kat_array(KAT, case["intensity"])
    check_props(case, ref.regionprops(lab, inten))


@pytest.mark.parametrize("case", KAT["misc"], ids=[c["name"] for c in KAT["misc"]])
def test_misc_transcription_meets_the_known_answers(case):
    got = getattr(ref, case["fn"])(np.array(case["image"], case["dtype"]), **case["kwargs"])
    want = np.array(case["expected"], case["expected_dtype"])
    assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("case", cases.ALL_LABEL_CASES, ids=[c[0] for c in cases.ALL_LABEL_CASES])
def test_find_objects_transcription_is_scipys(case):
    _, shape, kind, dtype = case
    lab = cases.labels(shape, kind, dtype)
    top = int(lab.max())
    for max_label in (0, max(top - 2, 1), top, top + 3):
        assert ref.find_objects(lab, max_label) == sndi.find_objects(np.where(lab > 0, lab, 0), max_label)


def test_table_layout_and_the_zero_region_case():
    lab = cases.kat_array(KAT, "SAMPLE_MULTIPLE")
    inten = cases.kat_array(KAT, "INTENSITY_SAMPLE_MULTIPLE")
    t = ref.regionprops_table(lab, inten, properties=("label", "area", "bbox", "centroid", "inertia_tensor", "min_intensity", "slice"))
    assert list(t) == ["label", "area", "bbox-0", "bbox-1", "bbox-2", "bbox-3", "centroid-0", "centroid-1", "inertia_tensor-0-0",
                       "inertia_tensor-0-1", "inertia_tensor-1-0", "inertia_tensor-1-1", "min_intensity", "slice"]
    assert t["label"].tolist() == [1, 2] and t["area"].tolist() == [10, 2] and t["label"].dtype == np.int64
    assert t["bbox-2"].tolist() == [10, 5] and t["centroid-0"].dtype == np.float64 and t["slice"].dtype == object
    assert t["min_intensity"].dtype == np.float64 and t["min_intensity"].tolist() == [2.0, 4.0]
    assert list(ref.regionprops_table(lab, properties=("moments",), separator="_"))[:2] == ["moments_0_0", "moments_0_1"]
    z = ref.regionprops_table(np.zeros((4, 5), np.int32), np.zeros((4, 5), np.float32), properties=("label", "centroid", "max_intensity", "image"))
    assert list(z) == ["label", "centroid-0", "centroid-1", "max_intensity", "image"]
    assert [v.shape for v in z.values()] == [(0,)] * 5
    assert [v.dtype for v in z.values()] == [np.int64, np.float64, np.float64, np.float32, object]


def _regions(case):
    name, shape, kind, ldt, idt = case
    lab = cases.labels(shape, kind, ldt)
    inten = None if idt is None else cases.intensity(shape, idt)
    return lab, inten, ref.regionprops(lab, inten)


@pytest.mark.parametrize("case", cases.TABLE_CASES, ids=[c[0] for c in cases.TABLE_CASES])
def test_central_tables_of_the_transcription_are_within_the_bound(case):
    """the reference's own dot-based evaluation against the rational one about the same float64 centre: well inside the bound
    (0.11 of it on blobs), which is what entitles the bound to judge the device"""
    lab, inten, regions = _regions(case)
    if not regions:
        pytest.fail("a case without regions measures nothing")
    areas = [r.area for r in regions]
    worst = 0.0
    for row in cases.bound_rows(areas):
        r = regions[row]
        worst = max(worst, ref.within_central_bound(r.moments_central, r.image, r.local_centroid, r.area))
        if inten is not None and inten.dtype.kind == "f":
            worst = max(worst, ref.within_central_bound(r.weighted_moments_central, r.intensity_image, r.weighted_local_centroid, r.area))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("case", cases.TABLE_CASES, ids=[c[0] for c in cases.TABLE_CASES])
def test_raw_moments_of_every_gpu_case_stay_below_2_to_the_53(case):
    """every term and every partial sum of an unweighted raw table (and of a weighted one with integer intensities) is an
    integer; below 2**53 all of them are float64 values, so the summation order cannot show"""
    lab, inten, regions = _regions(case)
    for r in regions:
        assert float(np.max(r.moments)) < 2.0 ** 53 and np.array_equal(r.moments, np.round(r.moments))
        if inten is not None and inten.dtype.kind in "iu":
            assert float(np.max(r.weighted_moments)) < 2.0 ** 53 and np.array_equal(r.weighted_moments, np.round(r.weighted_moments))


def test_cases_cover_both_atomic_routes():
    """regions below and above what a workgroup keeps in LDS, for both passes and both ranks"""
    counts = {}
    for name, shape, kind, ldt, _ in cases.TABLE_CASES:
        counts[name] = (len(shape), int(cases.labels(shape, kind, ldt).max()))
    for nd in (2, 3):
        rows = [m for d, m in counts.values() if d == nd]
        assert min(rows) * (1 + 3 * nd) <= cases.LDS_EXT_SLOTS < max(rows) * (1 + 3 * nd), (nd, rows)
        assert min(rows) * 4 ** nd * 2 <= cases.LDS_MOMENT_SLOTS < max(rows) * 4 ** nd, (nd, rows)


def test_ulp_distance_counts_representable_steps():
    assert ref.ulp_distance([1.0, -1.0, np.nan], [np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), np.nan]) == 1
    assert ref.ulp_distance([0.0], [-0.0]) == 0 and ref.ulp_distance([1.0], [np.nan]) == float("inf")
    assert ref.ulp_distance([-5e-324], [5e-324]) == 2
