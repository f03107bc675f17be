"""Writes tests/golden/regionprops_kat.json: the literal arrays and the stated expectations of the reference's tests of the
supported region properties (cupyimg/skimage/measure/tests/test_regionprops.py) and of remove_small_objects /
remove_small_holes (cupyimg/skimage/morphology/tests/test_misc.py, and the docstring examples of morphology/misc.py:96-113,
186-206), as data, each with its file:line.  Nothing here calls the library or the reference; every vector is checked
against the NumPy transcription (tests/helpers/regionprops_ref.py) before it is written.

"props" cases: {"name", "ref", "labels", "intensity" or null, "region": index into the region list, "expect": {property:
value, or {"index": [...], "value": v} entries under "entries"}}; "decimal" is the reference's assert_almost_equal setting
(|got - want| < 1.5 * 10^-decimal).  "misc" cases: {"fn", "image", "dtype", "kwargs", "expected", "warns"}.

    python tests/golden/make_regionprops_kat.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers import regionprops_ref as ref  # noqa: E402

SAMPLE = np.array([
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0],
    [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0],
    [1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0],
    [0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1],
    [0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1],
])
INTENSITY_SAMPLE = SAMPLE.copy()
INTENSITY_SAMPLE[1, 9:11] = 2
SAMPLE_MULTIPLE = np.eye(10, dtype=np.int32)
SAMPLE_MULTIPLE[3:5, 7:8] = 2
INTENSITY_SAMPLE_MULTIPLE = SAMPLE_MULTIPLE.copy() * 2.0
SAMPLE_3D = np.zeros((6, 6, 6), dtype=np.uint8)
SAMPLE_3D[1:3, 1:3, 1:3] = 1
SAMPLE_3D[3, 2, 2] = 1
NAN = float("nan")


def entries(pairs):
    return {"entries": [{"index": list(i), "value": v} for i, v in pairs]}


def main():
    T = "test_regionprops.py:"
    arrays = {
        "SAMPLE": {"dtype": "int64", "data": SAMPLE.tolist()},
        "INTENSITY_SAMPLE": {"dtype": "int64", "data": INTENSITY_SAMPLE.tolist()},
        "SAMPLE_MULTIPLE": {"dtype": "int32", "data": SAMPLE_MULTIPLE.tolist()},
        "INTENSITY_SAMPLE_MULTIPLE": {"dtype": "float64", "data": INTENSITY_SAMPLE_MULTIPLE.tolist()},
        "SAMPLE_3D": {"dtype": "uint8", "data": SAMPLE_3D.tolist()},
        "SAMPLE_MOD": {"dtype": "int64", "data": np.where(np.arange(18) == 17, 0, SAMPLE).tolist()},
        "PADDED_5": {"dtype": "int64", "data": np.pad(SAMPLE, 5, mode="constant").tolist()},
        "PADDED_SLICE": {"dtype": "int64", "data": np.pad(SAMPLE, ((2, 4), (5, 2)), mode="constant").tolist()},
        "DOT": {"dtype": "int64", "data": np.pad(np.ones((1, 1), int), 2).tolist()},
        "DIAG": {"dtype": "int64", "data": np.eye(10, dtype=int).tolist()},
        "DIAG_UD": {"dtype": "int64", "data": np.flipud(np.eye(10, dtype=int)).tolist()},
        "DIAG_LR": {"dtype": "int64", "data": np.fliplr(np.eye(10, dtype=int)).tolist()},
        "DIAG_LRUD": {"dtype": "int64", "data": np.fliplr(np.flipud(np.eye(10, dtype=int))).tolist()},
        "TWOS": {"dtype": "int64", "data": [[2, 2], [2, 2]]},
        "ZEROS": {"dtype": "int64", "data": [[0, 0], [0, 0]]},
    }
    props = []

    def add(name, where, labels, intensity, expect, decimal=7, region=0):
        props.append(dict(name=name, ref=T + where, labels=labels, intensity=intensity, region=region, decimal=decimal, expect=expect))

    add("area", "116-120", "SAMPLE", None, {"area": int(SAMPLE.sum())})
    add("area_3d", "116-120", "SAMPLE_3D", None, {"area": int(SAMPLE_3D.sum())})
    add("bbox", "123-125", "SAMPLE", None, {"bbox": [0, 0, 10, 18]})
    add("bbox_mod", "127-132", "SAMPLE_MOD", None, {"bbox": [0, 0, 10, 17]})
    add("bbox_3d", "134-135", "SAMPLE_3D", None, {"bbox": [1, 1, 1, 4, 3, 3]})
    add("bbox_area", "138-141", "PADDED_5", None, {"bbox_area": int(SAMPLE.size)})
    add("moments_central", "144-154", "SAMPLE", None, {"moments_central": entries([
        ((2, 0), 436.00000000000045), ((3, 0), -737.333333333333), ((1, 1), -87.33333333333303), ((2, 1), -127.5555555555593),
        ((0, 2), 1259.7777777777774), ((1, 2), 2000.296296296291), ((0, 3), -760.0246913580195)])})
    add("centroid", "157-160", "SAMPLE", None, {"centroid": [5.66666666666666, 9.444444444444444]})
    add("centroid_3d", "163-166", "SAMPLE_3D", None, {"centroid": [1.66666667, 1.55555556, 1.55555556]})
    add("slice", "207-212", "PADDED_SLICE", None, {"slice": [[2, 12], [5, 23]]})
    add("eccentricity", "215-217", "SAMPLE", None, {"eccentricity": 0.814629313427})
    add("eccentricity_dot", "219-222", "DOT", None, {"eccentricity": 0.0})
    add("equiv_diameter", "225-228", "SAMPLE", None, {"equivalent_diameter": 9.57461472963})
    add("extent", "263-265", "SAMPLE", None, {"extent": 0.4})
    add("moments_hu", "268-282", "SAMPLE", None, {"moments_hu": [3.27117627e-01, 2.63869194e-02, 2.35390060e-02, 1.23151193e-03,
                                                                  1.38882330e-06, -2.72586158e-05, -6.48350653e-06]}, decimal=6)
    add("image", "285-287", "SAMPLE", None, {"image": SAMPLE.astype(bool).tolist()})
    add("image_3d", "289-290", "SAMPLE_3D", None, {"image": SAMPLE_3D[1:4, 1:3, 1:3].astype(bool).tolist()})
    add("label", "293-298", "SAMPLE", None, {"label": 1})
    add("label_3d", "293-298", "SAMPLE_3D", None, {"label": 1})
    add("major_axis_length", "316-320", "SAMPLE", None, {"major_axis_length": 16.7924234999})
    add("max_intensity", "323-327", "SAMPLE", "INTENSITY_SAMPLE", {"max_intensity": 2})
    add("mean_intensity", "330-334", "SAMPLE", "INTENSITY_SAMPLE", {"mean_intensity": 1.02777777777777})
    add("min_intensity", "337-341", "SAMPLE", "INTENSITY_SAMPLE", {"min_intensity": 1})
    add("minor_axis_length", "344-348", "SAMPLE", None, {"minor_axis_length": 9.739302807263})
    add("moments", "351-363", "SAMPLE", None, {"moments": entries([
        ((0, 0), 72.0), ((0, 1), 680.0), ((0, 2), 7682.0), ((0, 3), 95588.0), ((1, 0), 408.0), ((1, 1), 3766.0), ((1, 2), 43882.0),
        ((2, 0), 2748.0), ((2, 1), 24836.0), ((3, 0), 19776.0)])})
    add("moments_normalized", "366-375", "SAMPLE", None, {"moments_normalized": entries([
        ((0, 2), 0.24301268861454037), ((0, 3), -0.017278118992041805), ((1, 1), -0.016846707818929982),
        ((1, 2), 0.045473992910668816), ((2, 0), 0.08410493827160502), ((2, 1), -0.002899800614433943)])})
    add("orientation", "378-381", "SAMPLE", None, {"orientation": -1.4663278802756865})
    for arr, val in (("DIAG", -np.pi / 4), ("DIAG_UD", np.pi / 4), ("DIAG_LR", np.pi / 4), ("DIAG_LRUD", -np.pi / 4)):
        add("orientation_" + arr.lower(), "383-391", arr, None, {"orientation": float(val)})
    add("weighted_moments_central", "415-431", "SAMPLE", "INTENSITY_SAMPLE", {"weighted_moments_central": [
        [7.4000000000e01, 3.7303493627e-14, 1.2602837838e03, -7.6561796932e02],
        [-2.1316282073e-13, -8.7837837838e01, 2.1571526662e03, -4.2385971907e03],
        [4.7837837838e02, -1.4801314828e02, 6.6989799420e03, -9.9501164076e03],
        [-7.5943608473e02, -1.2714707125e03, 1.5304076361e04, -3.3156729271e04]]}, decimal=6)
    add("weighted_centroid", "434-438", "SAMPLE", "INTENSITY_SAMPLE", {"weighted_centroid": [5.540540540540, 9.445945945945]})
    add("weighted_moments_hu", "441-456", "SAMPLE", "INTENSITY_SAMPLE", {"weighted_moments_hu": [
        3.1750587329e-01, 2.1417517159e-02, 2.3609322038e-02, 1.2565683360e-03, 8.3014209421e-07, -3.5073773473e-05,
        -6.7936409056e-06]}, decimal=6)
    add("weighted_moments", "459-471", "SAMPLE", "INTENSITY_SAMPLE", {"weighted_moments": [
        [7.4000000e01, 6.9900000e02, 7.8630000e03, 9.7317000e04], [4.1000000e02, 3.7850000e03, 4.4063000e04, 5.7256700e05],
        [2.7500000e03, 2.4855000e04, 2.9347700e05, 3.9007170e06], [1.9778000e04, 1.7500100e05, 2.0810510e06, 2.8078871e07]]}, decimal=6)
    add("weighted_moments_normalized", "474-486", "SAMPLE", "INTENSITY_SAMPLE", {"weighted_moments_normalized": [
        [NAN, NAN, 0.2301467830, -0.0162529732], [NAN, -0.0160405109, 0.0457932622, -0.0104598869],
        [0.0873590903, -0.0031421072, 0.0165315478, -0.0028544152], [-0.0161217406, -0.0031376984, 0.0043903193, -0.0011057191]]},
        decimal=6)
    add("label_sequence", "489-494", "TWOS", None, {"label": 2, "n_regions": 1})
    add("pure_background", "497-500", "ZEROS", None, {"n_regions": 0}, region=None)

    for case in props:                                   # every vector against the transcription
        lab = np.array(arrays[case["labels"]]["data"], arrays[case["labels"]]["dtype"])
        inten = None if case["intensity"] is None else np.array(arrays[case["intensity"]]["data"], arrays[case["intensity"]]["dtype"])
        regions = ref.regionprops(lab, inten)
        check_props(case, regions)

    M = "test_misc.py:"
    test_image = [[0, 0, 0, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 1]]
    labeled = [[2, 2, 2, 0, 1], [2, 2, 2, 0, 1], [2, 0, 0, 0, 0], [0, 0, 3, 3, 3]]
    labeled_out = [[2, 2, 2, 0, 0], [2, 2, 2, 0, 0], [2, 0, 0, 0, 0], [0, 0, 3, 3, 3]]
    holes = [[0, 0, 0, 0, 0, 0, 1, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0, 0, 0], [0, 1, 0, 0, 1, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 1, 0, 0, 0, 0],
             [0, 1, 1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1]]
    holes1 = [[0, 0, 0, 0, 0, 0, 1, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0, 0, 0],
              [0, 1, 1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1]]
    holes2 = [r[:] for r in holes1]
    holes2[2], holes2[3] = holes[2][:], holes[3][:]
    labeled_holes = [[2 if (v and i >= 5) else v for v in row] for i, row in enumerate(holes)]
    misc = []

    def madd(name, where, fn, image, dtype, kwargs, expected, expected_dtype, warns=None):
        misc.append(dict(name=name, ref=where, fn=fn, image=image, dtype=dtype, kwargs=kwargs, expected=expected,
                         expected_dtype=expected_dtype, warns=warns))

    rso, rsh = "remove_small_objects", "remove_small_holes"
    madd("one_connectivity", M + "18-25", rso, test_image, "bool", dict(min_size=6), [[0, 0, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]], "bool")
    madd("two_connectivity", M + "28-35", rso, test_image, "bool", dict(min_size=7, connectivity=2),
         [[0, 0, 0, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]], "bool")
    madd("docstring_b", "misc.py:101-105", rso, test_image, "bool", dict(min_size=6), [[0, 0, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]], "bool")
    madd("docstring_c", "misc.py:106-110", rso, test_image, "bool", dict(min_size=7, connectivity=2),
         [[0, 0, 0, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]], "bool")
    madd("labeled_image", M + "48-60", rso, labeled, "int64", dict(min_size=3), labeled_out, "int64")
    madd("uint_image", M + "63-75", rso, labeled, "uint8", dict(min_size=3), labeled_out, "uint8")
    madd("single_label_warning", M + "78-85", rso, [[0, 0, 0, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]], "int64", dict(min_size=6),
         [[0, 0, 0, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]], "int64", warns="use a boolean array?")
    madd("one_connectivity_holes", M + "115-130", rsh, holes, "bool", dict(area_threshold=3), holes1, "bool")
    madd("two_connectivity_holes", M + "133-150", rsh, holes, "bool", dict(area_threshold=3, connectivity=2), holes2, "bool")
    madd("labeled_image_holes", M + "161-190", rsh, labeled_holes, "int64", dict(area_threshold=3), holes1, "bool",
         warns="returned as a boolean array")
    madd("uint_image_holes", M + "193-222", rsh, labeled_holes, "uint8", dict(area_threshold=3), holes1, "bool",
         warns="returned as a boolean array")
    hd = [[1, 1, 1, 1, 1, 0], [1, 1, 1, 0, 1, 0], [1, 0, 0, 1, 1, 0], [1, 1, 1, 1, 1, 0]]
    madd("docstring_holes_b", "misc.py:192-197", rsh, hd, "bool", dict(area_threshold=2),
         [[1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 0], [1, 0, 0, 1, 1, 0], [1, 1, 1, 1, 1, 0]], "bool")
    madd("docstring_holes_c", "misc.py:198-203", rsh, hd, "bool", dict(area_threshold=2, connectivity=2), hd, "bool")
    for case in misc:
        got = getattr(ref, case["fn"])(np.array(case["image"], case["dtype"]), **case["kwargs"])
        assert np.array_equal(got, np.array(case["expected"], case["expected_dtype"])), case["name"]

    with open(os.path.join(HERE, "regionprops_kat.json"), "w") as f:
        json.dump(dict(arrays=arrays, props=props, misc=misc), f, indent=1)
    print("wrote regionprops_kat.json:", len(props), "property cases,", len(misc), "misc cases")


def check_props(case, regions, get=getattr):
    """the stated expectation of one case against a list of regions (`get(region, prop)` reads a property as a host value)"""
    expect = case["expect"]
    if "n_regions" in expect:
        assert len(regions) == expect["n_regions"], case["name"]
    if case["region"] is None:
        return
    r = regions[case["region"]]
    tol = 1.5 * 10.0 ** -case["decimal"]
    for prop, want in expect.items():
        if prop == "n_regions":
            continue
        got = get(r, prop)
        if prop == "slice":
            assert tuple(got) == tuple(slice(a, b) for a, b in want) or [[s.start, s.stop] for s in got] == want, case["name"]
        elif isinstance(want, dict):
            for e in want["entries"]:
                assert abs(float(np.asarray(got)[tuple(e["index"])]) - e["value"]) < tol, (case["name"], e)
        elif prop in ("image",):
            assert np.array_equal(np.asarray(got), np.array(want, bool)), case["name"]
        else:
            g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
            assert g.shape == w.shape, (case["name"], g.shape, w.shape)
            assert np.all((np.abs(g - w) < tol) | (np.isnan(g) & np.isnan(w))), (case["name"], prop, g, w)


if __name__ == "__main__":
    main()
