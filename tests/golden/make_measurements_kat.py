#!/usr/bin/env python3
"""Writes tests/golden/measurements_kat.json: the literal known-answer vectors of the reference's measurement tests
(data only -- inputs, arguments and the expected outputs, each with the reference file:line it is transcribed from).

* cupyimg/scipy/ndimage/tests/test_measurements.py: sum, mean, minimum, maximum, variance, standard_deviation,
  minimum_position, maximum_position, extrema, center_of_mass, histogram and test_stat_funcs_2d.  Every vector is
  evaluated with scipy.ndimage 1.15.3 here, the result is checked against the literal expectation of the reference test
  (where the test states one), and SciPy's result is what the fixture stores, one entry per input dtype the test loops
  over.  Not transcribed: median (absent from this package), maximum_position07 (float labels; this package takes
  integer and bool labels).
* cupyimg/skimage/measure/tests/test_ccomp.py: skimage.measure.label vectors of the 2-D class.  scikit-image is not
  installable in this image, so these are taken as written.

    python tests/golden/make_measurements_kat.py
"""
import json
import os

import numpy as np
import scipy
import scipy.ndimage as sndi

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "cupyimg/scipy/ndimage/tests/test_measurements.py:"
REF_CC = "cupyimg/skimage/measure/tests/test_ccomp.py:"
TYPES = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64"]
cases = []


def _enc(r):
    """SciPy result -> JSON: {"kind": value | positions | hist, "value": ...}"""
    if isinstance(r, tuple) and r and isinstance(r[0], (tuple, list, np.ndarray)) is False:
        return {"kind": "position", "value": [float(c) for c in r]}
    if isinstance(r, list) and r and isinstance(r[0], tuple):
        return {"kind": "positions", "value": [[float(c) for c in p] for p in r]}
    if isinstance(r, np.ndarray) and r.dtype == object:
        return {"kind": "hists", "value": [None if h is None else np.asarray(h).tolist() for h in r]}
    a = np.asarray(r, dtype=np.float64)
    return {"kind": "value", "value": a.tolist()}


def add(name, func, cite, data, dtypes, labels=None, index=None, literal=None, **kw):
    for dt in dtypes:
        x = np.asarray(data, dtype=dt)
        lab = None if labels is None else np.asarray(labels[0], dtype=labels[1])
        args = {k: v for k, v in kw.items()}
        with np.errstate(all="ignore"):
            ref = getattr(sndi, func)(x, *([lab] if lab is not None or index is not None else []),
                                      *([index] if index is not None else []), **args) if func != "histogram" else \
                sndi.histogram(x, args["min"], args["max"], args["bins"], lab, index)
        if literal is not None:
            got = ref
            if func == "extrema":
                got = [np.asarray(got[0], float), np.asarray(got[1], float), np.asarray(got[2], float), np.asarray(got[3], float)]
                for g, w in zip(got, literal):
                    np.testing.assert_allclose(g, np.asarray(w, float), rtol=1e-7, atol=1e-7, equal_nan=True)
            elif func == "histogram" and isinstance(literal, list) and literal and isinstance(literal[0], list):
                for g, w in zip(got, literal):
                    np.testing.assert_array_equal(g, w)
            else:
                np.testing.assert_allclose(np.asarray(got, float), np.asarray(literal, float), rtol=1e-7, atol=1e-7,
                                           equal_nan=True)
        if func == "extrema":
            enc = {"kind": "extrema", "value": [np.asarray(ref[0], float).tolist(), np.asarray(ref[1], float).tolist(),
                                                np.asarray(ref[2], float).tolist(), np.asarray(ref[3], float).tolist()]}
        else:
            enc = _enc(ref)
        cases.append({"name": name, "func": func, "cite": cite, "dtype": dt, "input": x.tolist(), "shape": list(x.shape),
                      "labels": None if lab is None else lab.tolist(), "labels_dtype": None if lab is None else str(lab.dtype),
                      "labels_shape": None if lab is None else list(lab.shape),
                      "index": None if index is None else np.asarray(index).tolist(), "kwargs": args, "expected": enc})


B = ["bool"]
I22 = [[1, 2], [3, 4]]
A34 = [[5, 4, 2, 5], [3, 7, 0, 2], [1, 5, 1, 1]]
A34b = [[5, 4, 2, 5], [3, 7, 8, 2], [1, 5, 1, 1]]
L10 = ([1, 0], "bool")

# ---- sum
add("sum01", "sum_labels", REF + "463-467", [], TYPES, literal=0.0)
add("sum02", "sum_labels", REF + "470-474", np.zeros((0, 4)), TYPES, literal=0.0)
add("sum03", "sum_labels", REF + "477-481", np.ones(()), TYPES, literal=1.0)
add("sum04", "sum_labels", REF + "484-488", [1, 2], TYPES, literal=3.0)
add("sum05", "sum_labels", REF + "491-495", I22, TYPES, literal=10.0)
add("sum06", "sum_labels", REF + "498-503", [], TYPES, labels=([], "bool"), literal=0.0)
add("sum07", "sum_labels", REF + "506-511", np.zeros((0, 4)), TYPES, labels=(np.ones((0, 4)), "bool"), literal=0.0)
add("sum08", "sum_labels", REF + "514-519", [1, 2], TYPES, labels=L10, literal=1.0)
add("sum09", "sum_labels", REF + "522-527", I22, TYPES, labels=L10, literal=4.0)
add("sum10", "sum_labels", REF + "530-534", I22, B, labels=L10, literal=2.0)
add("sum11", "sum_labels", REF + "537-542", I22, TYPES, labels=([1, 2], "int8"), index=2, literal=6.0)
add("sum12", "sum_labels", REF + "545-550", I22, TYPES, labels=([[1, 2], [2, 4]], "int8"), index=[4, 8, 2],
    literal=[4.0, 0.0, 5.0])
# ---- mean
add("mean01", "mean", REF + "553-558", I22, TYPES, labels=L10, literal=2.0)
add("mean02", "mean", REF + "561-565", I22, B, labels=L10, literal=1.0)
add("mean03", "mean", REF + "568-573", I22, TYPES, labels=([1, 2], "int64"), index=2, literal=3.0)
add("mean04", "mean", REF + "576-586", I22, TYPES, labels=([[1, 2], [2, 4]], "int8"), index=[4, 8, 2],
    literal=[4.0, np.nan, 2.5])
# ---- minimum / maximum
add("minimum01", "minimum", REF + "589-594", I22, TYPES, labels=L10, literal=1.0)
add("minimum02", "minimum", REF + "597-601", [[2, 2], [2, 4]], B, labels=L10, literal=1.0)
add("minimum03", "minimum", REF + "604-609", I22, TYPES, labels=([1, 2], "int64"), index=2, literal=2.0)
add("minimum04", "minimum", REF + "612-617", I22, TYPES, labels=([[1, 2], [2, 3]], "int64"), index=[2, 3, 8],
    literal=[2.0, 4.0, 0.0])
add("maximum01", "maximum", REF + "620-625", I22, TYPES, labels=L10, literal=3.0)
add("maximum02", "maximum", REF + "628-632", [[2, 2], [2, 4]], B, labels=L10, literal=1.0)
add("maximum03", "maximum", REF + "635-640", I22, TYPES, labels=([1, 2], "int64"), index=2, literal=4.0)
add("maximum04", "maximum", REF + "643-648", I22, TYPES, labels=([[1, 2], [2, 3]], "int64"), index=[2, 3, 8],
    literal=[3.0, 4.0, 0.0])
add("maximum05", "maximum", REF + "651-654", [-3, -2, -1], ["int64"], literal=-1)
# ---- variance / standard deviation
add("variance01", "variance", REF + "681-691", [], TYPES, literal=np.nan)
add("variance02", "variance", REF + "694-698", [1], TYPES, literal=0.0)
add("variance03", "variance", REF + "701-705", [1, 3], TYPES, literal=1.0)
add("variance04", "variance", REF + "708-711", [1, 0], B, literal=0.25)
add("variance05", "variance", REF + "714-719", [1, 3, 8], TYPES, labels=([2, 2, 3], "int64"), index=2, literal=1.0)
add("variance06", "variance", REF + "722-731", [1, 3, 8, 10, 8], TYPES, labels=([2, 2, 3, 3, 4], "int64"), index=[2, 3, 4],
    literal=[1.0, 1.0, 0.0])
add("standard_deviation01", "standard_deviation", REF + "734-744", [], TYPES, literal=np.nan)
add("standard_deviation02", "standard_deviation", REF + "747-751", [1], TYPES, literal=0.0)
add("standard_deviation03", "standard_deviation", REF + "754-758", [1, 3], TYPES, literal=1.0)
add("standard_deviation04", "standard_deviation", REF + "761-764", [1, 0], B, literal=0.5)
add("standard_deviation05", "standard_deviation", REF + "767-772", [1, 3, 8], TYPES, labels=([2, 2, 3], "int64"), index=2,
    literal=1.0)
add("standard_deviation06", "standard_deviation", REF + "775-786", [1, 3, 8, 10, 8], TYPES,
    labels=([2, 2, 3, 3, 4], "int64"), index=[2, 3, 4], literal=[1.0, 1.0, 0.0])
add("standard_deviation07", "standard_deviation", REF + "789-798", [-0.00619519], ["float32", "float64"],
    labels=([1], "int64"), index=[1], literal=[0.0])
# ---- positions
add("minimum_position01", "minimum_position", REF + "801-806", I22, TYPES, labels=L10, literal=(0, 0))
add("minimum_position02", "minimum_position", REF + "809-813", A34, TYPES, literal=(1, 2))
add("minimum_position03", "minimum_position", REF + "816-819", A34, B, literal=(1, 2))
add("minimum_position04", "minimum_position", REF + "822-825", [[5, 4, 2, 5], [3, 7, 1, 2], [1, 5, 1, 1]], B, literal=(0, 0))
add("minimum_position05", "minimum_position", REF + "828-833", [[5, 4, 2, 5], [3, 7, 0, 2], [1, 5, 2, 3]], TYPES,
    labels=([1, 2, 0, 4], "int64"), literal=(2, 0))
add("minimum_position06", "minimum_position", REF + "836-841", A34, TYPES, labels=([1, 2, 3, 4], "int64"), index=2,
    literal=(0, 1))
add("minimum_position07", "minimum_position", REF + "844-850", A34, TYPES, labels=([1, 2, 3, 4], "int64"), index=[2, 3],
    literal=[(0, 1), (1, 2)])
add("maximum_position01", "maximum_position", REF + "853-858", I22, TYPES, labels=L10, literal=(1, 0))
add("maximum_position02", "maximum_position", REF + "861-865", A34b, TYPES, literal=(1, 2))
add("maximum_position03", "maximum_position", REF + "868-871", A34b, B, literal=(0, 0))
add("maximum_position04", "maximum_position", REF + "874-879", A34b, TYPES, labels=([1, 2, 0, 4], "int64"), literal=(1, 1))
add("maximum_position05", "maximum_position", REF + "882-887", A34b, TYPES, labels=([1, 2, 0, 4], "int64"), index=1,
    literal=(0, 0))
add("maximum_position06", "maximum_position", REF + "890-896", A34b, TYPES, labels=([1, 2, 0, 4], "int64"), index=[1, 2],
    literal=[(0, 0), (1, 1)])
# ---- extrema (the reference checks them against minimum / maximum / *_position: SciPy's values are stored)
add("extrema01", "extrema", REF + "909-919", I22, TYPES, labels=L10, literal=(1, 3, (0, 0), (1, 0)))
add("extrema02", "extrema", REF + "922-932", I22, TYPES, labels=([1, 2], "int64"), index=2, literal=(2, 4, (0, 1), (1, 1)))
add("extrema03", "extrema", REF + "935-951", I22, TYPES, labels=([[1, 2], [2, 3]], "int64"), index=[2, 3, 8],
    literal=([2, 4, 0], [3, 4, 0], [(0, 1), (1, 1), (0, 0)], [(1, 0), (1, 1), (0, 0)]))
add("extrema04", "extrema", REF + "954-966", A34b, TYPES, labels=([1, 2, 0, 4], "int64"), index=[1, 2],
    literal=([1, 4], [5, 7], [(2, 0), (0, 1)], [(0, 0), (1, 1)]))
# ---- center of mass
add("center_of_mass01", "center_of_mass", REF + "969-974", [[1, 0], [0, 0]], TYPES, literal=[0.0, 0.0])
add("center_of_mass02", "center_of_mass", REF + "977-982", [[0, 0], [1, 0]], TYPES, literal=[1, 0])
add("center_of_mass03", "center_of_mass", REF + "985-990", [[0, 1], [0, 0]], TYPES, literal=[0, 1])
add("center_of_mass04", "center_of_mass", REF + "993-998", [[0, 0], [0, 1]], TYPES, literal=[1, 1])
add("center_of_mass05", "center_of_mass", REF + "1001-1006", [[1, 1], [1, 1]], TYPES, literal=[0.5, 0.5])
add("center_of_mass06", "center_of_mass", REF + "1009-1013", [[1, 2], [3, 1]], B, literal=[0.5, 0.5])
add("center_of_mass07", "center_of_mass", REF + "1016-1021", [[1, 2], [3, 1]], B, labels=([1, 0], "int64"),
    literal=[0.5, 0.0])
add("center_of_mass08", "center_of_mass", REF + "1024-1029", [[5, 2], [3, 1]], B, labels=([1, 2], "int64"), index=2,
    literal=[0.5, 1.0])
add("center_of_mass09", "center_of_mass", REF + "1032-1037", [[1, 2], [1, 1]], B, labels=([1, 2], "int64"), index=[1, 2],
    literal=[(0.5, 0.0), (0.5, 1.0)])
# ---- histogram
add("histogram01", "histogram", REF + "1040-1044", np.arange(10), ["int64"], literal=np.ones(10), min=0, max=10, bins=10)
add("histogram02", "histogram", REF + "1047-1052", [1, 1, 3, 4, 3, 3, 3, 3], ["int64"],
    labels=([1, 1, 1, 1, 2, 2, 2, 2], "int64"), index=1, literal=[0, 2, 0, 1, 1], min=0, max=4, bins=5)
add("histogram03", "histogram", REF + "1055-1063", [1, 1, 3, 4, 3, 5, 3, 3], ["int64"],
    labels=([1, 0, 1, 1, 2, 2, 2, 2], "int64"), index=[1, 2], literal=[[0, 1, 0, 1, 1], [0, 0, 0, 3, 0]],
    min=0, max=4, bins=5)
# ---- test_stat_funcs_2d
A = [[5, 6, 0, 0, 0], [8, 9, 0, 0, 0], [0, 0, 0, 3, 5]]
LBL = ([[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 2, 2]], "int64")
for f, want in (("mean", [7.0, 4.0]), ("variance", [2.5, 1.0]), ("standard_deviation", list(np.sqrt([2.5, 1.0]))),
                ("minimum", [5, 3]), ("maximum", [9, 5])):
    add("stat_funcs_2d_" + f, f, REF + "1066-1087", A, ["int64"], labels=LBL, index=[1, 2], literal=want)

# ---- skimage.measure.label (test_ccomp.py, 2-D class), taken as written
ccomp = []
x = [[0, 0, 3, 2, 1, 9], [0, 1, 1, 9, 2, 9], [0, 0, 1, 9, 9, 9], [3, 1, 1, 5, 3, 0]]
labels = np.array([[0, 0, 1, 2, 3, 4], [0, 5, 5, 4, 2, 4], [0, 0, 5, 4, 4, 4], [6, 5, 5, 7, 8, 0]])
nobg = labels + 1
nobg[-1, -1] = 10
bg9 = nobg.copy()
bg9[np.array(x) == 9] = 0
bg9[bg9 > 5] -= 1
ccomp += [{"cite": REF_CC + "15-44", "input": x, "kwargs": {}, "expected": labels.tolist()},
          {"cite": REF_CC + "25-48", "input": x, "kwargs": {"background": 99}, "expected": nobg.tolist()},
          {"cite": REF_CC + "29-50", "input": x, "kwargs": {"background": 9}, "expected": bg9.tolist()},
          {"cite": REF_CC + "61-66", "input": [[0, 0, 1], [0, 1, 0], [1, 0, 0]], "kwargs": {},
           "expected": [[0, 0, 1], [0, 1, 0], [1, 0, 0]]},
          {"cite": REF_CC + "69-76", "input": [[0, 1], [1, 0]], "kwargs": {"connectivity": 1}, "expected": [[0, 1], [2, 0]]},
          {"cite": REF_CC + "69-79", "input": [[0, 1], [1, 0]], "kwargs": {"connectivity": 2}, "expected": [[0, 1], [1, 0]]},
          {"cite": REF_CC + "82-91", "input": [[1, 0, 0], [1, 1, 5], [0, 0, 0]], "kwargs": {},
           "expected": [[1, 0, 0], [1, 1, 2], [0, 0, 0]]},
          {"cite": REF_CC + "82-96", "input": [[1, 0, 0], [1, 1, 5], [0, 0, 0]], "kwargs": {"background": 0},
           "expected": [[1, 0, 0], [1, 1, 2], [0, 0, 0]]},
          {"cite": REF_CC + "98-109", "input": [[0, 0, 6], [0, 0, 6], [5, 5, 5]], "kwargs": {"background": 0},
           "expected": [[0, 0, 1], [0, 0, 1], [2, 2, 2]]},
          {"cite": REF_CC + "111-121", "input": [[0, 0, 0], [0, 1, 0], [0, 0, 0]], "kwargs": {"connectivity": 1, "background": 0},
           "expected": [[0, 0, 0], [0, 1, 0], [0, 0, 0]]},
          {"cite": REF_CC + "123-129", "input": [[1, 0, 6], [0, 0, 6], [5, 5, 5]], "kwargs": {}, "expected_num": 3},
          {"cite": REF_CC + "123-131", "input": [[1, 0, 6], [0, 0, 6], [5, 5, 5]], "kwargs": {"background": -1},
           "expected_num": 4}]

with open(os.path.join(HERE, "measurements_kat.json"), "w") as f:
    json.dump({"generator": "tests/golden/make_measurements_kat.py", "scipy": scipy.__version__, "numpy": np.__version__,
               "ndimage": cases, "skimage_label": ccomp}, f, indent=0)
print("wrote {} ndimage vectors and {} skimage.measure.label vectors".format(len(cases), len(ccomp)))
