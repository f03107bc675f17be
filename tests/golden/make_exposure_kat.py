#!/usr/bin/env python3
"""Writes tests/golden/exposure_kat.json: the literal known-answer vectors of the reference's exposure tests that need no
image download (data only -- inputs, arguments and the expectation the reference test states, each with the reference
file:line it is transcribed from).

* cupyimg/skimage/exposure/tests/test_exposure.py: the histogram vectors (test_negative_overflow ... test_normalize) and
  the test_rescale_* family, except the two items that state no vector: test_rescale_nan_warning (302: a warning and a
  result that is NaN throughout) and test_rescale_raises_on_incorrect_out_range (345: an exception), which are tests of
  their own -- test_rescale_nan_is_broadcast in tests/test_exposure_yardstick.py and test_rescale_nan_warning in
  tests/test_gpu_exposure.py; test_rescale_raises_on_incorrect_out_range in tests/test_exposure_host.py.  The
  test_equalize_* functions of that file all start from skimage.data.camera(), which is a
  download; their properties are checked on synthetic images in tests/test_exposure_yardstick.py instead.

"compare": "equal" = assert_array_equal, "almost" = assert_array_almost_equal (6 decimals), as the reference test does.

    python tests/golden/make_exposure_kat.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "cupyimg/skimage/exposure/tests/test_exposure.py:"
U10, U12, U14, U16 = 2 ** 10 - 1, 2 ** 12 - 1, 2 ** 14 - 1, 2 ** 16 - 1

rescale = [
    # name, line, image, dtype, kwargs, expected, expected dtype (None: not stated), compare
    ("rescale_stretch", 217, [51, 102, 153], "uint8", {}, [0, 127, 255], "uint8", "almost"),
    ("rescale_shrink", 224, [51.0, 102.0, 153.0], "float64", {}, [0, 0.5, 1], None, "almost"),
    ("rescale_in_range", 230, [51.0, 102.0, 153.0], "float64", {"in_range": [0, 255]}, [0.2, 0.4, 0.6], None, "almost"),
    ("rescale_in_range_clip", 236, [51.0, 102.0, 153.0], "float64", {"in_range": [0, 102]}, [0.5, 1, 1], None, "almost"),
    ("rescale_out_range", 242, [-10, 0, 10], "int8", {"out_range": [0, 127]}, [0, 63.5, 127], "float64", "almost"),
    ("rescale_named_in_range", 255, [0, U10, U10 + 100], "uint16", {"in_range": "uint10"}, [0, U16, U16], None, "almost"),
    ("rescale_named_out_range", 261, [0, U16], "uint16", {"out_range": "uint10"}, [0, U10], None, "almost"),
    ("rescale_uint12_limits", 267, [0, U16], "uint16", {"out_range": "uint12"}, [0, U12], None, "almost"),
    ("rescale_uint14_limits", 273, [0, U16], "uint16", {"out_range": "uint14"}, [0, U14], None, "almost"),
    ("rescale_all_zeros", 279, [[0, 0], [0, 0]], "uint8", {}, [[0, 0], [0, 0]], None, "almost"),
    ("rescale_constant", 286, [130, 130], "uint16", {"out_range": [0, 127]}, [127, 127], None, "almost"),
    ("rescale_same_values", 292, [[1.0, 1.0], [1.0, 1.0]], "float64", {}, [[1.0, 1.0], [1.0, 1.0]], None, "almost"),
    ("rescale_output_dtype_uint8", 325, [-128, 0, 127], "int8", {"out_range": "uint8"}, None, "uint8", None),
    ("rescale_output_dtype_uint10", 325, [-128, 0, 127], "int8", {"out_range": "uint10"}, None, "uint16", None),
    ("rescale_output_dtype_uint12", 325, [-128, 0, 127], "int8", {"out_range": "uint12"}, None, "uint16", None),
    ("rescale_output_dtype_uint16", 325, [-128, 0, 127], "int8", {"out_range": "uint16"}, None, "uint16", None),
    ("rescale_output_dtype_float", 325, [-128, 0, 127], "int8", {"out_range": "float"}, None, "float64", None),
    ("rescale_no_overflow", 331, [-128, 0, 127], "int8", {"out_range": "uint8"}, [0, 128, 255], "uint8", "equal"),
    ("rescale_float_output", 338, [-128, 0, 127], "int8", {"out_range": [0, 255]}, [0, 128, 255], "float64", "equal"),
]

# name, line, image, dtype, kwargs, centers as [start, stop) of an arange plus an offset, {index: count}, every other count 0 (or None), length
histogram = [
    ("negative_overflow", 28, [-1, 100], "int8", {}, [-1, 101, 0.0], {"0": 1, "-1": 1}, True, 102),
    ("all_negative_image", 37, [-100, -1], "int8", {}, [-100, 0, 0.0], {"0": 1, "-1": 1}, True, 100),
    ("int_range_image", 46, [10, 100], "int8", {}, [10, 101, 0.0], {}, False, 91),
    ("peak_uint_range_dtype", 54, [10, 100], "uint8", {"source_range": "dtype"}, [0, 256, 0.0], {"10": 1, "100": 1, "101": 0}, False, 256),
    ("peak_int_range_dtype", 64, [10, 100], "int8", {"source_range": "dtype"}, [-128, 128, 0.0], {"138": 1, "228": 1, "229": 0}, False, 256),
    ("peak_float_out_of_range_image", 88, [10, 100], "float16", {"nbins": 90}, [10, 100, 0.5], {}, False, 90),
    ("normalize_false", 106, [0, 255, 255], "uint8", {"source_range": "dtype", "normalize": False}, [0, 256, 0.0], {"0": 1, "-1": 2}, True, 256),
    ("normalize_true", 106, [0, 255, 255], "uint8", {"source_range": "dtype", "normalize": True}, [0, 256, 0.0],
     {"0": 1 / 3.0, "-1": 2 / 3.0}, True, 256),
]

cases = {"rescale_intensity": [], "histogram": []}
for name, line, image, dtype, kw, want, want_dtype, compare in rescale:
    cases["rescale_intensity"].append({"name": name, "cite": REF + str(line), "image": image, "dtype": dtype, "kwargs": kw,
                                       "expected": want, "expected_dtype": want_dtype, "compare": compare})
for name, line, image, dtype, kw, centers, counts, rest_zero, length in histogram:
    cases["histogram"].append({"name": name, "cite": REF + str(line), "image": image, "dtype": dtype, "kwargs": kw,
                               "centers_arange": centers, "counts": counts, "others_zero": rest_zero, "length": length})

with open(os.path.join(HERE, "exposure_kat.json"), "w") as f:
    json.dump(cases, f, indent=1)
    f.write("\n")
print("wrote", len(cases["rescale_intensity"]), "+", len(cases["histogram"]), "cases")
