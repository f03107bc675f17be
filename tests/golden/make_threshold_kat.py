"""Writes tests/golden/threshold_kat.json: the literal inputs and stated expectations of the reference's thresholding tests
(cupyimg/skimage/filters/tests/test_thresholding.py) that need no skimage.data image, as data, each with its file:line.
Nothing here calls the library or the reference.  Inputs the reference's tests build with a few NumPy calls are kept as
recipes (tests/helpers/threshold_ref.py kat_image turns them into arrays); inf and nan are written as strings.

    python tests/golden/make_threshold_kat.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

SIMPLE = [[0, 0, 1, 3, 5],
          [0, 1, 4, 3, 4],
          [1, 2, 5, 4, 1],
          [2, 4, 5, 2, 1],
          [4, 5, 1, 0, 0]]
F, T = False, True


def simple(dtype="int64", shift=0):
    return dict(data=[[v + shift for v in row] for row in SIMPLE], dtype=dtype)


def build():
    cases = []

    def add(name, ref, function, image, expect, **kwargs):
        cases.append(dict(name=name, ref="test_thresholding.py:" + ref, function=function, image=image, kwargs=kwargs, expect=expect))

    eq = lambda v: dict(kind="equals", value=v)
    between = lambda lo, hi, closed=False: dict(kind="between", low=lo, high=hi, low_closed=closed)
    raises = lambda e: dict(kind="raises", error=e)
    mask = lambda m: dict(kind="mask_above", value=m)

    # ---- TestSimpleImage
    add("simple_minimum", "56-58", "threshold_minimum", simple(), raises("RuntimeError"))
    add("simple_otsu", "68-69", "threshold_otsu", simple(), eq(2))
    add("simple_otsu_negative_int", "71-73", "threshold_otsu", simple(shift=-2), eq(0))
    add("simple_otsu_float", "75-77", "threshold_otsu", simple("float64"), between(2, 3, True))
    add("simple_li", "79-80", "threshold_li", simple(), between(2, 3))
    add("simple_li_negative_int", "82-84", "threshold_li", simple(shift=-2), between(0, 1))
    add("simple_li_float", "86-88", "threshold_li", simple("float64"), between(2, 3))
    add("li_constant_image", "90-91", "threshold_li", dict(recipe="full", shape=[10, 10], value=1.0, dtype="float64"), eq(1.0))
    add("simple_yen", "93-94", "threshold_yen", simple(), eq(2))
    add("simple_yen_negative_int", "96-98", "threshold_yen", simple(shift=-2), eq(0))
    add("simple_yen_float", "100-102", "threshold_yen", simple("float64"), between(2, 3, True))
    add("yen_arange", "104-106", "threshold_yen", dict(recipe="arange", n=256, dtype="int64"), eq(127))
    add("yen_binary", "108-111", "threshold_yen",
        dict(recipe="rows", base=dict(recipe="full", shape=[2, 256], value=0, dtype="uint8"), set_rows=[[0, 1, 255]]), dict(kind="below", value=1))
    add("yen_blank_zero", "113-115", "threshold_yen", dict(recipe="full", shape=[5, 5], value=0, dtype="uint8"), eq(0))
    add("yen_blank_max", "117-120", "threshold_yen", dict(recipe="full", shape=[5, 5], value=255, dtype="uint8"), eq(255))
    add("simple_isodata", "122-123", "threshold_isodata", simple(), eq(2))
    add("simple_isodata_all", "124", "threshold_isodata", simple(), dict(kind="array_equal", value=[2]), return_all=True)
    add("isodata_blank_zero", "126-128", "threshold_isodata", dict(recipe="full", shape=[5, 5], value=0, dtype="uint8"), eq(0))
    add("isodata_blank_zero_all", "129", "threshold_isodata", dict(recipe="full", shape=[5, 5], value=0, dtype="uint8"),
        dict(kind="array_equal", value=[0]), return_all=True)
    lin = dict(recipe="linspace", start=-127, stop=0, n=256)
    add("isodata_linspace", "131-133", "threshold_isodata", lin, between(-63.8, -63.6))
    add("isodata_linspace_all", "134-137", "threshold_isodata", lin, dict(kind="array_almost_equal", value=[-63.74804688, -63.25195312]),
        return_all=True)
    rnd = dict(recipe="legacy_rand", seed=0, shape=[256, 256])
    add("isodata_16bit", "139-142", "threshold_isodata", rnd, between(0.49, 0.51), nbins=1024)
    add("isodata_16bit_all", "143-145", "threshold_isodata", rnd, dict(kind="all_above", value=0.49), nbins=1024, return_all=True)
    local_ref = [[F, F, F, F, T], [F, F, T, F, T], [F, F, T, T, F], [F, T, T, F, F], [T, T, F, F, F]]
    add("local_gaussian", "147-158", "threshold_local", simple(), mask(local_ref), block_size=3, method="gaussian")
    add("local_gaussian_param", "160-161", "threshold_local", simple(), mask(local_ref), block_size=3, method="gaussian", param=1.0 / 3.0)
    add("local_mean", "163-174", "threshold_local", simple(), mask(local_ref), block_size=3, method="mean")
    add("local_median", "176-187", "threshold_local", simple(),
        mask([[F, F, F, F, T], [F, F, T, F, F], [F, F, T, F, F], [F, F, T, T, F], [F, T, F, F, F]]), block_size=3, method="median")
    add("local_median_constant", "189-201", "threshold_local", simple(),
        dict(kind="array_equal", value=[[20., 1., 3., 4., 20.], [1., 1., 3., 4., 4.], [2., 2., 4., 4., 4.], [4., 4., 4., 1., 2.],
                                        [20., 5., 5., 2., 20.]]), block_size=3, method="median", mode="constant", cval=20)
    add("simple_niblack", "203-215", "threshold_niblack", simple(),
        mask([[F, F, F, T, T], [F, T, T, T, T], [F, T, T, T, F], [F, T, T, T, T], [T, T, F, F, F]]), window_size=3, k=0.5)
    sauvola_ref = [[F, F, F, T, T], [F, F, T, T, T], [F, F, T, T, F], [F, T, T, T, F], [T, T, F, F, F]]
    add("simple_sauvola", "217-229", "threshold_sauvola", simple(), mask(sauvola_ref), window_size=3, k=0.2, r=128)
    add("simple_niblack_iterable", "231-243", "threshold_niblack", simple(),
        mask([[F, F, F, T, T], [F, F, T, T, T], [F, T, T, T, F], [F, T, T, T, F], [T, T, F, F, F]]), window_size=[3, 5], k=0.5)
    add("simple_sauvola_iterable", "245-257", "threshold_sauvola", simple(), mask(sauvola_ref), window_size=[3, 5], k=0.2, r=128)

    # ---- the module-level cases
    add("otsu_one_color", "296-298", "threshold_otsu", dict(recipe="full", shape=[10, 10], value=1, dtype="uint8"), eq(1))
    add("otsu_one_color_3d", "301-303", "threshold_otsu", dict(recipe="full", shape=[10, 10, 10], value=1, dtype="uint8"), eq(1))
    add("li_nan_image", "346-348", "threshold_li", dict(recipe="full", shape=[5, 5], value="nan", dtype="float64"), dict(kind="isnan"))
    add("li_inf_image", "351-353", "threshold_li", dict(data=["inf", "nan"], dtype="float64"), eq("inf"))
    add("li_inf_minus_inf", "356-358", "threshold_li", dict(data=["inf", "-inf"], dtype="float64"), eq(0))
    add("li_constant_with_nan", "361-363", "threshold_li", dict(data=[8, 8, 8, 8, "nan"], dtype="float64"), eq(8))
    for tag, data, dtype in (("a", [0, 0, 1, 0, 0, 1, 0, 1], "int64"), ("b", [0, 0, 0.1, 0, 0, 0.1, 0, 0.1], "float64"),
                             ("c", [0, 0, 0.1, 0, 0, 0.1, 0.01, 0.1], "float64"), ("d", [0, 0, 1, 0, 0, 1, 0.5, 1], "float64"),
                             ("e", [1, 1], "int64"), ("f", [1, 2], "int64")):
        add("li_pathological_" + tag, "383-393", "threshold_li", dict(data=data, dtype=dtype), dict(kind="finite"))
    add("local_even_block_size", "426-429", "threshold_local", dict(recipe="full", shape=[8, 8], value=0, dtype="uint8"), raises("ValueError"),
        block_size=4)
    synth = dict(recipe="rows", base=dict(recipe="arange", n=625, dtype="uint8", shape=[25, 25]), set_rows=[[0, 9, 50], [14, 25, 250]])
    add("minimum_synthetic", "577-583", "threshold_minimum", synth, eq(95))
    add("minimum_failure", "586-589", "threshold_minimum", dict(recipe="full", shape=[256], value=0, dtype="uint8"), raises("RuntimeError"))
    add("mean", "592-596", "threshold_mean",
        dict(recipe="columns", base=dict(recipe="full", shape=[2, 6], value=0.0, dtype="float64"), set_columns=[[2, 4, 1], [4, 6, 2]]), eq(1.0))
    add("niblack_pathological", "697-704", "threshold_niblack",
        dict(recipe="full", shape=[4, 4], value=0.03082192 + 2.19178082e-09, dtype="float64"), dict(kind="no_nan"))
    quarter = dict(recipe="scaled", factor=0.25, base=dict(data=[[0, 1, 2, 3, 4]] * 4, dtype="float64"))
    for classes in (3, 4, 5):
        add("multiotsu_lengths_{}".format(classes), "717-726", "threshold_multiotsu", quarter, dict(kind="length", value=classes - 1), classes=classes)
    discs = dict(recipe="discs", shape=[100, 100], dtype="int64", centers=[[25, 25], [50, 50], [75, 75]], radii=[20, 20, 20], values=[64, 128, 192])
    add("multiotsu_discs", "729-738", "threshold_multiotsu", discs, dict(kind="array_equal", value=[0, 64, 128]), classes=4)
    ones = dict(recipe="full", shape=[10, 10], value=1, dtype="uint8")
    add("multiotsu_one_value_two_classes", "747-750", "threshold_multiotsu", ones, raises("ValueError"), classes=2)
    two = dict(recipe="columns", base=ones, set_columns=[[3, 10, 2]])
    add("multiotsu_two_values_three_classes", "751-753", "threshold_multiotsu", two, raises("ValueError"), classes=3)
    three = dict(recipe="columns", base=ones, set_columns=[[3, 10, 2], [6, 10, 3]])
    add("multiotsu_three_values_four_classes", "754-756", "threshold_multiotsu", three, raises("ValueError"), classes=4)
    return dict(source="cupyimg/skimage/filters/tests/test_thresholding.py", cases=cases)


def dumps():
    return json.dumps(build(), indent=1) + "\n"


def main():
    with open(os.path.join(HERE, "threshold_kat.json"), "w") as f:
        f.write(dumps())


if __name__ == "__main__":
    main()
