"""skimage.feature.match_template on the device (csrc/template.hip) against the transcription of tests/helpers/template_ref.py
under the three settings of mi_debug_set_match_template: the planner's tiles (mt_fused_kernel), the per-output kernel
(mt_generic_kernel), and the fused kernel on small tiles with a 4 KiB staging budget (seams along every axis of a small array,
templates walked in slabs).  The route is read back from last_kernel().

Integer-valued data: x, s1 and s2 are exact in any order of summation, so the result must equal the transcription bit for bit.
Real data: the routes are bit-identical to each other, and every output lies within the per-output bound of
template_ref.error_bound of the long-double transcription; the largest error-to-bound ratio seen is printed."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from helpers import dirty_pool
from helpers import template_ref as R

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "template_kat.json")))

ROUTES = {"planner": 0, "generic": 1, "small": 2}
# x crossing a 64-lane wave, rows no multiple of anything, even and odd templates, a template larger than any halo of the other
# families, template == image (one output unpadded, more than one bounce padded), axes of extent 1 and 2, a unit template axis;
# the last 2-D case's staged box is larger than the planner's 64 KiB: its template is walked in slabs of rows
CASES = [((5, 7), (2, 3)), ((2, 9), (1, 4)), ((13, 67), (3, 5)), ((37, 70), (5, 9)), ((33, 40), (16, 17)), ((12, 12), (12, 12)),
         ((30, 70), (29, 60)),
         ((3, 5, 7), (2, 2, 3)), ((9, 21, 67), (3, 4, 5)), ((6, 6, 6), (6, 6, 6)), ((17, 18, 19), (9, 1, 8))]
CASE_IDS = ["x".join(map(str, i)) + "-" + "x".join(map(str, t)) for i, t in CASES]
# (setting, image shape, template shape) -> the slab walk last_kernel() must name (worked out from the tile, the padded row
# pitch and the budget of csrc/template.hip); every other fused launch of CASES stages its whole box: "slabs=none"
SLABS = {("planner", (30, 70), (29, 60)): "slabs=rows:28", ("planner", (6, 6, 6), (6, 6, 6)): "slabs=planes:4",
         ("small", (33, 40), (16, 17)): "slabs=rows:14", ("small", (30, 70), (29, 60)): "slabs=rows:4",
         ("small", (6, 6, 6), (6, 6, 6)): "slabs=planes:2", ("small", (17, 18, 19), (9, 1, 8)): "slabs=planes:7"}
MODES = ["constant", "edge", "reflect", "symmetric", "wrap"]
# (pad_input, mode, constant_values): unpadded once, every mode padded, 'constant' with 0 and with 3
SETTINGS = [(False, "constant", 0)] + [(True, m, 0) for m in MODES] + [(True, "constant", 3)]
TNAME = {"uint8": "uint8", "uint16": "uint16", "int16": "int16", "float32": "float32", "float64": "float64"}


@pytest.fixture(scope="module")
def match(gpu):
    from cupyimg_amd.skimage.feature import match_template
    return match_template


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_match_template
    fn.argtypes = [ctypes.c_int]
    yield lambda route: fn(ROUTES[route])
    fn(0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_route(gpu, route, ishape, tshape, dtype):
    name = gpu.last_kernel()
    kernel = "mt_generic_kernel" if route == "generic" else "mt_fused_kernel"
    assert "{}<{},{}>".format(kernel, TNAME[np.dtype(dtype).name], len(ishape)) in name and "one launch" in name, (route, name)
    if route != "generic":
        assert SLABS.get((route, tuple(ishape), tuple(tshape)), "slabs=none") + " " in name, (route, name)
        tile = ((2, 3, 8) if len(ishape) == 3 else (1, 3, 8)) if route == "small" else ((2, 4, 128) if len(ishape) == 3 else (1, 8, 128))
        assert "tile={}x{}x{} ".format(*tile) in name, (route, name)


def run(gpu, match, knob, route, image, template, pad_input=False, mode="constant", constant_values=0, native=None):
    """the result as a host array; the route is checked when `native` names the dtype the kernel loads"""
    knob(route)
    out = match(image, template, pad_input=pad_input, mode=mode, constant_values=constant_values)
    if native is not None:
        check_route(gpu, route, np.shape(image) if not hasattr(image, "shape") else image.shape,
                    np.shape(template) if not hasattr(template, "shape") else template.shape, native)
    assert out.dtype == np.float64 and out._is_c_contiguous()
    return out.get()


# ------------------------------------------------------------------ inputs and references, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def integer_inputs(case, dtype):
    ishape, tshape = CASES[case]
    rng = np.random.default_rng(1000 + case)
    lo, hi = (-300, 300) if dtype == "int16" else (0, 255)
    image = rng.integers(lo, hi + 1, size=ishape).astype(dtype)
    template = rng.integers(-4, 5, size=tshape).astype(np.float64 if dtype == "float64" else np.int16 if dtype == "int16" else np.float32)
    if template.size > 1 and template.min() == template.max():
        template.flat[0] += 1
    image.setflags(write=False)
    template.setflags(write=False)
    return image, template


@functools.lru_cache(maxsize=None)
def integer_want(case, dtype, setting):
    image, template = integer_inputs(case, dtype)
    want = R.match_template(image, template, *setting)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def real_inputs(case, dtype):
    ishape, tshape = CASES[case]
    rng = np.random.default_rng(2000 + case)
    image = (rng.random(ishape) + 0.25).astype(dtype)
    template = rng.random(tshape).astype(dtype)
    image.setflags(write=False)
    template.setflags(write=False)
    return image, template


@functools.lru_cache(maxsize=None)
def real_want(case, dtype, setting):
    image, template = real_inputs(case, dtype)
    r, sums = R.match_template_longdouble(image, template, *setting)
    return r, R.error_bound(r, sums), R.conditioning(sums)


# ------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("route", list(ROUTES))
def test_known_answers(gpu, match, knob, route):
    k = KAT["docstring"]
    image, template = np.array(k["image"]), np.array(k["template"])
    assert np.array_equal(np.round(run(gpu, match, knob, route, image, template, native="float64"), k["decimals"]), np.array(k["expected"]))
    assert np.array_equal(np.round(run(gpu, match, knob, route, image, template, pad_input=True), k["decimals"]),
                          np.array(k["expected_pad_input"]))

    k = KAT["normalization"]
    r = run(gpu, match, knob, route, np.array(k["image"]), np.array(k["template"]))
    assert list(np.unravel_index(int(r.argmin()), r.shape)) == k["argmin"] and list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax"]
    assert np.allclose(r.min(), k["min"]) and np.allclose(r.max(), k["max"])

    k = KAT["pad_input"]
    r = run(gpu, match, knob, route, np.array(k["image"]), np.array(k["template"]), pad_input=True, constant_values=k["constant_values"])
    order = np.argsort(r.ravel(), kind="stable")
    assert list(np.unravel_index(order[:2], r.shape)[1]) == k["lowest_two_columns"]
    assert list(np.unravel_index(order[-2:], r.shape)[1]) == k["highest_two_columns"]

    k = KAT["volume"]
    template = np.array(k["template"])
    image = np.zeros(k["image_shape"])
    z, y, x = k["planted_at"]
    image[z:z + 3, y:y + 3, x:x + 3] = template
    r = run(gpu, match, knob, route, image, template, native="float64")
    assert list(r.shape) == k["shape"] and list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax"]
    r = run(gpu, match, knob, route, image, template, pad_input=True)
    assert list(r.shape) == k["shape_pad_input"] and list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax_pad_input"]

    k = KAT["padding_reflect"]
    r = run(gpu, match, knob, route, np.array(k["image"]), np.array(k["template"]), pad_input=True, mode=k["mode"])
    assert list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax"]

    k = KAT["no_nans"]
    image = 0.5 + k["scale"] * np.random.RandomState(k["seed"]).normal(size=k["shape"])
    template = np.ones(k["template_shape"])
    template[:k["zero_rows"], :] = 0
    assert not np.isnan(run(gpu, match, knob, route, image, template)).any()


@pytest.mark.parametrize("route", ["planner", "generic"])
def test_known_answer_two_planted_targets(gpu, match, knob, route):
    """the reference's test_template: peak_local_max of the response finds both targets"""
    from cupyimg_amd.skimage.feature import peak_local_max
    k = KAT["planted"]
    size = k["size"]
    image = np.full(k["shape"], 0.5)
    target = 0.1 * (np.tri(size) + np.tri(size)[::-1])
    for y, x in k["positions"]:
        image[y:y + size, x:x + size] = target
    image += 0.1 * np.random.RandomState(k["seed"]).uniform(size=k["shape"])
    knob(route)
    result = match(gpu.asarray(image), gpu.asarray(target))
    name = gpu.last_kernel()
    assert ("mt_generic_kernel<float64,2>" in name) if route == "generic" else ("mt_fused_kernel<float64,2>" in name and "slabs=rows:" in name), name
    positions = peak_local_max(result, min_distance=k["min_distance"]).get()
    values = result.get()[tuple(positions.T)]
    best = positions[np.argsort(values)[::-1][:2]]
    assert sorted(map(list, best)) == sorted(k["positions"])


# ------------------------------------------------------------------ 2. exact
@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32", "float64"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_integer_data_bit_for_bit(gpu, match, knob, case, dtype):
    image, template = integer_inputs(case, dtype)
    x, t = gpu.asarray(image), gpu.asarray(template)
    for setting in SETTINGS:
        want = integer_want(case, dtype, setting)
        got = {route: run(gpu, match, knob, route, x, t, *setting, native=dtype) for route in ROUTES}
        for route, g in got.items():
            assert g.shape == want.shape and same_bits(g, want), (route, setting, int((g != want).sum()))


@pytest.mark.parametrize("dtype", ["bool", "int8", "uint16", "float16", "int32", "uint32", "int64", "uint64"])
def test_converted_dtypes_bit_for_bit(gpu, match, knob, dtype):
    """dtypes the kernels do not load are converted on the device, at their values: bool and float16 as they are"""
    rng = np.random.default_rng(77)
    if dtype == "bool":
        image = rng.random((13, 67)) < 0.5
    elif dtype == "float16":
        image = (rng.integers(-64, 65, size=(13, 67)) / 4).astype(dtype)
    else:
        image = rng.integers(max(np.iinfo(dtype).min, -1000), min(np.iinfo(dtype).max, 1000) + 1, size=(13, 67)).astype(dtype)
    template = rng.integers(-3, 4, size=(3, 5)).astype(np.int8)
    want = R.match_template(image, template, True, "symmetric")
    for route in ROUTES:
        got = run(gpu, match, knob, route, gpu.asarray(image), template, True, "symmetric")
        assert same_bits(got, want), (route, dtype)


# ------------------------------------------------------------------ 3. real data
_ratios = {}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_real_data_routes_agree_and_meet_the_bound(gpu, match, knob, case, dtype):
    image, template = real_inputs(case, dtype)
    x, t = gpu.asarray(image), gpu.asarray(template)
    worst = 0.0
    for setting in SETTINGS:
        want, bound, cond = real_want(case, dtype, setting)
        assert cond.min() >= 1e-3, (setting, float(cond.min()))          # nothing is ill-conditioned: no output is skipped
        got = {route: run(gpu, match, knob, route, x, t, *setting, native=dtype) for route in ROUTES}
        assert same_bits(got["planner"], got["generic"]) and same_bits(got["planner"], got["small"]), setting
        ratio = float((np.abs(got["planner"] - want) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (setting, ratio)
    _ratios[(case, dtype)] = worst
    print("match_template error / bound: case {} {} worst {:.4f} (all cases so far {:.4f})".format(CASE_IDS[case], dtype, worst, max(_ratios.values())))


# ------------------------------------------------------------------ 4. meaning
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("ishape, tshape, at", [((37, 70), (5, 9), (20, 43)), ((9, 21, 67), (3, 4, 5), (5, 11, 60))])
def test_template_cut_from_the_image(gpu, match, knob, route, ishape, tshape, at):
    rng = np.random.default_rng(31)
    image = rng.random(ishape) + 0.25
    template = image[tuple(slice(a, a + t) for a, t in zip(at, tshape))].copy()
    rl, sums = R.match_template_longdouble(image, template)
    bound = R.error_bound(rl, sums)[at]
    r = run(gpu, match, knob, route, image, template, native="float64")
    assert np.unravel_index(int(r.argmax()), r.shape) == at and abs(r[at] - 1.0) <= bound
    rl, sums = R.match_template_longdouble(image, -template)
    bound = R.error_bound(rl, sums)[at]
    r = run(gpu, match, knob, route, image, -template)
    assert np.unravel_index(int(r.argmin()), r.shape) == at and abs(r[at] + 1.0) <= bound


@pytest.mark.parametrize("route", list(ROUTES))
def test_peak_local_max_finds_two_planted_copies(gpu, match, knob, route):
    from cupyimg_amd.skimage.feature import peak_local_max
    rng = np.random.default_rng(32)
    image = rng.random((37, 70)).astype(np.float32)
    template = rng.random((5, 9)).astype(np.float32) + 2.0
    for y, x in ((4, 50), (25, 11)):
        image[y:y + 5, x:x + 9] = template
    knob(route)
    result = match(gpu.asarray(image), gpu.asarray(template), pad_input=True)
    peaks = peak_local_max(result, min_distance=3, threshold_abs=0.99).get()
    assert sorted(map(tuple, peaks)) == [(6, 54), (27, 15)]


# ------------------------------------------------------------------ 5. degenerate
@pytest.mark.parametrize("route", list(ROUTES))
def test_degenerate_inputs(gpu, match, knob, route):
    rng = np.random.default_rng(33)
    template = rng.integers(0, 9, size=(3, 5)).astype(np.float32)
    # constant blocks larger than the template: exactly 0.0 wherever the window lies inside one
    image = rng.integers(0, 200, size=(37, 70)).astype(np.int16)
    image[5:15, 20:40] = 7
    image[20:30, 3:30] = -11
    r = run(gpu, match, knob, route, image, template, native="int16")
    assert same_bits(r, R.match_template(image, template))
    assert not r[5:13, 20:36].any() and not r[20:28, 3:26].any() and not np.signbit(r[5:13, 20:36]).any()
    # a constant image, a constant template (ssd == 0): all zeros
    for setting in SETTINGS:
        if not (setting[0] and setting[1] == "constant"):           # padded with another constant the border windows are not constant
            assert not run(gpu, match, knob, route, np.full((13, 67), 3.25, np.float32), template, *setting).any()
        assert not run(gpu, match, knob, route, image, np.full((3, 5), 2.0), *setting).any()
    assert not run(gpu, match, knob, route, np.full((13, 67), 3.0, np.float32), template, True, "constant", 3).any()
    assert not run(gpu, match, knob, route, np.full((9, 21, 67), 200, np.uint8), np.arange(60.0).reshape(3, 4, 5), True, "reflect").any()
    # one NaN and one infinity: 0.0 where the window touches them, the transcription's value everywhere else
    for dtype in ("float32", "float64"):
        bad = rng.integers(-50, 50, size=(37, 70)).astype(dtype)
        bad[10, 20] = np.nan
        bad[30, 60] = np.inf
        for setting in ((False, "constant", 0), (True, "symmetric", 0)):
            r = run(gpu, match, knob, route, bad, template, *setting, native=dtype)
            want = R.match_template(bad, template, *setting)
            touched = ~np.isfinite(R.windows(bad, template.shape, setting[0], setting[1])).all(axis=(-2, -1))
            assert touched.any() and not want[touched].any()
            assert not np.isnan(r).any() and same_bits(r, want)


# ------------------------------------------------------------------ 6. memory
@pytest.mark.parametrize("route", list(ROUTES))
def test_strided_views(gpu, match, knob, route):
    rng = np.random.default_rng(34)
    big = rng.integers(0, 255, size=(26, 201)).astype(np.uint8)
    tbig = rng.integers(-4, 5, size=(6, 10)).astype(np.float32)
    image, template = big[::2, 1::3], tbig[::2, ::2]
    want = R.match_template(image, template, True, "reflect")
    dev_image, dev_template = gpu.asarray(big)[::2, 1::3], gpu.asarray(tbig)[::2, ::2]
    assert not dev_image._is_c_contiguous() and not dev_template._is_c_contiguous()
    assert same_bits(run(gpu, match, knob, route, dev_image, dev_template, True, "reflect"), want)
    assert same_bits(run(gpu, match, knob, route, image, template, True, "reflect"), want)          # strided on the host
    assert same_bits(run(gpu, match, knob, route, image.tolist(), template.tolist(), True, "reflect"), want.astype(np.float64))


@pytest.mark.parametrize("route", list(ROUTES))
def test_poisoned_pool_memory(gpu, match, knob, route):
    """every output is written, and nothing is read before it is written: the whole result under every fill byte"""
    case = CASE_IDS.index("9x21x67-3x4x5")
    image, template = integer_inputs(case, "uint8")
    x, t = gpu.asarray(image), gpu.asarray(template)
    gpu.synchronize()
    for setting in ((False, "constant", 0), (True, "wrap", 0)):
        want = integer_want(case, "uint8", setting)
        for byte in dirty_pool.FILLS:
            with dirty_pool.pool_fill(gpu, byte):
                got = run(gpu, match, knob, route, x, t, *setting, native="uint8")
            assert same_bits(got, want), (setting, hex(byte))
