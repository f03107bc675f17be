"""The yardstick of the structure-tensor family (no GPU): tests/helpers/corner_ref.py, the host transcription the device is held
to bit for bit, is itself held to scipy.ndimage.sobel -- its two NumPy restatements of the derivative stage (one 3-tap pass
at a time, as the generic kernels run it; every pass from the 3^rank samples around a voxel, as the fused kernel runs it) give
SciPy's bits for float32 and float64 in every mode SciPy has, with cval 0, 0.5 and 0.37, on the shapes the device tests use --
and it meets the known answers of tests/golden/corner_kat.json."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
from scipy import ndimage as sndi

from helpers import corner_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "corner_kat.json")) as _f:
    KAT = json.load(_f)

SHAPES = [(12, 20, 70), (9, 37, 64), (33, 18, 257), (3, 3, 3), (1, 5, 9), (2, 5, 1040), (70, 96), (5, 1040), (2, 2), (1, 7), (17,), (5, 6, 7, 8)]
MODES = R.MODES
CVALS = [0.37, 0.5]            # one that float32 cannot hold and one that it can


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def same_bits(got, want):
    """equal bit for bit, the sign of zeros included; a NaN matches a NaN (the sign and payload of a generated NaN are the
    processor's)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    view = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(view)[~nan], np.ascontiguousarray(want).view(view)[~nan])


@functools.lru_cache(maxsize=None)
def image_of(shape, dtype):
    rng = np.random.RandomState(len(shape) * 1000 + int(np.prod(shape)) % 997)
    if np.dtype(dtype).kind == "f":
        image = (rng.uniform(size=shape) * 4 - 1).astype(dtype)
    else:
        info = np.iinfo(dtype)
        image = rng.randint(info.min, info.max + 1, size=shape).astype(dtype)
    image.setflags(write=False)
    return image


def seam_index(shape):
    """a voxel on a seam of the small boxes (2 x 3 x 5 voxels, 3 x 5 pixels) along every axis that is long enough, and of the
    planner's boxes where the array has more than one"""
    small = {3: (2, 3, 5), 2: (3, 5)}.get(len(shape), (2,) * len(shape))
    big = {3: (8, 8, 64), 2: (32, 64)}.get(len(shape), small)
    return tuple(b if n > b else (s if n > s else n - 1) for n, s, b in zip(shape, small, big))


@functools.lru_cache(maxsize=None)
def planted_image(shape, dtype):
    """NaN, +inf, -inf and -0.0 on the border, one sample inside it, and on a box seam"""
    image = image_of(shape, dtype).copy()
    values = [np.nan, np.inf, -np.inf, -0.0]
    last = tuple(n - 1 for n in shape)
    inner = tuple(min(1, n - 1) for n in shape)
    inner_far = tuple(max(n - 2, 0) for n in shape)
    seam = seam_index(shape)
    spots = [(0,) * len(shape), last, inner, inner_far, seam, tuple(max(i - 1, 0) for i in seam)]
    for j, spot in enumerate(spots):
        image[spot] = values[j % 4]
    flat = image.reshape(-1)
    flat[flat.size // 2] = -0.0
    flat[flat.size // 3] = np.inf
    image.setflags(write=False)
    return image


def _cvals_for(mode):
    return [0.0] + CVALS if "constant" in mode else [CVALS[0]]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_both_formulations_equal_scipy_sobel_bit_for_bit(shape, dtype):
    for image in (image_of(shape, dtype), planted_image(shape, dtype)):
        for mode in MODES:
            w = R.neighbourhood(image, mode)
            for cval in _cvals_for(mode):
                want = R.derivatives(image, mode, cval)
                for axis in range(image.ndim):
                    with np.errstate(all="ignore"):
                        assert same_bits(sndi.sobel(image, axis=axis, mode=mode, cval=cval), want[axis])
                    assert same_bits(R.sobel_by_passes(image, axis, mode, cval), want[axis]), (mode, cval, axis, "passes")
                    assert same_bits(R.sobel_by_registers(image, axis, mode, cval, w), want[axis]), (mode, cval, axis, "registers")


def test_constant_mode_is_not_the_sobel_of_the_padded_image():
    """the trap the contract names: every pass extends its own line with cval, so with a cval other than 0 'constant' differs
    from the filter of the cval-padded array, while the index-mapped modes equal the filter of the mapped array"""
    image = image_of((9, 11), "float32")
    for mode, pad in (("reflect", "symmetric"), ("nearest", "edge"), ("mirror", "reflect"), ("wrap", "wrap")):
        padded = np.pad(image, 1, mode=pad)
        assert same_bits(sndi.sobel(padded, axis=0, mode="nearest")[1:-1, 1:-1], sndi.sobel(image, axis=0, mode=mode))
    padded = np.pad(image, 1, mode="constant", constant_values=np.float32(0.37))
    assert not same_bits(sndi.sobel(padded, axis=0, mode="nearest")[1:-1, 1:-1], sndi.sobel(image, axis=0, mode="constant", cval=0.37))


def test_an_infinite_centre_sample_gives_nan():
    image = np.zeros((5, 5), np.float32)
    image[2, 2] = np.inf
    d = R.derivatives(image, "reflect", 0)[0]
    assert np.isnan(d[2, 2]) and same_bits(R.sobel_by_passes(image, 0, "reflect", 0.0), d)


# ---------------------------------------------------------------- known answers
def _take(element, index):
    if index is None:
        return element
    return element[tuple(slice(None) if i is None else i for i in index)]


def check_structure_case(case, structure_tensor):
    """`structure_tensor(image, sigma=, order=)` returns host arrays"""
    image = np.asarray(case["image"], dtype=np.float64)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        elems = structure_tensor(image, sigma=case["sigma"], order=case["order"])
    future = [w for w in caught if issubclass(w.category, FutureWarning)]
    if case.get("warns"):
        assert any(case["warns"] in str(w.message) for w in future)
    else:
        assert not future
    if "count" in case:
        assert len(elems) == case["count"]
    for e in case["expected"]:
        got = _take(np.asarray(elems[e["element"]]), e["index"])
        assert np.array_equal(got, np.asarray(e["values"], dtype=np.float64)), (case["name"], e["element"], e["index"])


def check_finite_case(case, detectors):
    image = np.zeros(case["shape"])
    for name in case["detectors"]:
        out = detectors[name](image)
        for o in (out if isinstance(out, tuple) else (out,)):
            assert np.isfinite(np.asarray(o)).all(), name


def maximum_image(case):
    image = np.zeros(case["shape"])
    image[tuple(slice(a, b) for a, b in case["ones"])] = 1
    return image


def has_unique_maximum_at(response, at):
    response = np.asarray(response)
    peak = response.max()
    return int(np.count_nonzero(response == peak)) == 1 and tuple(np.argwhere(response == peak)[0]) == tuple(at)


def _host_structure_tensor(image, sigma=1, mode="constant", cval=0, order=None):
    """the transcription behind the public signature: the default order's warning included"""
    image = np.asarray(image)
    if order == "xy" and image.ndim > 2:
        raise ValueError('Only "rc" order is supported for dim > 2.')
    if order is None:
        if image.ndim == 2:
            warnings.warn("the default order of the structure tensor values will change", FutureWarning)
            order = "xy"
        else:
            order = "rc"
    return R.structure_tensor(image, sigma, mode, cval, order)


HOST_DETECTORS = {name: functools.partial(R.detector, name) for name in
                  ("corner_harris", "corner_shi_tomasi", "corner_foerstner", "corner_kitchen_rosenfeld")}


@functools.lru_cache(maxsize=None)
def admitted_maximum_cases():
    """(case name, detector) of the "global maximum lies at ..." candidates the transcription confirms with a unique maximum"""
    admitted = []
    for case in KAT["maximum"]:
        for name in case["detectors"]:
            if has_unique_maximum_at(HOST_DETECTORS[name](maximum_image(case)), case["at"]):
                admitted.append((case["name"], name))
    return tuple(admitted)


@pytest.mark.parametrize("case", KAT["structure_tensor"], ids=[c["name"] for c in KAT["structure_tensor"]])
def test_transcription_meets_the_structure_tensor_answers(case):
    check_structure_case(case, _host_structure_tensor)


def test_transcription_meets_the_other_answers():
    for case in KAT["raises"]:
        with pytest.raises(ValueError):
            _host_structure_tensor(np.zeros(case["shape"]), sigma=case["sigma"], order=case["order"])
    for case in KAT["finite"]:
        check_finite_case(case, HOST_DETECTORS)
    # the candidates are symmetric images: a maximum that is not unique, or not where the reference's peak finder reported
    # it, is not a known answer of the response itself and is left to the pull request that brings peak_local_max
    names = {c["name"] for c in KAT["maximum"]}
    assert all(n in names for n, _ in admitted_maximum_cases())


def test_responses_keep_the_dtype_rules():
    """a float32 tensor gives float32 Harris and Shi-Tomasi responses (k and eps are weak scalars); Foerstner and
    Kitchen-Rosenfeld are float64 whatever the image"""
    image = image_of((70, 96), "float32")
    elems = R.structure_tensor(image, 1)
    assert all(e.dtype == np.float32 for e in elems)
    assert R.corner_harris(*elems).dtype == np.float32 and R.corner_harris(*elems, method="eps").dtype == np.float32
    assert R.corner_shi_tomasi(*elems).dtype == np.float32
    assert all(o.dtype == np.float64 for o in R.corner_foerstner(*elems))
    assert R.corner_kitchen_rosenfeld(image).dtype == np.float64
    assert R.structure_tensor(image_of((70, 96), "uint8"), 1)[0].dtype == np.float64
