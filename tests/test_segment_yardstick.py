"""The yardsticks of the segmentation tests, without a GPU: the host references of tests/helpers/segment_ref.py meet every
known answer of tests/golden/segment_kat.json (the literal cases of the reference's test_boundaries.py, test_join.py and
test_map_array.py and of its docstrings), the JSON is what its generator writes, and the two closed forms the kernels of
csrc/segment.hip evaluate equal the transcriptions of the reference on the case table the GPU tests share."""
import importlib.util
import json
import os

import numpy as np
import pytest

from helpers import segment_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_PATH = os.path.join(HERE, "golden", "segment_kat.json")
KAT = json.load(open(KAT_PATH))
KAT_CASES = KAT["cases"]
KAT_IDS = [c["name"] for c in KAT_CASES]
ERRORS = {"ValueError": ValueError, "TypeError": TypeError}


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def kat_array(spec):
    """the array a known-answer case describes: literal data, or one of the few recipes the reference's tests use"""
    if "data" in spec:
        return np.array(spec["data"], dtype=spec["dtype"])
    if spec["recipe"] == "box":
        a = np.zeros(spec["shape"], dtype=spec["dtype"])
        a[tuple(slice(lo, hi) for lo, hi in spec["box"])] = spec["value"]
        return a
    if spec["recipe"] == "sparse":
        a = np.zeros(spec["n"], dtype=spec["dtype"])
        for k, v in spec["pairs"]:
            a[k] = v
        return a
    if spec["recipe"] == "legacy_rand_round2":
        return np.round(np.random.RandomState(spec["seed"]).rand(*spec["shape"]), 2)
    raise KeyError(spec["recipe"])


# ------------------------------------------------------------------ the case table the GPU tests share
BOUNDARY_SHAPES = [(37, 41), (9, 7), (1, 23), (6, 67), (2, 2), (11, 12, 13), (3, 70, 5), (9, 10, 70), (50,), (5, 6, 7, 8)]
BOUNDARY_DTYPES = ["uint8", "uint16", "int16", "int32", "int64", "bool"]
BOUNDARY_MODES = ["thick", "inner", "outer"]
BACKGROUNDS = [0, 1]
LABEL_VALUES = (0, 1, 2, 5)


def shape_id(shape):
    return "x".join(map(str, shape))


def label_image(shape, dtype, variant, seed=7):
    """blocks of about three samples a side drawn from LABEL_VALUES.  variant "max": the largest label is the dtype's largest
    value; "negative" (signed dtypes): every label shifted down by 3."""
    rng = np.random.default_rng([seed, len(shape)] + list(shape))
    dtype = np.dtype(dtype)
    coarse = rng.integers(0, len(LABEL_VALUES), size=[(s + 2) // 3 for s in shape])
    for axis in range(len(shape)):
        coarse = np.repeat(coarse, 3, axis=axis)
    coarse = coarse[tuple(slice(0, s) for s in shape)]
    # single samples of another label, so that a window holds three labels now and then
    coarse = np.where(rng.random(shape) < 0.08, rng.integers(0, len(LABEL_VALUES), size=shape), coarse)
    if dtype == np.bool_:
        return coarse >= 2
    values = np.array(LABEL_VALUES, dtype=np.int64)
    if variant == "max":
        values[-1] = np.iinfo(dtype).max
    elif variant == "negative":
        values = values - 3
    return values[coarse].astype(dtype)


def variants(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return ["plain"]
    return ["plain", "max"] + (["negative"] if dtype.kind == "i" else [])


def boundary_settings(ndim):
    """(connectivity, mode, background) of every non-subpixel call on an image of this rank"""
    return [(c, m, b) for c in range(1, ndim + 1) for m in BOUNDARY_MODES for b in BACKGROUNDS]


_BOUNDARY_REFS = {}


def boundary_reference(shape, dtype, variant, connectivity, mode, background):
    """the transcription's answer, computed once and left unchanged"""
    key = (shape, dtype, variant, connectivity, mode, background)
    if key not in _BOUNDARY_REFS:
        labels = label_image(shape, dtype, variant)
        want = R.find_boundaries(labels, connectivity, mode, background) if mode != "subpixel" else R.find_boundaries_subpixel(labels)
        want.setflags(write=False)
        _BOUNDARY_REFS[key] = want
    return _BOUNDARY_REFS[key]


# ------------------------------------------------------------------ known answers
def check_kat(case, fb, mb, relabel, join, map_array_fn, ArrayMap, to_host, to_dev):
    """one known-answer case through a set of implementations (the host references, or the library's public functions)"""
    kind = case["kind"]
    if kind == "find_boundaries":
        got = to_host(fb(to_dev(kat_array(case["labels"])), **case["kwargs"]))
        assert got.dtype == np.bool_ and np.array_equal(got, np.array(case["expect"], dtype=bool))
    elif kind in ("mark_boundaries_mean", "mark_boundaries_ones"):
        kw = dict(case["kwargs"])
        marked = to_host(mb(to_dev(kat_array(case["image"])), to_dev(kat_array(case["labels"])), **kw))
        mean = marked.mean(axis=-1)
        if kind == "mark_boundaries_mean":
            assert np.array_equal(mean, np.array(case["expect"], dtype=np.float64))
        else:
            assert np.array_equal(np.round(mean, 2) == 1, np.array(case["expect"]) == 1)
    elif kind == "join_segmentations":
        s1, s2 = to_dev(kat_array(case["s1"])), to_dev(kat_array(case["s2"]))
        if "raises" in case:
            with pytest.raises(ERRORS[case["raises"]]):
                join(s1, s2)
        else:
            assert np.array_equal(to_host(join(s1, s2)), np.array(case["expect"]))
    elif kind == "relabel_sequential":
        labels = kat_array(case["labels"])
        if "raises" in case:
            with pytest.raises(ERRORS[case["raises"]]):
                relabel(to_dev(labels), offset=case["offset"])
            return
        relab, fw, inv = relabel(to_dev(labels), offset=case["offset"])
        relab_h = to_host(relab)
        if "relabeled_max" in case:
            assert int(relab_h.max()) == case["relabeled_max"]
            return
        assert np.array_equal(relab_h, np.array(case["relabeled"], dtype=object).astype(relab_h.dtype))
        assert np.array_equal(to_host(fw[to_dev(labels)]), relab_h) and np.array_equal(to_host(inv[relab]), labels)
        if "forward" in case:
            assert np.array_equal(np.asarray(fw), kat_array(case["forward"]))
            assert np.array_equal(np.asarray(inv), np.array(case["inverse"]))
        if "dtypes" in case:
            assert [str(relab_h.dtype), str(fw.dtype), str(inv.dtype)] == case["dtypes"]
    elif kind == "arraymap_len":
        labels = kat_array(case["labels"])
        relab, fw, inv = relabel(to_dev(labels), offset=1)
        assert len(fw) == case["forward_len"] == len(np.asarray(fw)) and len(inv) == case["inverse_len"] == len(np.asarray(inv))
        assert np.array_equal(to_host(fw(to_dev(labels))), to_host(relab)) and np.array_equal(to_host(inv(relab)), labels)
    elif kind == "map_array_raises":
        rng = np.random.default_rng(3)
        labels = rng.integers(0, 5, size=case["shape"])
        out = to_dev(np.zeros(case["out_shape"]))[tuple(slice(None, None, s) for s in case["out_step"])]
        in_values = np.unique(labels)
        with pytest.raises(ERRORS[case["raises"]]):
            map_array_fn(to_dev(labels), to_dev(in_values), to_dev(rng.random(in_values.shape)), out=out)
    elif kind == "arraymap_str_lines":
        values = np.arange(case["nvalues"])
        m = ArrayMap(to_dev(values), to_dev(np.random.default_rng(4).random(values.shape)))
        assert len(str(m).split("\n")) == case["lines"]
    else:
        raise KeyError(kind)


class HostArrayMap:
    """the host twin of ArrayMap the references are checked through"""

    def __init__(self, in_values, out_values):
        self.in_values, self.out_values = np.asarray(in_values), np.asarray(out_values)
        self.dtype = self.out_values.dtype

    def __len__(self):
        return int(self.in_values.max()) + 1

    def __array__(self, dtype=None, copy=None):
        return R.dense_map(self.in_values, self.out_values)

    def __getitem__(self, index):
        return R.map_array(index, self.in_values, self.out_values)

    __call__ = __getitem__

    def __str__(self):
        n = len(self.in_values)
        rows = list(range(n)) if n <= 5 else [0, 1, None, n - 2, n - 1]
        return "\n".join(["ArrayMap:"] + ["  ..." if i is None else "  {} → {}".format(self.in_values[i], self.out_values[i]) for i in rows])


def _host_mark(image, labels, color=(1, 1, 0), outline_color=None, mode="outer"):
    bd = R.find_boundaries(labels, mode=mode)
    if mode == "subpixel":
        # the zoomed image is not asked for: only the positions equal to the colour are compared
        out = np.zeros(bd.shape + (3,))
        out[bd] = color
        return out
    return np.repeat(R.mark_boundaries_mean(labels.shape, bd, color, outline_color)[..., None], 3, axis=-1)


def _host_relabel(labels, offset=1):
    relab, in_vals, out_vals = R.relabel_sequential(labels, offset)
    return relab, HostArrayMap(in_vals, out_vals), HostArrayMap(out_vals, in_vals)


def _host_map_array(input_arr, input_vals, output_vals, out=None):
    if out is not None and (out.shape != input_arr.shape or not out.flags.c_contiguous):
        raise ValueError("out")
    return R.map_array(input_arr, input_vals, output_vals)


@pytest.mark.parametrize("case", KAT_CASES, ids=KAT_IDS)
def test_references_meet_the_known_answers(case):
    check_kat(case, R.find_boundaries, _host_mark, _host_relabel, R.join_segmentations, _host_map_array, HostArrayMap, np.asarray, np.asarray)


def test_json_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("make_segment_kat", os.path.join(HERE, "golden", "make_segment_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert open(KAT_PATH).read() == mod.text()
    assert all(":" in c["ref"] for c in KAT_CASES)


# ------------------------------------------------------------------ the closed forms
@pytest.mark.parametrize("dtype", BOUNDARY_DTYPES)
@pytest.mark.parametrize("shape", BOUNDARY_SHAPES, ids=shape_id)
def test_closed_form_boundaries_equal_the_transcription(shape, dtype):
    for variant in variants(dtype):
        labels = label_image(shape, dtype, variant)
        if dtype != "bool" and labels.size > 30:
            assert len(np.unique(labels)) == len(LABEL_VALUES)
        for connectivity, mode, background in boundary_settings(len(shape)):
            want = boundary_reference(shape, dtype, variant, connectivity, mode, background)
            got = R.closed_form_boundaries(labels, connectivity, mode, background)
            assert same_bits(got, want), (variant, connectivity, mode, background, int((got != want).sum()))


@pytest.mark.parametrize("dtype", BOUNDARY_DTYPES)
@pytest.mark.parametrize("shape", [s for s in BOUNDARY_SHAPES if len(s) <= 3], ids=shape_id)
def test_closed_form_subpixel_equals_the_transcription(shape, dtype):
    for variant in variants(dtype):
        labels = label_image(shape, dtype, variant)
        want = boundary_reference(shape, dtype, variant, 1, "subpixel", 0)
        assert want.shape == tuple(2 * s - 1 for s in shape)
        assert same_bits(R.closed_form_subpixel(labels), want), variant


def test_closed_forms_keep_the_quirks():
    """a label equal to MAX, a background that is not the smallest label, and the image border between two equal labels"""
    labels = np.array([[255, 255, 3, 3], [255, 1, 1, 3], [0, 0, 1, 3]], np.uint8)
    for mode in BOUNDARY_MODES:
        for background in (0, 1, 3):
            assert same_bits(R.closed_form_boundaries(labels, 1, mode, background), R.find_boundaries(labels, 1, mode, background))
    ones = np.ones((2, 3), np.int16)
    sub = R.find_boundaries_subpixel(ones)
    assert sub[0, 1] and sub[1, 0] and not sub[1, 1] and same_bits(R.closed_form_subpixel(ones), sub)


def test_int64_join_differs_from_the_wrapping_one_only_where_it_wraps():
    rng = np.random.default_rng(5)
    small1, small2 = rng.integers(0, 4, size=(9, 10)).astype(np.uint8), rng.integers(0, 5, size=(9, 10)).astype(np.uint8)
    assert same_bits(R.join_segmentations(small1, small2, int64=True), R.join_segmentations(small1, small2))
    big1, big2 = rng.integers(0, 20, size=(30, 40)).astype(np.uint8), rng.integers(0, 20, size=(30, 40)).astype(np.uint8)
    joined = R.join_segmentations(big1, big2, int64=True)
    pairs = set(zip(big1.ravel().tolist(), big2.ravel().tolist()))
    assert len(np.unique(joined)) == len(pairs) and len(set(zip(big1.ravel().tolist(), big2.ravel().tolist(), joined.ravel().tolist()))) == len(pairs)
    assert len(np.unique(R.join_segmentations(big1, big2))) < len(pairs)         # 21 * 20 + 20 > 255: the reference's key wraps
