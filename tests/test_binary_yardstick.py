"""Guards the yardstick of the binary-morphology fuzz (tests/helpers/binary_ref.py) on the CPU: the plain NumPy reference
equals scipy.ndimage bit for bit over the seeded draw, the draw really covers what it claims (real masks, every dtype, rank,
function and edge value, until-stable cases that end), and a reference that is subtly wrong is caught by the same
comparison.

SciPy is always called with brute_force=True (its coordinate-list path corrupts the heap); float16 arrays reach it as
float32 (exact; SciPy has no float16).  No case of this draw needs to be excluded: the skip count is asserted to stay
under the 2 % cap, and is 0 at this seed."""
import warnings
from collections import Counter

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import binary_ref as br

SEED, CASES = 11, 600


@pytest.fixture(scope="module")
def drawn():
    rng = np.random.default_rng(SEED)
    return [br.draw_case(rng) for _ in range(CASES)]


def _mismatches(cases, **dbg):
    """indices of the cases where the reference (with `dbg` mutations) and SciPy disagree"""
    bad = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, case in enumerate(cases):
            want = br.reference(case, **dbg)
            ret, out, base = br.call(sndi, case, f16_as_f32=True)
            ok, why = br.judge(case, want, ret, out, base, f16_as_f32=True)
            if not ok:
                bad.append((i, case["desc"], why))
    return bad


def test_reference_equals_scipy_bit_for_bit(drawn):
    skipped = 0                     # cases where SciPy is documented as wrong: none in this draw
    assert skipped <= 0.02 * len(drawn)
    bad = _mismatches(drawn)
    assert not bad, bad[:5]


def test_draw_covers_what_it_claims(drawn):
    share = []
    for case in drawn:
        x = br.view_of(case["x_base"], case["x_layout"])
        assert x.shape == case["shape"] and x.dtype == np.dtype(case["dtype"])
        share.append(float(br.truth(x).mean()) if x.size else 0.0)
    share = np.array(share)
    assert ((share >= 0.1) & (share <= 0.9)).mean() >= 0.85, ((share >= 0.1) & (share <= 0.9)).mean()
    assert {c["dtype"] for c in drawn} == set(br.IN_DTYPES)
    assert {len(c["shape"]) for c in drawn} == {1, 2, 3, 4, 5}
    assert {c["func"] for c in drawn} == set(br.FUNCS)
    assert {e for c in drawn for e in c["edges"]} == set(br.EDGE_VALUES)
    assert {c["density_kind"] for c in drawn} == {"mixed", "all-false", "all-true", "single"}
    assert {c["out_kind"] for c in drawn} == {"none", "dtype", "array"}
    assert {c["out_layout"] for c in drawn} == {None, "c", "strided", "input"}
    assert {c["x_layout"] for c in drawn} == {"c", "every-other", "transposed"}
    assert {c["out_dtype"] for c in drawn if c["out_kind"] == "array"} >= set(br.OUT_DTYPES)
    its = Counter(c["kw"].get("iterations") for c in drawn if "iterations" in c["kw"])
    assert set(br.ITERATIONS) <= set(its) and any(k < 1 for k in its)
    masks = {None if c["kw"].get("mask") is None else c["kw"]["mask"].dtype.name for c in drawn}
    assert masks == {None, "bool", "uint8", "int32", "float32"}
    assert any(np.isnan(c["kw"]["mask"]).any() for c in drawn if c["kw"].get("mask") is not None and c["kw"]["mask"].dtype.kind == "f")
    assert any((c["kw"]["mask"] == 256).any() for c in drawn if c["kw"].get("mask") is not None and c["kw"]["mask"].dtype == np.int32)
    sts = [c["kw"].get("structure", c["kw"].get("structure1")) for c in drawn]
    assert any(s is None for s in sts)
    assert any(s is not None and any(not n & 1 for n in s.shape) for s in sts)                       # even extents
    assert any(s is not None and not s[tuple(n // 2 for n in s.shape)] for s in sts)                 # without the centre
    assert any(s is not None and s.shape[-1] in (7, 9) for s in sts)
    assert any(s is not None and any(a > b for a, b in zip(s.shape, c["shape"])) for s, c in zip(sts, drawn))
    names = {c["desc"][5] for c in drawn}
    assert {"cube2", "octa2", "cube3", "octa3", "cube2-1", "octa2-1"} <= names, sorted(names)
    hm = [c for c in drawn if c["func"] == "hit_or_miss"]
    assert any(c["kw"]["structure2"] is not None and c["kw"]["origin2"] is not None and c["kw"]["origin1"] != c["kw"]["origin2"] for c in hm)


def test_until_stable_draws_are_monotone_and_end(drawn):
    n = 0
    for case in drawn:
        if not case["until_stable"]:
            continue
        n += 1
        nd = len(case["shape"])
        for offs in br.monotone_offsets(case):
            assert (0,) * nd in offs, case["desc"]
        count = []
        br.reference(case, count=count)
        assert count and max(count) <= sum(case["shape"]), (case["desc"], count)
    assert n >= 100


def test_a_subtly_wrong_reference_is_caught(drawn):
    """the comparison has teeth: one tap offset negated, or truth taken after narrowing to a byte, fails on this draw"""
    assert _mismatches(drawn, negate=0)
    assert _mismatches(drawn, truth_of=lambda x: np.asarray(x).astype(np.uint8) != 0)


def test_iterate_structure_equals_scipy():
    rng = np.random.default_rng(3)
    for nd in (1, 2, 3):
        for _ in range(6):
            st = rng.random([int(rng.integers(1, 5)) for _ in range(nd)]) > 0.4
            for it in (1, 2, 3):
                assert np.array_equal(br.iterate_structure(st, it), sndi.iterate_structure(st, it))
            a, o = br.iterate_structure(st, 3, origin=[0] * nd)
            b, p = sndi.iterate_structure(st, 3, origin=[0] * nd)
            assert np.array_equal(a, b) and list(o) == list(p)
