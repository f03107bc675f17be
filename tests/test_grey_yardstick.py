"""Guards the yardstick of the grey-morphology fuzz (tests/helpers/grey_ref.py) on the CPU: the plain NumPy reference equals
scipy.ndimage bit for bit over the seeded draw, the draw really covers what it claims (every function, dtype, rank, window
kind, structure kind, mode and output form, even extents, windows longer than the axis, missing centres, origins with a
structure, illegal origins), and a reference that is subtly wrong is caught by the same comparison.

No case of this draw needs to be excluded: what SciPy computes through an undefined C conversion is never drawn
(grey_ref.py), the skip count is asserted to stay under the 2 % cap, and is 0 at this seed."""
import warnings

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import grey_ref as gr



@pytest.fixture(scope="module")
def drawn():
    cases = gr.drawn()              # one fixed seed (gr.SEED), gr.CASES cases
    assert len(cases) == gr.CASES and 550 <= gr.CASES <= 650
    return cases


def _mismatches(cases, **mutations):
    """the cases where the reference (with `mutations`) and SciPy disagree"""
    bad = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, case in enumerate(cases):
            want = gr.reference(case, **mutations)
            ok, why = gr.judge(case, want, gr.call(sndi, case))
            if not ok:
                bad.append((i, case["desc"], why))
    return bad


def test_reference_equals_scipy_bit_for_bit(drawn):
    skipped = 0                     # cases where SciPy's result is undefined: none in this draw, by construction
    assert skipped <= 0.02 * len(drawn)
    bad = _mismatches(drawn)
    assert not bad, (len(bad), bad[:5])


def test_draw_covers_what_it_claims(drawn):
    for c in drawn:
        assert c["x"].shape == c["shape"] and c["x"].dtype == np.dtype(c["dtype"]) and c["x"].flags.c_contiguous
    assert {c["func"] for c in drawn} == set(gr.FUNCS)
    assert {c["dtype"] for c in drawn} == set(gr.IN_DTYPES)
    assert {c["dtype"] for c in drawn if gr.has_structure(c)} == set(gr.STRUCT_DTYPES)
    assert {len(c["shape"]) for c in drawn} == {1, 2, 3, 4, 5}
    assert {len(c["shape"]) for c in drawn if gr.has_structure(c)} == {1, 2, 3, 4, 5}
    assert {c["wkind"] for c in drawn} == set(gr.WINDOW_KINDS)
    assert {c["skind"] for c in drawn} == set(gr.STRUCT_KINDS) | {None}
    assert {c["kw"]["mode"] for c in drawn} == set(gr.MODES)
    assert {c["kw"]["mode"] for c in drawn if gr.has_structure(c)} == set(gr.MODES)
    assert {c["kw"]["cval"] for c in drawn} == set(gr.CVALS)
    assert all(c["kw"]["cval"] >= 0 for c in drawn if np.dtype(c["dtype"]).kind in "ub")
    assert {c["out_kind"] for c in drawn} == {"none", "dtype", "array"}
    assert {c["out_layout"] for c in drawn} == {None, "c", "strided", "input"}
    assert {gr.family(c) for c in drawn} == set(gr.FAMILIES)
    # another output dtype: every pair, and with a structure
    pairs = {(c["dtype"], c["out_dtype"]) for c in drawn if c["out_dtype"] != c["dtype"]}
    assert pairs == {(a, b) for a, bs in gr.WIDER.items() for b in bs}, sorted(pairs)
    assert any(c["out_dtype"] != c["dtype"] and gr.has_structure(c) for c in drawn)
    assert all(c["out_dtype"] == c["dtype"] or (not c["wide"] and c["func"] in gr.SIMPLE) for c in drawn)
    # the exclusions hold by construction
    assert not any(gr.has_structure(c) and c["dtype"] in ("bool", "uint64") for c in drawn)
    assert all(abs(int(v)) <= 2 ** 40 for c in drawn if np.dtype(c["dtype"]).kind in "iu" for v in (c["x"].min(), c["x"].max()))
    assert any(c["wide"] and np.dtype(c["dtype"]).kind in "iu" for c in drawn) and any(not c["wide"] for c in drawn)
    assert any(c["has_inf"] for c in drawn) and all(c["func"] in gr.SIMPLE for c in drawn if c["has_inf"])
    assert all(np.isfinite(c["x"]).all() for c in drawn if not c["has_inf"] and np.dtype(c["dtype"]).kind == "f")
    # windows
    assert any(not f & 1 for c in drawn for f in c["ext"])                                              # an even extent
    assert any(not f & 1 for c in drawn if gr.has_structure(c) and "dilation" in c["func"] for f in c["ext"])
    assert any(f > n for c in drawn for f, n in zip(c["ext"], c["shape"]))                              # longer than its axis
    assert any(1 in c["shape"] for c in drawn)
    fps = [c["kw"]["footprint"] for c in drawn if c["kw"].get("footprint") is not None]
    assert any(not fp[tuple(f // 2 for f in fp.shape)] for fp in fps)                                   # a missing centre
    assert all(fp.any() for fp in fps) and all(not c["kw"]["footprint"].all() for c in drawn if c["wkind"] == "holes")
    sts = [c["kw"]["structure"] for c in drawn if gr.has_structure(c)]
    assert any((s != np.floor(s)).any() for s in sts) and any((s < 0).any() for s in sts)
    assert any((s != s.astype(np.float32)).any() for s in sts)          # a value no float32 holds
    # origins
    assert any(gr.has_structure(c) and np.any(c["kw"]["origin"]) and not c["illegal"] for c in drawn)
    illegal = [c for c in drawn if c["illegal"]]
    assert 0.04 * len(drawn) <= len(illegal) <= 0.16 * len(drawn), len(illegal)
    assert all(isinstance(gr.reference(c), ValueError) for c in illegal)
    assert not any(isinstance(gr.reference(c), ValueError) for c in drawn if not c["illegal"])


@pytest.mark.parametrize("mutation", gr.MUTATIONS)
def test_a_subtly_wrong_reference_is_caught(drawn, mutation):
    """the comparison has teeth: each single deviation from SciPy's arithmetic fails on this draw"""
    assert _mismatches(drawn, **{mutation: True})
