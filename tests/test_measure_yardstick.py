"""CPU check of the yardstick of the labelled reductions (tests/helpers/measure_ref.py, used by
`fuzz_vs_scipy.py --measure` and tests/test_gpu_measure_routes.py): SciPy's own results meet the host references and
their bounds on every value generator, and deliberately wrong results -- the mistakes a reduction kernel makes -- break
them."""
import warnings

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import measure_ref as mr


def _scipy_judged(case):
    c = dict(case)
    if case["func"] in ("sum_labels", "mean", "variance", "standard_deviation", "center_of_mass") and \
            (case["labels"] is None or mr.index_form(case["index"]) != "seq"):
        c["x"] = case["x"].astype(np.float64)       # with no index SciPy sums in the input dtype (input.sum())
    try:
        want = mr.call(sndi, c)
    except Exception as e:                          # judged on the device side against the same exception
        return None, e
    return want, None


def test_references_and_bounds_agree_with_scipy():
    rng = np.random.default_rng(2024)
    seen, worst = set(), {}
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        while n < 600:
            case = mr.draw_reduction(rng)
            if not mr.scipy_exact(case):
                continue
            want, exc = _scipy_judged(case)
            if exc is not None:
                continue
            seq = case["labels"] is not None and mr.index_form(case["index"]) == "seq"
            if seq and "position" in case["func"] or seq and case["func"] == "extrema":
                continue                            # SciPy picks among tied extremes by an unstable argsort
            ok, r, why = mr.judge(case, want, check_struct=False)
            assert ok, (case["func"], case["x"].dtype, case["gen"], case["index_kind"], why)
            seen.add(case["gen"])
            worst[case["func"]] = max(worst.get(case["func"], 0.0), r)
            n += 1
    assert seen == {"mr", "ct", "1e4", "extremes", "small"}
    assert set(worst) >= set(mr.FUNCS) - {"minimum_position", "maximum_position", "extrema"}


def _case(func, x, labels=None, index=None, **kw):
    return dict(func=func, x=np.asarray(x), labels=labels, index=index,
                index_kind="none" if index is None else "list", kw=kw, gen="test")


def test_negative_zero_below_positive_zero_is_caught():
    c = _case("minimum_position", np.array([0.0, -0.0, 1.0]))
    assert mr.judge(c, (0,))[0]
    assert not mr.judge(c, (1,))[0]                 # -0.0 ordered strictly below +0.0
    c = _case("maximum_position", np.array([-0.0, 0.0, -1.0]))
    assert not mr.judge(c, (1,))[0]


def _wave_data(real):
    rng = np.random.default_rng(7)
    n = 64 * 40 + 9
    lab = (np.arange(n) // 64) % 5 + 1               # runs of exactly one wave
    x = rng.integers(0, 4096, n).astype(np.float64)
    if real:
        x = x + rng.standard_normal(n) * 0.25
    return x, lab, list(range(1, 6))


@pytest.mark.parametrize("real", [False, True])
def test_dropped_run_voxel_is_caught(real):
    x, lab, idx = _wave_data(real)
    ref = mr.Ref(x, lab, idx)
    good = ref.sums()[0][ref.rows]
    c = _case("sum_labels", x, lab, idx)
    assert mr.judge(c, good)[0]
    bad = good.copy()
    bad[0] -= x[63]                                  # the last lane of the first run of label 1
    ok, r, _ = mr.judge(c, bad)
    assert not ok and r > 10
    bad = good.copy()
    bad[0] += x[0]                                   # the run head counted twice
    assert not mr.judge(c, bad)[0]


@pytest.mark.parametrize("real", [False, True])
def test_slot_off_by_one_is_caught(real):
    x, lab, idx = _wave_data(real)
    ref = mr.Ref(x, lab, idx)
    c = _case("sum_labels", x, lab, idx)
    good = ref.sums()[0][ref.rows]
    ok, r, _ = mr.judge(c, np.roll(good, 1))
    assert not ok and r > 10
    com = [tuple(r_) for r_ in ref.com()[0][ref.rows]]
    cc = _case("center_of_mass", x, lab, idx)
    assert mr.judge(cc, com)[0]
    assert not mr.judge(cc, com[1:] + com[:1])[0]


@pytest.mark.parametrize("real", [False, True])
def test_skipped_lds_flush_is_caught(real):
    """one workgroup (256 consecutive voxels) never adds its LDS partial of one slot"""
    x, lab, idx = _wave_data(real)
    ref = mr.Ref(x, lab, idx)
    c = _case("sum_labels", x, lab, idx)
    bad = ref.sums()[0][ref.rows].copy()
    wg = slice(256, 512)
    bad[1] -= x[wg][lab[wg] == 2].sum()
    ok, r, _ = mr.judge(c, bad)
    assert not ok and r > 10
    m = ref.mean()[0][ref.rows].copy()
    m[1] = bad[1] / ref.n[1]
    assert not mr.judge(_case("mean", x, lab, idx), m)[0]


def test_open_last_histogram_bin_is_caught():
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.0])
    c = _case("histogram", x, min=0.0, max=4.0, bins=4)
    good = np.histogram(x, np.linspace(0, 4, 5))[0]
    assert mr.judge(c, good, sndi.histogram(x, 0, 4, 4))[0]
    bad = good.copy()
    bad[-1] -= 2                                     # the closed last bin left open: v == max not counted
    assert not mr.judge(c, bad)[0]
