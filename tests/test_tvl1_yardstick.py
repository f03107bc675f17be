"""The host transcription of TV-L1 optical flow (tests/helpers/tvl1_ref.py) is a legitimate yardstick for the device tests:
identical images give a flow of exact zeros, skimage's own accuracy criteria hold on its sinusoidal case, and every case
whose stopping decisions tests/test_gpu_tvl1.py compares is clear of the threshold (the device takes the stopping sum in
double in a fixed order, the transcription in the image dtype, so a decision may differ only within summation error of it)."""
import functools

import numpy as np
import pytest

from helpers import tvl1_ref as R


@pytest.mark.parametrize("shape", [(40, 44), (24, 20, 28)], ids=["2d", "3d"])
def test_identical_images_give_exact_zeros(shape):
    x = np.random.RandomState(0).normal(size=shape)
    for dtype in (np.float32, np.float64):
        flow = R.optical_flow_tvl1(x, x, dtype=dtype)
        assert flow.shape == (len(shape),) + shape and flow.dtype == dtype
        assert np.all(flow == 0)


@functools.lru_cache(maxsize=None)
def _sin_flows():
    ref, mov, truth = R.sin_case()
    return truth, {dt: R.optical_flow_tvl1(ref, mov, attachment=5, dtype=dt) for dt in (np.float32, np.float64)}


def test_sinusoidal_case_meets_skimage_criterion():
    """test_tvl1.py test_2d_motion: the mean absolute error is below half a pixel (measured here: 0.351 in both dtypes)"""
    truth, flows = _sin_flows()
    for dt, flow in flows.items():
        err = np.abs(flow - truth).mean()
        print(np.dtype(dt).name, err)
        assert err < 0.5


def test_float32_and_float64_flows_agree():
    """test_tvl1.py test_optical_flow_dtype: below 1e-3 in the mean (measured here: 6.4e-5 on this white-noise input)"""
    _, flows = _sin_flows()
    diff = np.abs(flows[np.float64] - flows[np.float32]).mean()
    print(diff)
    assert diff < 1e-3


@pytest.mark.parametrize("case", [c[0] for c in R.STOP_CASES])
def test_stop_cases_are_clear_of_the_threshold(case):
    """a condition on the inputs: sum / (tol * size) outside [0.5, 2] at every level and warp, in both dtypes"""
    warps = {}
    for dtype in (np.float32, np.float64):
        ref, mov, kw = R.stop_case(case, dtype)
        rec = []
        R.optical_flow_tvl1(ref, mov, dtype=dtype, record=rec, **kw)
        print(case, np.dtype(dtype).name, rec)
        for level in rec:
            for ratio in level["ratios"]:
                assert ratio < 0.5 or ratio > 2.0, (case, level)
        warps[dtype] = [(level["shape"], level["warps"]) for level in rec]
    assert warps[np.float32] == warps[np.float64]


def test_cases_cover_a_middle_stop_and_running_out():
    num_warp = 5
    stops = {}
    for case, *_ in R.STOP_CASES:
        ref, mov, kw = R.stop_case(case, np.float32)
        rec = []
        R.optical_flow_tvl1(ref, mov, record=rec, **kw)
        stops[case] = [(level["warps"] - 1, level["ratios"][-1] < 1) for level in rec]
    flat = [s for v in stops.values() for s in v]
    assert any(stopped and 1 <= idx <= num_warp - 2 for idx, stopped in flat), stops
    assert any(not stopped and idx == num_warp - 1 for idx, stopped in flat), stops
    assert len(stops["two_levels_2d"]) == 2 and len(stops["two_levels_3d"]) == 2


def test_both_data_term_branches_and_zero_gradient_voxels_occur():
    """what the stage tests of tests/test_gpu_tvl1.py rely on"""
    for shape in [(12, 20, 70), (3, 3, 3), (70, 96), (5, 6, 7, 8)]:
        for dtype in (np.float32, np.float64):
            warped, ref, flow, proj = R.stage_inputs(shape, dtype)
            grad, NI, rho_0 = R.prepare(warped, ref, flow)
            raw = sum(g * g for g in grad)
            assert (raw == 0).any() and np.all(NI[raw == 0] == 1)
            rho = rho_0 + sum(g * f for g, f in zip(grad, flow))
            near = np.abs(rho) <= dtype(15 * 0.3) * NI
            assert near.any() and (~near).any(), shape
