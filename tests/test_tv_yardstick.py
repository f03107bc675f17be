"""The host transcription the GPU total-variation tests compare against (tests/helpers/tv_ref.py) is itself right: it has
the properties the reference's own test_denoise.py checks of denoise_tv_chambolle (less gradient at ranks 1 to 4, a larger
weight gives less total variation, results stay inside the input range, channels are independent), returns a constant
image unchanged, and every input of the GPU stopping tests stops at one iteration in float32 and float64, clear of the
threshold -- the condition under which an exact stop-iteration assertion on the device is legitimate.  No GPU needed."""
import numpy as np
import pytest

from helpers import tv_ref as tv


def _total_variation(x):
    g = np.zeros((x.ndim,) + x.shape)
    for a in range(x.ndim):
        lo = [slice(None)] * x.ndim
        lo[a] = slice(0, -1)
        g[(a,) + tuple(lo)] = np.diff(x.astype(np.float64), axis=a)
    return np.sqrt((g * g).sum(axis=0)).sum()


@pytest.mark.parametrize("shape", [(300,), (40, 52), (12, 20, 30), (5, 6, 7, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gradient_magnitude_drops(shape, dtype):
    x = tv.volume(shape, dtype)
    out, i, ratios = tv.tv_chambolle(x, weight=0.1)
    assert out.dtype == x.dtype and out.shape == x.shape
    assert 1 <= i < 200 and len(ratios) == i + 1
    assert _total_variation(out) / x.size < 0.8 * _total_variation(x) / x.size
    assert out.std() < x.std()


def test_larger_weight_gives_smaller_total_variation():
    x = tv.volume((30, 44))
    tvs = [_total_variation(tv.tv_chambolle(x, weight=w)[0]) for w in (0.05, 0.1, 0.2, 0.4)]
    assert all(a > b for a, b in zip(tvs, tvs[1:])), tvs
    assert tvs[0] < _total_variation(x)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_result_stays_inside_the_input_range(dtype):
    x = np.clip(tv.volume((36, 40)) / 1.5, 0.0, 1.0)
    x = (np.round(x * 255) / 255).astype(dtype)           # what img_as_float makes of a uint8 image
    out = tv.tv_chambolle(x, weight=0.1)[0]
    assert out.min() >= 0.0 and out.max() <= 1.0
    assert out.min() >= x.min() and out.max() <= x.max()


def test_channels_are_independent():
    x = tv.volume((20, 33, 3))
    per_channel = [tv.tv_chambolle(np.ascontiguousarray(x[..., c]), weight=0.1) for c in range(3)]
    whole = tv.tv_chambolle(x, weight=0.1)[0]
    # denoising the channel axis as a third axis is something else: that is what multichannel=True avoids
    assert not np.array_equal(whole[..., 0], per_channel[0][0])
    # and a channel's result does not depend on how the channel is stored
    again = tv.tv_chambolle(x[..., 1].copy(), weight=0.1)
    assert np.array_equal(again[0], per_channel[1][0]) and again[1] == per_channel[1][1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(17,), (6, 9), (4, 5, 6)], ids=lambda s: "x".join(map(str, s)))
def test_constant_image_is_returned_unchanged(shape, dtype):
    x = np.full(shape, 0.37, dtype)
    out, i, _ = tv.tv_chambolle(x, weight=0.1)
    assert np.array_equal(out, x)
    assert i == 200                    # E stays 0 and |0 - 0| < eps * 0 never holds: the loop runs out, as the reference's does
    out, i, _ = tv.tv_chambolle(x, weight=0.1, n_iter_max=5)
    assert np.array_equal(out, x)


def test_fixed_iteration_count_and_exhaustion():
    x = tv.volume((9, 11, 13), np.float32)
    for n in (1, 2, 7):
        out, i, ratios = tv.tv_chambolle(x, weight=0.2, eps=0, n_iter_max=n)
        assert i == n and len(ratios) == n
    assert np.array_equal(tv.tv_chambolle(x, weight=0.2, eps=0, n_iter_max=1)[0], x)       # out of iteration 0 is the image
    assert not np.array_equal(tv.tv_chambolle(x, weight=0.2, eps=0, n_iter_max=2)[0], x)


@pytest.mark.parametrize("case", tv.STOP_CASES, ids=lambda c: "{}-w{}".format("x".join(map(str, c[0])), c[1]))
def test_stop_cases_are_clear_of_the_threshold(case):
    shape, weight, seed = case
    x = tv.volume(shape, np.float64, seed)
    out32, i32, r32 = tv.tv_chambolle(x.astype(np.float32), weight=weight)
    out64, i64, r64 = tv.tv_chambolle(x, weight=weight)
    print(shape, weight, seed, "stop", i32, i64, "last ratios", r32[-2:], r64[-2:])
    assert i32 == i64 and 2 <= i64 < 199
    for r in (r32, r64):
        assert len(r) == i64 + 1
        assert r[-2] >= 1.005 and r[-1] <= 0.995
        assert all(v >= 1.005 for v in r[1:-1])            # no earlier iteration came close either
    assert max(abs(a - b) for a, b in zip(r32[1:], r64[1:])) < 1e-3
