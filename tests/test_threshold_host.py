"""What thresholding decides without a device: argument checking, the NotImplementedErrors, the multi-Otsu refusal above 2^34
tuples before anything touches the device, window validation, the `hist=` forms and the return types, and the ordering
operators' presence on core.ndarray."""
import math

import numpy as np
import pytest
from scipy import ndimage as sndi

from cupyimg_amd import core
from cupyimg_amd.skimage import filters as F
from cupyimg_amd.skimage.filters import _thresholding as T
from helpers import threshold_ref as R
from test_threshold_yardstick import same_bits


@pytest.fixture()
def no_device(monkeypatch):
    """any path that would reach the device fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(T.S, "as_device", touched)
    monkeypatch.setattr(T.E, "_masked", touched)
    monkeypatch.setattr(T.core, "asarray", touched)
    monkeypatch.setattr(T.core, "empty", touched)
    monkeypatch.setattr(T.core, "zeros", touched)


def test_public_names():
    for name in T.__all__:
        assert name in F.__all__ and getattr(F, name) is getattr(T, name)
    assert F._mean_std is T._mean_std


def test_not_implemented(no_device):
    with pytest.raises(NotImplementedError):
        F.try_all_threshold(np.zeros((4, 4)))
    with pytest.raises(NotImplementedError):
        F.threshold_local(np.zeros((4, 4)), 3, method="generic", param=np.mean)


def test_threshold_local_arguments(no_device):
    with pytest.raises(ValueError, match="must be odd"):
        F.threshold_local(np.zeros((4, 4)), 4)
    with pytest.raises(ValueError):
        F.threshold_local(np.zeros((4, 4, 4)), 3)
    with pytest.raises(ValueError, match="Invalid method"):
        F.threshold_local(np.zeros((4, 4)), 3, method="mode")


@pytest.mark.parametrize("fn", [F.threshold_niblack, F.threshold_sauvola, F._mean_std])
def test_window_validation(no_device, fn):
    image = np.zeros((6, 7), np.uint8)
    with pytest.raises(ValueError, match="must not be even"):
        fn(image, 4)
    with pytest.raises(ValueError, match="must not be even"):
        fn(image, (3, 6))
    with pytest.raises(ValueError):
        fn(image, (3, 3, 3))
    with pytest.raises(ValueError):
        fn(image, -3)
    with pytest.raises(ValueError):
        fn(np.zeros((2, 2), np.uint8), (46341, 46341))            # 2^31 samples or more


def test_multiotsu_refuses_above_2_34_tuples_before_the_device(no_device):
    assert T._multiotsu_tuples(256, 5) == math.comb(255, 4) == 172061505
    assert T._multiotsu_tuples(65536, 3) == 2147385345
    assert T._multiotsu_tuples(4096, 5) > 2 ** 34
    with pytest.raises(ValueError, match=r"2\*\*34"):
        F.threshold_multiotsu(np.zeros((4, 4), np.float32), classes=5, nbins=4096)
    with pytest.raises(ValueError, match=r"2\*\*34"):
        F.threshold_multiotsu(np.zeros((4, 4)), classes=3, nbins=200000)
    for classes in (1, 6):
        with pytest.raises(ValueError, match="2 to 5 classes"):
            F.threshold_multiotsu(np.zeros((4, 4), np.uint8), classes=classes)


def test_histogram_needs_image_or_hist(no_device):
    for fn in (F.threshold_otsu, F.threshold_yen, F.threshold_isodata, F.threshold_minimum):
        with pytest.raises(Exception, match="Either image or hist"):
            fn()


HISTS = [np.array([5, 1, 0, 2, 6, 3, 0, 4]), np.random.default_rng(1).integers(0, 900, size=200),
         np.concatenate([np.arange(40), np.arange(40)[::-1], np.arange(60)])]


@pytest.mark.parametrize("counts", HISTS, ids=["8bins", "200bins", "140bins"])
def test_hist_forms_and_return_types(no_device, counts):
    int_centers = np.arange(counts.size) + 10
    float_centers = np.linspace(-1.0, 1.0, counts.size).astype(np.float32)
    for fn, ref in ((F.threshold_otsu, R.otsu), (F.threshold_yen, R.yen), (F.threshold_isodata, R.isodata)):
        got = fn(hist=counts)
        assert isinstance(got, np.integer) and same_bits(got, ref(hist=counts))
        for form in (tuple, list):
            got = fn(hist=form((counts, int_centers)))
            assert isinstance(got, np.integer) and got.dtype == int_centers.dtype and same_bits(got, ref(hist=(counts, int_centers)))
        got = fn(hist=(counts.astype(np.float64), float_centers))
        assert isinstance(got, np.float64) and same_bits(got, ref(hist=(counts, float_centers)))
    got = F.threshold_isodata(hist=(counts, float_centers), return_all=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and same_bits(got, R.isodata(hist=(counts, float_centers), return_all=True))
    got = F.threshold_isodata(hist=counts, return_all=True)
    assert isinstance(got, np.ndarray) and got.dtype.kind == "i" and same_bits(got, R.isodata(hist=counts, return_all=True))


def test_minimum_on_histograms(no_device):
    two_peaks = np.array([0, 2, 9, 30, 9, 3, 1, 1, 4, 12, 40, 11, 2, 0], dtype=np.int64)
    got = F.threshold_minimum(hist=two_peaks)
    assert isinstance(got, np.integer) and same_bits(got, R.minimum(hist=two_peaks))
    with pytest.raises(RuntimeError, match="two maxima"):
        F.threshold_minimum(hist=np.zeros(256))
    with pytest.raises(RuntimeError):
        F.threshold_minimum(hist=np.random.default_rng(5).integers(0, 100, size=300), max_iter=2)


def test_three_bin_smoothing_is_scipys_reflect_filter():
    h = np.random.default_rng(2).integers(0, 1000, size=57).astype(np.float64)
    for hist in (h, h[:1], h[:2]):
        np.testing.assert_allclose(T._smooth3(hist), sndi.uniform_filter1d(hist, 3), rtol=4e-16, atol=0)
        assert same_bits(T._smooth3(hist), R.smooth3(hist))


def test_multiotsu_tables():
    p = np.array([0.25, 0.0, 0.5, 0.25])
    cum_p, cum_s = T._multiotsu_tables(p)
    assert cum_p.tolist() == [0.0, 0.25, 0.25, 0.75, 1.0] and cum_s.tolist() == [0.0, 0.0, 0.0, 1.0, 1.75]
    want = R.multiotsu_tables(p)
    assert same_bits(cum_p, want[0]) and same_bits(cum_s, want[1])


def test_ordering_operators_exist_and_equality_is_untouched():
    for name in ("__gt__", "__ge__", "__lt__", "__le__"):
        assert name in vars(core.ndarray)
    assert "__eq__" not in vars(core.ndarray) and "__ne__" not in vars(core.ndarray)
    a = object.__new__(core.ndarray)
    a.shape, a.dtype = (3,), np.dtype(np.uint8)
    for other in ("text", None, [1, 2, 3], 1j):
        assert core._compare(a, other, 0) is NotImplemented
        with pytest.raises(TypeError):
            a > other
