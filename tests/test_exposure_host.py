"""skimage.exposure: everything equalize_adapthist refuses is refused before the device is touched, so these run without a
GPU (a device call would raise RuntimeError here, not the error asked for); the module is part of the skimage package."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def exposure():
    from cupyimg_amd.skimage import exposure
    return exposure


def test_module_is_exported(exposure):
    import cupyimg_amd.skimage as sk
    assert sk.exposure is exposure
    for name in ("rescale_intensity", "histogram", "cumulative_distribution", "equalize_hist", "equalize_adapthist"):
        assert callable(getattr(exposure, name)) and name in exposure.__all__


@pytest.mark.parametrize("channels", [3, 4])
def test_rgb_shaped_arrays_are_refused(exposure, channels):
    with pytest.raises(NotImplementedError, match="colour"):
        exposure.equalize_adapthist(np.zeros((16, 16, channels), np.uint8), kernel_size=4)


def test_default_kernel_on_a_short_axis_is_refused(exposure):
    with pytest.raises(ValueError, match="kernel_size"):
        exposure.equalize_adapthist(np.zeros((7, 64), np.uint8))


@pytest.mark.parametrize("kernel", [0, (4, 0), -2, (0.5, 4)])
def test_kernel_below_one_is_refused(exposure, kernel):
    with pytest.raises(ValueError, match="kernel_size"):
        exposure.equalize_adapthist(np.zeros((16, 16), np.uint8), kernel_size=kernel)


@pytest.mark.parametrize("kernel", [(4,), (4, 4, 4), []])
def test_kernel_of_the_wrong_length_is_refused(exposure, kernel):
    with pytest.raises(ValueError, match="kernel_size"):
        exposure.equalize_adapthist(np.zeros((16, 16), np.uint16), kernel_size=kernel)


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "int64"])
def test_signed_integer_images_are_refused(exposure, dtype):
    with pytest.raises(NotImplementedError, match="signed"):
        exposure.equalize_adapthist(np.zeros((16, 16), dtype), kernel_size=4)


@pytest.mark.parametrize("nbins", [16385, 1 << 20])
def test_too_many_bins_are_refused(exposure, nbins):
    with pytest.raises(ValueError, match="nbins"):
        exposure.equalize_adapthist(np.zeros((16, 16), np.uint8), kernel_size=4, nbins=nbins)


@pytest.mark.parametrize("nbins", [0, -3, 2.5])
def test_nbins_must_be_a_positive_integer(exposure, nbins):
    with pytest.raises(ValueError, match="nbins"):
        exposure.equalize_adapthist(np.zeros((16, 16), np.uint8), kernel_size=4, nbins=nbins)


@pytest.mark.parametrize("shape", [(), (2, 2, 2, 2, 2)])
def test_ranks_outside_one_to_four_are_refused(exposure, shape):
    with pytest.raises(NotImplementedError, match="rank"):
        exposure.equalize_adapthist(np.zeros(shape, np.uint8), kernel_size=1)


def test_clip_limit_in_voxels_follows_the_reference(exposure):
    f = exposure._clahe_arguments
    assert f((20, 33, 70), "uint16", (5, 8, 16), 0.01, 256) == ([5, 8, 16], 6, 256)
    assert f((64, 64), "uint8", None, 0.01, 256) == ([8, 8], 1, 256)
    assert f((64, 64), "float32", 8, 0, 16384) == ([8, 8], 64, 16384)
    assert f((64, 64), "float64", 8.0, 1, 1)[1] == 64
    assert f((64, 64), "float16", 8, 0.5, 1)[1] == 32


@pytest.mark.parametrize("out_range", ["flat", "uint9", np.complex64])
def test_rescale_raises_on_incorrect_out_range(exposure, out_range):
    """test_rescale_raises_on_incorrect_out_range of the reference (test_exposure.py:345), before the device is touched"""
    with pytest.raises(ValueError, match="out_range"):
        exposure.rescale_intensity(np.asarray([-128, 0, 127], dtype=np.int8), out_range=out_range)
