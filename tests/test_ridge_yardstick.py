"""The host transcription tests/helpers/ridge_ref.py has the properties the reference's filters/tests/test_ridges.py and the
docstring examples of feature/corner.py check, so it can serve as the yardstick of tests/test_gpu_ridges.py; and the
float32 LAPACK baseline against which the device solver's bound (8 eps ||H||_F) is set.  No GPU."""
import numpy as np
import pytest

from helpers import ridge_ref as rr


@pytest.mark.parametrize("shape", [(10, 10), (6, 7, 8)])
def test_null_and_constant_images_give_the_null_result(shape):
    for img in (np.zeros(shape), np.ones(shape)):
        kw = dict(sigmas=[1], mode="reflect")
        assert np.array_equal(rr.meijering(img, **kw), np.zeros(shape))
        assert np.array_equal(rr.sato(img, **kw), np.zeros(shape))
        assert np.array_equal(rr.frangi(img, **kw), np.zeros(shape))
        assert np.array_equal(rr.hessian(img, **kw), np.ones(shape))


def _tube(shape, bright):
    img = np.zeros(shape) if bright else np.ones(shape)
    mid = tuple(n // 2 for n in shape[:-1])
    img[mid] = 1.0 if bright else 0.0                 # a line along the last axis
    return img, mid


@pytest.mark.parametrize("shape", [(15, 15), (11, 11, 11)])
@pytest.mark.parametrize("name", ["meijering", "sato", "frangi"])
def test_bright_and_dark_tubes_respond_under_the_matching_black_ridges(shape, name):
    fn = getattr(rr, name)
    centre = tuple(n // 2 for n in shape)
    for bright in (True, False):
        img, _ = _tube(shape, bright)
        match = fn(img, sigmas=[1.5], black_ridges=not bright, mode="reflect")
        other = fn(img, sigmas=[1.5], black_ridges=bright, mode="reflect")
        assert match[centre] > 0
        assert match[centre] >= 0.5 * match.max()
        assert other[centre] == 0


def test_hessian_matrix_docstring_example():
    square = np.zeros((5, 5))
    square[2, 2] = 4
    Hrr, Hrc, Hcc = rr.hessian_matrix(square, sigma=0.1, order="rc")
    want = np.array([[0, 0, 0, 0, 0], [0, 1, 0, -1, 0], [0, 0, 0, 0, 0], [0, -1, 0, 1, 0], [0, 0, 0, 0, 0]], float)
    assert np.allclose(Hrc, want, atol=1e-12)


def test_hessian_matrix_eigvals_docstring_example():
    square = np.zeros((5, 5))
    square[2, 2] = 4
    eigs = rr.hessian_matrix_eigvals(rr.hessian_matrix(square, sigma=0.1, order="rc"))
    want = np.array([[0, 0, 2, 0, 0], [0, 1, 0, 1, 0], [2, 0, -2, 0, 2], [0, 1, 0, 1, 0], [0, 0, 2, 0, 0]], float)
    assert np.allclose(eigs[0], want, atol=1e-12)


def test_sato_peaks_on_the_tube_axis_in_3d():
    img, mid = _tube((13, 13, 13), True)
    out = rr.sato(img, sigmas=[2], black_ridges=False, mode="reflect")
    section = out[:, :, 6]
    assert np.unravel_index(section.argmax(), section.shape) == mid


def test_abs_ordering_keeps_the_decreasing_order_on_ties():
    eigs = np.array([[2.0], [1.0], [-2.0]])
    assert rr.sortbyabs(eigs)[:, 0].tolist() == [1.0, 2.0, -2.0]


@pytest.mark.parametrize("shape", [(24, 25, 26), (6, 7, 8, 9)])
def test_float32_lapack_is_within_one_eps_of_float64_on_the_generators_hessians(shape):
    """the baseline of the device bound: LAPACK's own float32 error on these matrices, in units of eps32 ||H||_F"""
    from scipy import ndimage as ndi
    g = ndi.gaussian_filter(rr.volume(shape, np.float32, 3), 1.5, mode="reflect")
    elems = [np.float32(1.5 ** 2) * e for e in rr.hessian_from_smoothed(g)]
    e32 = rr.hessian_matrix_eigvals(elems, np.float32).astype(np.float64)
    e64 = rr.hessian_matrix_eigvals(elems, np.float64)
    fro = np.sqrt((rr.symmetric_image(elems).astype(np.float64) ** 2).sum((-1, -2)))
    err = np.abs(e32 - e64).max(0)
    ratio = (err[fro > 0] / (np.finfo(np.float32).eps * fro[fro > 0])).max()
    print("float32 LAPACK error / (eps32 ||H||_F):", ratio)
    assert ratio <= 1.0
