"""skimage.restoration.richardson_lucy without a device: the export, the signature, every argument check (they run on shapes and
dtypes alone, before the library is loaded), the dtype table and the number of iterations queued."""
import inspect

import numpy as np
import pytest

from cupyimg_amd.skimage import restoration
from cupyimg_amd.skimage.restoration import _deconvolution as D
from helpers import rl_ref


def test_exported_with_a_docstring():
    assert "richardson_lucy" in restoration.__all__ and "denoise_tv_chambolle" in restoration.__all__
    assert restoration.richardson_lucy is D.richardson_lucy
    doc = D.richardson_lucy.__doc__
    assert doc and "filter_epsilon" in doc and "Deviations" in doc and "mirror(psf)" in doc


def test_signature_is_the_references():
    sig = inspect.signature(restoration.richardson_lucy)
    assert str(sig) == "(image, psf, iterations=50, clip=True, filter_epsilon=None)"
    assert [p.kind for p in sig.parameters.values()] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 5


@pytest.mark.parametrize("which", ["image", "psf"])
@pytest.mark.parametrize("ctype", [np.complex64, np.complex128])
def test_complex_input(which, ctype):
    image = np.ones((5, 5), ctype if which == "image" else np.float32)
    psf = np.ones((3, 3), ctype if which == "psf" else np.float32)
    with pytest.raises(TypeError, match="Complex type not supported"):
        restoration.richardson_lucy(image, psf)


@pytest.mark.parametrize("ishape, pshape", [((5, 5), (3,)), ((5, 5), (3, 3, 3)), ((7,), (3, 3)), ((4, 5, 6), (3, 3)), ((5, 5), ())])
def test_psf_of_another_rank(ishape, pshape):
    with pytest.raises(ValueError, match="number of dimensions"):
        restoration.richardson_lucy(np.ones(ishape, np.float32), np.ones(pshape, np.float32))


@pytest.mark.parametrize("pshape", [(0, 3), (3, 0), (0, 0)])
def test_psf_with_an_empty_axis(pshape):
    with pytest.raises(ValueError, match="empty axis"):
        restoration.richardson_lucy(np.ones((5, 5), np.float32), np.ones(pshape, np.float32))
    with pytest.raises(ValueError, match="empty axis"):          # also when the image is empty too
        restoration.richardson_lucy(np.ones((0, 5), np.float32), np.ones(pshape, np.float32))


def test_rank_0():
    with pytest.raises(ValueError, match="rank 0"):
        restoration.richardson_lucy(np.float32(1.0), np.float32(1.0))


def test_rank_above_the_library_limit():
    with pytest.raises(ValueError, match="rank 1 to 8"):
        restoration.richardson_lucy(np.ones((1,) * 9, np.float32), np.ones((1,) * 9, np.float32))


DTYPE_TABLE = [("float16", "float32"), ("bool", "float32"), ("uint8", "float32"), ("int8", "float32"), ("uint16", "float32"),
               ("int16", "float32"), ("float32", "float32"), ("uint32", "float64"), ("int32", "float64"), ("uint64", "float64"),
               ("int64", "float64"), ("float64", "float64")]


@pytest.mark.parametrize("dtype, want", DTYPE_TABLE)
def test_dtype_table(dtype, want):
    T, _ = D._plan((5, 6), np.dtype(dtype), (3, 3), np.dtype(np.float64), 50)
    assert T == np.dtype(want)
    assert T == np.promote_types(np.dtype(dtype), np.float32)
    assert rl_ref.float_type(dtype) == T
    assert rl_ref.richardson_lucy(np.ones((3, 4), dtype), np.ones((2, 2), np.float64), iterations=1).dtype == T


@pytest.mark.parametrize("iterations, queued", [(0, 0), (-3, 0), (1, 1), (50, 50)])
def test_iterations_queued(iterations, queued):
    assert D._plan((5, 6), np.dtype(np.float32), (3, 3), np.dtype(np.float32), iterations)[1] == queued


@pytest.mark.parametrize("iterations", [0, -1])
def test_iterations_0_in_the_transcription(iterations):
    rng = np.random.default_rng(0)
    got = rl_ref.richardson_lucy(rng.random((4, 5)).astype(np.float32), rng.random((3, 3)), iterations=iterations)
    assert got.dtype == np.float32 and np.array_equal(got, np.full((4, 5), 0.5, np.float32))
