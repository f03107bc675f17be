"""skimage.feature.match_template without a device: the signature, the export, and every argument check -- they run on shapes
and dtypes alone, before anything is uploaded or queued, so they raise on a machine without a GPU.  The transcription of
tests/helpers/template_ref.py is held to the known answers of tests/golden/template_kat.json here too."""
import inspect
import json
import os

import numpy as np
import pytest

from cupyimg_amd.skimage import feature
from cupyimg_amd.skimage.feature import match_template
from helpers import template_ref

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "template_kat.json")))


def test_signature_is_the_references():
    sig = inspect.signature(match_template)
    assert str(sig) == "(image, template, pad_input=False, mode='constant', constant_values=0)"
    assert [p.kind for p in sig.parameters.values()] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 5


def test_exported_with_a_docstring():
    assert "match_template" in feature.__all__
    assert feature.match_template is match_template
    doc = match_template.__doc__
    assert doc and "pad_input" in doc and "float64" in doc and "Deviations" in doc


@pytest.mark.parametrize("shape", [(7,), (2, 3, 4, 5), ()])
def test_rank_other_than_2_or_3(shape):
    with pytest.raises(ValueError, match="must be a 2-or-3-dimensional array"):
        match_template(np.ones(shape), np.ones((1,) * len(shape)))


def test_empty_image_and_empty_template():
    with pytest.raises(ValueError, match="`image` cannot be an empty array"):
        match_template(np.ones((0, 5)), np.ones((1, 1)))
    with pytest.raises(ValueError, match="empty"):
        match_template(np.ones((5, 5)), np.ones((0, 3)))
    with pytest.raises(ValueError, match="empty"):
        match_template(np.ones((5, 5, 5)), np.ones((2, 0, 2)))


def test_template_of_higher_rank():
    with pytest.raises(ValueError, match="Dimensionality of template must be less than or equal to the dimensionality of image."):
        match_template(np.ones((5, 5)), np.ones((3, 3, 2)))


@pytest.mark.parametrize("ishape, tshape", [((3, 3), (5, 5)), ((5, 5), (3, 6)), ((5, 5, 1), (3, 3, 2)), ((4, 9, 9), (5, 1, 1))])
def test_image_smaller_than_template(ishape, tshape):
    with pytest.raises(ValueError, match="Image must be larger than template."):
        match_template(np.ones(ishape), np.ones(tshape))


def test_template_of_lower_rank_raises_up_front():
    with pytest.raises(ValueError, match="number of dimensions"):
        match_template(np.ones((5, 5, 3)), np.ones((3, 3)))


@pytest.mark.parametrize("which", ["image", "template"])
def test_complex_input(which):
    image = np.ones((5, 5), np.complex64 if which == "image" else np.float32)
    template = np.ones((3, 3), np.complex128 if which == "template" else np.float32)
    with pytest.raises(TypeError):
        match_template(image, template)


@pytest.mark.parametrize("mode", ["linear_ramp", "maximum", "mean", "median", "minimum", "empty"])
def test_other_numpy_pad_modes(mode):
    with pytest.raises(NotImplementedError, match=mode):
        match_template(np.ones((5, 5)), np.ones((3, 3)), pad_input=True, mode=mode)


@pytest.mark.parametrize("mode", ["nearest", "mirror", "grid-wrap", "", None, 3])
def test_unknown_modes(mode):
    with pytest.raises(ValueError):
        match_template(np.ones((5, 5)), np.ones((3, 3)), pad_input=True, mode=mode)


@pytest.mark.parametrize("cv", [(1, 2), [0.5], ((1, 2), (3, 4)), np.array([1.0, 2.0])])
def test_constant_values_sequences(cv):
    with pytest.raises(NotImplementedError):
        match_template(np.ones((5, 5)), np.ones((3, 3)), pad_input=True, constant_values=cv)


@pytest.mark.parametrize("cv", [1j, "0", None])
def test_constant_values_must_be_real(cv):
    with pytest.raises(TypeError):
        match_template(np.ones((5, 5)), np.ones((3, 3)), pad_input=True, constant_values=cv)


def test_size_guard():
    """2**31 voxels: refused on the shape alone (a broadcast view holds one byte)"""
    image = np.broadcast_to(np.uint8(1), (2 ** 11, 2 ** 10, 2 ** 10))
    with pytest.raises(ValueError, match=r"2\*\*31"):
        match_template(image, np.ones((2, 2, 2)))


def test_checks_come_before_the_device(monkeypatch):
    """no check may load the library: with the loader broken, every error above is still the one raised"""
    from cupyimg_amd import _lib

    def broken():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", broken)
    with pytest.raises(ValueError, match="Image must be larger"):
        match_template(np.ones((3, 3)), np.ones((5, 5)))
    with pytest.raises(NotImplementedError):
        match_template(np.ones((5, 5)), np.ones((3, 3)), mode="mean")
    with pytest.raises(NotImplementedError):
        match_template(np.ones((5, 5)), np.ones((3, 3)), constant_values=(0, 1))
    with pytest.raises(TypeError):
        match_template(np.ones((5, 5), np.complex64), np.ones((3, 3)))


# ------------------------------------------------------------------ the transcription against the known answers
def test_transcription_docstring_example():
    k = KAT["docstring"]
    image, template = np.array(k["image"]), np.array(k["template"])
    assert np.array_equal(np.round(template_ref.match_template(image, template), k["decimals"]), np.array(k["expected"]))
    assert np.array_equal(np.round(template_ref.match_template(image, template, pad_input=True), k["decimals"]), np.array(k["expected_pad_input"]))


def test_transcription_reflect_padding_and_volume():
    k = KAT["padding_reflect"]
    r = template_ref.match_template(np.array(k["image"]), np.array(k["template"]), pad_input=True, mode=k["mode"])
    assert list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax"]
    k = KAT["volume"]
    template = np.array(k["template"])
    image = np.zeros(k["image_shape"])
    z, y, x = k["planted_at"]
    image[z:z + 3, y:y + 3, x:x + 3] = template
    r = template_ref.match_template(image, template)
    assert list(r.shape) == k["shape"] and list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax"]
    r = template_ref.match_template(image, template, pad_input=True)
    assert list(r.shape) == k["shape_pad_input"] and list(np.unravel_index(int(r.argmax()), r.shape)) == k["argmax_pad_input"]


def test_transcription_longdouble_agrees_and_bound_is_small():
    rng = np.random.default_rng(5)
    image, template = rng.random((13, 17)) + 0.25, rng.random((3, 5))
    r = template_ref.match_template(image, template, pad_input=True, mode="symmetric")
    rl, sums = template_ref.match_template_longdouble(image, template, pad_input=True, mode="symmetric")
    bound = template_ref.error_bound(rl, sums)
    assert template_ref.conditioning(sums).min() > 1e-3
    assert bound.max() < 1e-12 and np.all(np.abs(r - rl) <= bound)
