"""cupyimg_amd.skimage.segmentation without a GPU: the module exists with the reference's `__all__`, its public signatures
are the reference's (recorded here as literals: argument names and the source text of the defaults), and the argument
errors that need no device are raised before any device work (this machine may have no device at all)."""
import ast
import inspect
import warnings

import numpy as np
import pytest

ALL = ["morphological_chan_vese", "morphological_geodesic_active_contour", "inverse_gaussian_gradient", "circle_level_set",
       "disk_level_set", "checkerboard_level_set"]

# cupyimg/skimage/segmentation/morphsnakes.py:133, 167, 204, 237, 269, 381 (and 55, 75 for the two operators)
SIGNATURES = {
    "sup_inf": [("u", None)],
    "inf_sup": [("u", None)],
    "circle_level_set": [("image_shape", None), ("center", "None"), ("radius", "None")],
    "disk_level_set": [("image_shape", None), ("center", "None"), ("radius", "None")],
    "checkerboard_level_set": [("image_shape", None), ("square_size", "5")],
    "inverse_gaussian_gradient": [("image", None), ("alpha", "100.0"), ("sigma", "5.0")],
    "morphological_chan_vese": [("image", None), ("iterations", None), ("init_level_set", "'checkerboard'"), ("smoothing", "1"),
                                ("lambda1", "1"), ("lambda2", "1"), ("iter_callback", "lambda x: None")],
    "morphological_geodesic_active_contour": [("gimage", None), ("iterations", None), ("init_level_set", "'circle'"), ("smoothing", "1"),
                                              ("threshold", "'auto'"), ("balloon", "0"), ("iter_callback", "lambda x: None")],
}


@pytest.fixture(scope="module")
def seg():
    from cupyimg_amd.skimage import segmentation
    return segmentation


def test_module_and_all(seg):
    import cupyimg_amd.skimage as sk
    assert sk.segmentation is seg
    assert list(seg.__all__) == ALL
    for name in ALL + ["sup_inf", "inf_sup", "last_snake_launches"]:
        assert callable(getattr(seg, name))
    assert "sup_inf" not in seg.__all__ and "inf_sup" not in seg.__all__


def test_signatures_are_the_reference_s(seg):
    tree = ast.parse(inspect.getsource(seg))
    found = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in SIGNATURES:
            a = node.args
            assert not (a.vararg or a.kwarg or a.kwonlyargs or a.posonlyargs), node.name
            defaults = [None] * (len(a.args) - len(a.defaults)) + [ast.unparse(d) for d in a.defaults]
            found[node.name] = [(arg.arg, d) for arg, d in zip(a.args, defaults)]
    assert found == SIGNATURES


def test_argument_errors_come_before_any_device_work(seg):
    img = np.zeros((6, 7))
    for fn in (seg.morphological_chan_vese, seg.morphological_geodesic_active_contour):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 4, 4, 4)), 1, np.zeros((4, 4, 4, 4)))           # rank
        with pytest.raises(ValueError):
            fn(np.zeros(5), 1, np.zeros(5))
        with pytest.raises(ValueError):
            fn(np.zeros((10, 10, 3)), 1, np.zeros((10, 9)))                  # rank of the level set
        with pytest.raises(ValueError):
            fn(img, 1, np.zeros((6, 8)))                                     # shape of the level set
        with pytest.raises(ValueError):
            fn(img, 1, "square")                                             # unknown name
        with pytest.raises(ValueError):
            fn(img, -1, "disk")
        with pytest.raises(ValueError):
            fn(img, 1, "disk", smoothing=-1)
        with pytest.raises(ValueError):
            fn(np.zeros((1, 7)), 1, "disk")                                  # numpy.gradient needs two elements
        with pytest.raises(TypeError):
            fn(np.zeros((6, 7), np.complex64), 1, "disk")
    for fn in (seg.sup_inf, seg.inf_sup):
        with pytest.raises(ValueError):
            fn(np.zeros(5, np.int8))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 2, 2, 2), np.int8))


def test_circle_names_warn_before_any_device_work(seg):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with pytest.raises(ValueError):
            seg.morphological_geodesic_active_contour(np.zeros((6, 7)), -1, "circle")     # warns, then refuses the count
    assert not seen                                                                         # the count is checked first
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with pytest.raises(ValueError):
            seg.morphological_geodesic_active_contour(np.zeros((1, 7)), 1)                 # the default start is "circle"
    assert any(issubclass(w.category, FutureWarning) and "circle_level_set is deprecated" in str(w.message) for w in seen)
