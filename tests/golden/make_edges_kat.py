"""Writes tests/golden/edges_kat.json: the literal inputs and the stated expectations of the reference's edge and Canny tests
(cupyimg/skimage/filters/tests/test_edges.py, cupyimg/skimage/feature/tests/test_canny.py), as data, each with its file:line.
Nothing here calls the library or the reference; the expectations are the ones the reference's tests state.

Left out: the cases built on skimage.data (`camera`: test_canny.py:85-165 test_use_quantiles, the image of
test_invalid_use_quantiles and test_dtype; `binary_blobs`: test_edges.py:570-582), because scikit-image's data files are not
available here.  The three cubes of test_edges.py:519-558 are kept: the tests check them against random binary cubes
instead of the blobs volume.  The uniform-noise images of the reference come from the device's generator; the cases below
name a NumPy seed instead.

    python tests/golden/make_edges_kat.py
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


ROW, COL = np.indices((10, 10))


def step(axis):
    """11 x 11, 0 before the centre line along `axis` and 1 from it on"""
    image = np.zeros((11, 11))
    image[(slice(5, None), slice(None))[::1 if axis == 0 else -1]] = 1.0
    return image


def mask_line(axis):
    """an 11 x 11 ramp of slope 0.1 along `axis` with line 5 overwritten by 1 and masked out; a unit-spacing derivative of
    the ramp over two samples is 0.2 inside, and the masked line takes its two neighbours with it"""
    ramp = np.linspace(0.0, 1.0, 11)
    grad = np.repeat(ramp[:, None], 11, axis=1) if axis == 0 else np.repeat(ramp[None, :], 11, axis=0)
    mask = np.ones((11, 11))
    expected = np.zeros((11, 11))
    expected[1:10, 1:10] = 0.2
    line = (5, slice(None)) if axis == 0 else (slice(None), 5)
    near = (slice(4, 7), slice(1, 10)) if axis == 0 else (slice(1, 10), slice(4, 7))
    grad[line] = 1
    mask[line] = 0
    expected[near] = 0
    return grad, mask, expected


def main():
    kat = {"source": "cupyimg/skimage/filters/tests/test_edges.py and cupyimg/skimage/feature/tests/test_canny.py", "edges": [], "canny": []}
    e = kat["edges"]
    all2d = ["sobel", "scharr", "prewitt", "roberts", "farid"]
    hv = ["sobel_h", "sobel_v", "scharr_h", "scharr_v", "prewitt_h", "prewitt_v", "farid_h", "farid_v", "roberts_pos_diag", "roberts_neg_diag"]
    e.append(dict(name="zeros", ref="test_edges.py:13-16, 43-46, 77-80, 109-112, 371-376, 406-411, 440-445", funcs=all2d + hv,
                  image=np.zeros((10, 10)).tolist(), mask=np.ones((10, 10)).tolist(), expect="all_zero"))
    e.append(dict(name="zero_mask", ref="test_edges.py:49-54, 83-88, 115-120, 379-384, 414-419, 448-453", funcs=all2d + hv + ["laplace"],
                  image_seed=0, image_shape=[10, 10], mask=np.zeros((10, 10)).tolist(), expect="all_zero"))
    for axis, name in ((0, "horizontal"), (1, "vertical")):
        e.append(dict(name="step_" + name, ref="test_edges.py:57-74", funcs=["sobel", "scharr", "prewitt"], image=step(axis).tolist(), step_axis=axis,
                      expect="times_sqrt2_is_1_on_the_step_and_0_beyond_one_pixel", rtol=1e-7))
        same = ("sobel_h", "scharr_h", "prewitt_h") if axis == 0 else ("sobel_v", "scharr_v", "prewitt_v")
        e.append(dict(name="step_" + name + "_signed", ref="test_edges.py:91-98 and the scharr / prewitt twins", funcs=list(same), image=step(axis).tolist(), step_axis=axis,
                      expect="abs_is_1_on_the_step_and_0_beyond_one_pixel", rtol=1e-7, atol=1e-10))
        cross = ("sobel_h", "scharr_h", "prewitt_h", "farid_h") if axis == 1 else ("sobel_v", "scharr_v", "prewitt_v", "farid_v")
        e.append(dict(name="step_" + name + "_cross", ref="test_edges.py:101-106, 432-437, 466-471", funcs=list(cross),
                      image=(step(axis) * np.sqrt(2)).tolist(), expect="all_zero", atol=1e-10))
        e.append(dict(name="farid_step_" + name, ref="test_edges.py:387-403, 422-429, 456-463", funcs=["farid", "farid_h" if axis == 0 else "farid_v"],
                      image=step(axis).tolist(), step_axis=axis, expect="constant_on_the_step_and_0_beyond_two_pixels", atol=1e-10))
        grad, mask, expected = mask_line(axis)
        funcs = ("prewitt_h", "sobel_h", "scharr_h") if axis == 0 else ("prewitt_v", "sobel_v", "scharr_v")
        e.append(dict(name="mask_line_" + name, ref="test_edges.py:474-509", funcs=list(funcs), image=grad.tolist(), mask=mask.tolist(),
                      expected=expected.tolist(), expect="allclose", rtol=1e-7))
    # a lower-triangular image of ones: Roberts' cross responds on the diagonal and the one above it, except at the last
    # pixel, where 'reflect' supplies equal neighbours; the second case is the same picture turned by three quarter turns
    lower = (COL <= ROW).astype(float)
    band = (COL == ROW) | (COL == ROW + 1)
    band[9, 9] = False
    e.append(dict(name="roberts_diagonal1", ref="test_edges.py:19-28", funcs=["roberts"], image=lower.tolist(), expected=band.astype(int).tolist(),
                  expect="nonzero_pattern"))
    anti = (COL + ROW == 9) | (COL + ROW == 8)
    e.append(dict(name="roberts_diagonal2", ref="test_edges.py:31-40", funcs=["roberts"], image=(COL + ROW <= 9).astype(float).tolist(),
                  expected=anti.astype(int).tolist(), expect="nonzero_pattern"))
    image = np.zeros((9, 9))
    image[3:-3, 3:-3] = 1
    check = [[0.0] * 9, [0.0] * 9,
             [0.0, 0.0, 0.0, -1.0, -1.0, -1.0, 0.0, 0.0, 0.0],
             [0.0, 0.0, -1.0, 2.0, 1.0, 2.0, -1.0, 0.0, 0.0],
             [0.0, 0.0, -1.0, 1.0, 0.0, 1.0, -1.0, 0.0, 0.0],
             [0.0, 0.0, -1.0, 2.0, 1.0, 2.0, -1.0, 0.0, 0.0],
             [0.0, 0.0, 0.0, -1.0, -1.0, -1.0, 0.0, 0.0, 0.0], [0.0] * 9, [0.0] * 9]
    e.append(dict(name="laplace_square", ref="test_edges.py:339-358", funcs=["laplace"], image=image.tolist(), expected=check, expect="allclose", rtol=1e-7))
    cubes = {
        "MAX_SOBEL_0": [[[0, 0, 0]] * 3, [[0, 0, 0]] * 3, [[1, 1, 1]] * 3],
        "MAX_SOBEL_ND": [[[1, 0, 0], [1, 0, 0], [1, 0, 0]], [[1, 0, 0], [1, 1, 0], [1, 1, 0]], [[1, 1, 0], [1, 1, 0], [1, 1, 0]]],
        "MAX_SCHARR_ND": [[[0, 0, 0], [0, 0, 1], [0, 1, 1]], [[0, 0, 1], [0, 1, 1], [0, 1, 1]], [[0, 0, 1], [0, 1, 1], [1, 1, 1]]],
    }
    e.append(dict(name="max_cubes", ref="test_edges.py:512-582", cubes=cubes,
                  pairs=[["prewitt", "MAX_SOBEL_ND", None], ["sobel", "MAX_SOBEL_ND", None], ["scharr", "MAX_SCHARR_ND", None],
                         ["prewitt", "MAX_SOBEL_0", 0], ["sobel", "MAX_SOBEL_0", 0], ["scharr", "MAX_SOBEL_0", 0]],
                  expect="the_centre_response_of_the_cube_is_the_maximum_over_binary_volumes"))
    e.append(dict(name="range", ref="test_edges.py:585-604", funcs=all2d, image_seed=1, image_shape=[100, 100], expect="within_0_1"))

    c = kat["canny"]
    c.append(dict(name="zeros", ref="test_canny.py:13-18", image="zeros", shape=[20, 20], args=[4, 0, 0], mask="ones", expect="no_edges"))
    c.append(dict(name="zeros_mask", ref="test_canny.py:20-25", image="uniform", image_seed=2, shape=[20, 20], args=[4, 0, 0], mask="zeros",
                  expect="no_edges"))
    c.append(dict(name="mask_none", ref="test_canny.py:77-82", image="zeros", shape=[20, 20], args=[4, 0, 0], expect="equals_the_all_ones_mask"))
    c.append(dict(name="circle", ref="test_canny.py:27-50", image="ring", args=[4, 0, 0], mask="ones", band_iterations=3, count_above=1200,
                  count_below=1600, expect="edges_inside_the_band_and_counted"))
    c.append(dict(name="circle_with_noise", ref="test_canny.py:52-70", image="noisy_ring", image_seed=0, args=[4, 0.1, 0.2], mask="ones",
                  band_iterations=4, count_above=1200, count_below=1600, expect="edges_inside_the_band_and_counted"))
    c.append(dict(name="image_shape", ref="test_canny.py:72-75", shape=[20, 20, 20], args=[4, 0, 0], expect="ValueError"))
    c.append(dict(name="invalid_use_quantiles", ref="test_canny.py:107-155", shape=[11, 11],
                  thresholds=[[0.5, 3.6], [-5, 0.5], [99, 0.9], [0.5, -100], [50, 150]], expect="ValueError"))
    with open(os.path.join(HERE, "edges_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
