"""Writes tests/golden/template_kat.json: known answers for skimage.feature.match_template.

    python tests/golden/make_template_kat.py

`docstring`: the example of the reference's docstring (template.py:93-123), both `pad_input` settings, its two tables as
printed there (3 decimals).  The other entries are the expectations of those tests of the reference's
feature/tests/test_template.py that need no scikit-image data file: their inputs (stored, or the seed they are drawn from) and
the positions, shapes and extremes those tests assert.  Only data is written."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def diamond(radius):
    g = np.abs(np.arange(-radius, radius + 1))
    return (g[:, None] + g[None, :] <= radius).astype(np.float64)


def docstring():
    template = np.zeros((3, 3))
    template[1, 1] = 1
    image = np.zeros((6, 6))
    image[1, 1] = 1
    image[4, 4] = -1
    expected = [[1.0, -0.125, 0.0, 0.0],
                [-0.125, -0.125, 0.0, 0.0],
                [0.0, 0.0, 0.125, 0.125],
                [0.0, 0.0, 0.125, -1.0]]
    padded = [[-0.125, -0.125, -0.125, 0.0, 0.0, 0.0],
              [-0.125, 1.0, -0.125, 0.0, 0.0, 0.0],
              [-0.125, -0.125, -0.125, 0.0, 0.0, 0.0],
              [0.0, 0.0, 0.0, 0.125, 0.125, 0.125],
              [0.0, 0.0, 0.0, 0.125, -1.0, 0.125],
              [0.0, 0.0, 0.0, 0.125, 0.125, 0.125]]
    return dict(image=image.tolist(), template=template.tolist(), decimals=3, expected=expected, expected_pad_input=padded)


def normalization():
    n, size = 5, 20
    ipos, jpos, ineg, jneg = 2, 3, 12, 11
    image = np.full((size, size), 0.5)
    image[ipos:ipos + n, jpos:jpos + n] = 1
    image[ineg:ineg + n, jneg:jneg + n] = 0
    template = np.zeros((n + 2, n + 2))             # a white square with a black border
    template[1:1 + n, 1:1 + n] = 1
    # the extremes sit one sample before the squares, because of the template's border
    return dict(image=image.tolist(), template=template.tolist(), argmin=[ineg - 1, jneg - 1], argmax=[ipos - 1, jpos - 1], min=-1.0, max=1.0)


def pad_input():
    template = 0.5 * diamond(2)
    image = 0.5 * np.ones((9, 19))
    mid = slice(2, 7)
    image[mid, :3] -= template[:, -3:]              # half a minimum, centred on column 0
    image[mid, 4:9] += template                     # a full maximum, centred on column 6
    image[mid, -9:-4] -= template                   # a full minimum, centred on column 12
    image[mid, -3:] += template[:, :3]              # half a maximum, centred on column 18
    return dict(image=image.tolist(), template=template.tolist(), constant_values=float(image.mean()),
                lowest_two_columns=[12, 0], highest_two_columns=[18, 6])


def volume():
    np.random.seed(1)
    template = np.random.rand(3, 3, 3)
    image = np.zeros((12, 12, 12))
    image[3:6, 5:8, 4:7] = template
    return dict(seed=1, image_shape=[12, 12, 12], template_shape=[3, 3, 3], planted_at=[3, 5, 4], shape=[10, 10, 10], argmax=[3, 5, 4],
                shape_pad_input=[12, 12, 12], argmax_pad_input=[4, 6, 5], template=template.tolist())


def padding_reflect():
    template = diamond(2)
    image = np.zeros((10, 10))
    image[2:7, :3] = template[:, -3:]
    return dict(image=image.tolist(), template=template.tolist(), mode="reflect", argmax=[4, 0])


def planted():
    # image = 0.5 everywhere, 0.1 * (tri(size) + tri(size)[::-1]) at the two positions, plus 0.1 * uniform noise from the seed
    return dict(seed=1, shape=[400, 400], size=100, positions=[[50, 50], [200, 200]], min_distance=5)


def no_nans():
    # image = 0.5 + 1e-9 * normal(size) from the seed; template = ones with its upper half zero
    return dict(seed=1, shape=[20, 20], template_shape=[6, 6], zero_rows=3, scale=1e-9)


if __name__ == "__main__":
    kat = dict(docstring=docstring(), normalization=normalization(), pad_input=pad_input(), volume=volume(),
               padding_reflect=padding_reflect(), planted=planted(), no_nans=no_nans())
    with open(os.path.join(HERE, "template_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")
