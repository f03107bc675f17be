"""Writes tests/golden/corner_kat.json: the literal inputs and the stated expectations of the reference's structure-tensor and
corner tests (cupyimg/skimage/feature/tests/test_corner.py), as data, each with its file:line.  Nothing here calls the library
or the reference; the expectations are the ones the reference's tests state.

The impulse cases use sigma = 0.1: the Gaussian is then a single tap of weight 1, so the stated integers are exact.

Left out: everything that needs peak_local_max or corner_peaks (test_corner.py:399-456 count peaks without naming a place,
479-603), skimage.data images, and the Hessian cases, which tests/test_gpu_ridges.py already holds.  The squared dot of
test_corner.py:459-476 names a place, [6, 6]; it is kept as a CANDIDATE "the response's global maximum lies there", which
tests/test_corners_yardstick.py admits only if the host transcription has a unique global maximum at that pixel.

    python tests/golden/make_corner_kat.py
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def impulse(ndim):
    image = np.zeros((5,) * ndim)
    image[(2,) * ndim] = 1
    return image


def main():
    kat = {"source": "cupyimg/skimage/feature/tests/test_corner.py", "structure_tensor": [], "raises": [], "finite": [], "maximum": []}
    s = kat["structure_tensor"]
    acc = [[0, 0, 0, 0, 0], [0, 1, 0, 1, 0], [0, 4, 0, 4, 0], [0, 1, 0, 1, 0], [0, 0, 0, 0, 0]]
    arc = [[0, 0, 0, 0, 0], [0, 1, 0, -1, 0], [0, 0, 0, 0, 0], [0, -1, 0, 1, 0], [0, 0, 0, 0, 0]]
    arr = [[0, 0, 0, 0, 0], [0, 1, 4, 1, 0], [0, 0, 0, 0, 0], [0, 1, 4, 1, 0], [0, 0, 0, 0, 0]]
    s.append(dict(name="impulse_rc", ref="test_corner.py:49-88", image=impulse(2).tolist(), sigma=0.1, order="rc",
                  expected=[dict(element=0, index=None, values=arr), dict(element=1, index=None, values=arc), dict(element=2, index=None, values=acc)]))
    s.append(dict(name="impulse_xy", ref="test_corner.py:144-154 (the xy elements are the rc elements reversed)", image=impulse(2).tolist(), sigma=0.1, order="xy",
                  expected=[dict(element=0, index=None, values=acc), dict(element=1, index=None, values=arc), dict(element=2, index=None, values=arr)]))
    s.append(dict(name="impulse_default_order", ref="test_corner.py:144-152 (the default warns and means xy)", image=impulse(2).tolist(), sigma=0.1, order=None,
                  warns="the default order of the structure",
                  expected=[dict(element=0, index=None, values=acc), dict(element=1, index=None, values=arc), dict(element=2, index=None, values=arr)]))
    plane = [[0, 0, 0, 0, 0], [0, 1, 4, 1, 0], [0, 4, 16, 4, 0], [0, 1, 4, 1, 0], [0, 0, 0, 0, 0]]
    rows = [[0, 0, 0, 0, 0], [0, 4, 16, 4, 0], [0, 0, 0, 0, 0], [0, 4, 16, 4, 0], [0, 0, 0, 0, 0]]
    s.append(dict(name="impulse_3d", ref="test_corner.py:91-131", image=impulse(3).tolist(), sigma=0.1, order=None, count=6,
                  expected=[dict(element=0, index=[None, 1, None], values=arr), dict(element=0, index=[1], values=plane),
                            dict(element=3, index=[2], values=rows)]))
    s.append(dict(name="impulse_3d_rc", ref="test_corner.py:134-141 (rc is the default in 3-D)", image=impulse(3).tolist(), sigma=0.1, order="rc", count=6,
                  expected=[dict(element=0, index=[None, 1, None], values=arr), dict(element=0, index=[1], values=plane),
                            dict(element=3, index=[2], values=rows)]))
    kat["raises"].append(dict(name="xy_in_3d", ref="test_corner.py:134-137", shape=[5, 5, 5], sigma=0.1, order="xy", expect="ValueError"))
    kat["finite"].append(dict(name="blank_image", ref="test_corner.py:606-627", shape=[20, 20],
                              detectors=["corner_harris", "corner_shi_tomasi", "corner_kitchen_rosenfeld", "corner_foerstner"]))
    kat["maximum"].append(dict(name="squared_dot", ref="test_corner.py:459-476", shape=[50, 50], ones=[[4, 8], [4, 8]], at=[6, 6],
                               detectors=["corner_harris", "corner_shi_tomasi"]))
    with open(os.path.join(HERE, "corner_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
