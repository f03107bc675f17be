#!/usr/bin/env python3
"""Writes tests/golden/morphsnakes_kat.json: the literal images and expected arrays of the reference's morphological-snakes
tests (data only -- inputs, arguments and the expectation the reference test states, each with the reference file:line it is
transcribed from).

    python tests/golden/make_morphsnakes_kat.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "cupyimg/skimage/segmentation/tests/test_morphsnakes.py:"

gac_11x11 = [
    "00000000000",
    "00000000000",
    "00000100000",
    "00011111000",
    "00011111000",
    "00111111100",
    "00011111000",
    "00011111000",
    "00000100000",
    "00000000000",
    "00000000000",
]
checkerboard_6x6 = ["000001", "000001", "000001", "000001", "000001", "111110"]
disk_6x6 = ["000000", "001110", "011111", "011111", "011111", "001110"]


def rows(text):
    return [[int(c) for c in line] for line in text]


cases = {
    # image = disk (11, 11), centre (5, 5), radius 3.5 as float64; gimage = inverse_gaussian_gradient(image, alpha, sigma)
    "gac_simple_shape": {"cite": REF + "86", "shape": [11, 11], "image_disk": {"center": [5, 5], "radius": 3.5}, "alpha": 10.0, "sigma": 1.0,
                         "level_set_disk": {"center": [5, 5], "radius": 6}, "iterations": 10, "balloon": -1, "expected": rows(gac_11x11)},
    "init_level_sets": {"cite": REF + "121", "shape": [6, 6], "iterations": 0,
                        "checkerboard": rows(checkerboard_6x6), "disk": rows(disk_6x6)},
    # a black image: MorphACWE and MorphGAC empty the disk; MorphGAC with a balloon over the whole image fills it
    "black": {"cite": REF + "45", "shape": [11, 11], "level_set_disk": {"center": [5, 5], "radius": 3}, "iterations": 6,
              "acwe": 0, "gac": 0, "gac_balloon": {"balloon": 1, "threshold": -1, "smoothing": 0, "expected": 1}},
    # MorphACWE from the default disk on a black 7 x 7 x 7 volume: the sums of the level set seen by the callback
    "evolution_3d": {"cite": REF + "153", "shape": [7, 7, 7], "iterations": 5, "init_level_set": "disk", "first_sum": 81, "last_sum": 0,
                     "monotone": "non-increasing"},
    # two disks around a Gaussian blob exp(-r^2 / 10) on mgrid[-5:6, -5:6] converge to the same set
    "acwe_simple_shape": {"cite": REF + "73", "blob_half_width": 5, "blob_scale": 10, "center": [5, 5], "radii": [3, 6], "iterations": 10},
}

with open(os.path.join(HERE, "morphsnakes_kat.json"), "w") as f:
    json.dump(cases, f, indent=1)
    f.write("\n")
print("wrote", len(cases), "cases")
