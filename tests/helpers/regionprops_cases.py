"""The label images tests/test_gpu_regionprops.py runs and tests/test_regionprops_yardstick.py vets on the host: small shapes at
which the kernels of csrc/regionprops.hip can still go wrong.

    (10, 18)      the reference's known answers (SAMPLE)
    (37, 70)      2-D regions crossing wave boundaries
    (5, 131)      a row longer than two waves, not a multiple of 64
    (40, 9)       several rows per wave
    (9, 10, 11)   a small volume
    (3, 40, 67)   3-D rows that are not a multiple of 64
    (2, 3, 300)   a 3-D row longer than a wave, few rows
    (7,), (4, 5, 6, 7)   find_objects and remove_small_objects only

Label kinds: "smooth" (the connected components of a smoothed random field: a few blobs), "noise" (those of a 30 % noise mask:
hundreds of regions, many of one voxel), "scatter" (every foreground voxel a label drawn from 1 .. 700: more regions than the
extent pass keeps in LDS, none of them connected, boxes that overlap), "odd" (gaps in the label range, negative values, a
region that touches every face, one-voxel regions) and "full" (one region filling the array).
"""
import json
import os

import numpy as np
import scipy.ndimage as sndi

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES_2D = ((10, 18), (37, 70), (5, 131), (40, 9))
SHAPES_3D = ((9, 10, 11), (3, 40, 67), (2, 3, 300))
SHAPES_OTHER = ((7,), (4, 5, 6, 7))
# rows x columns of the extent table the extent pass keeps in LDS, and entries of the moment tables (csrc/regionprops.hip)
LDS_EXT_SLOTS = 4096
LDS_MOMENT_SLOTS = 4096


def kat():
    with open(os.path.join(os.path.dirname(HERE), "golden", "regionprops_kat.json")) as f:
        return json.load(f)


def kat_array(k, name):
    a = k["arrays"][name]
    return np.array(a["data"], a["dtype"])


def _seed(shape, kind):
    return sum(shape) * 7919 + len(kind) * 104729 + len(shape)


def labels(shape, kind, dtype=np.int32):
    rng = np.random.default_rng(_seed(shape, kind))
    if kind == "kat":
        return kat_array(kat(), "SAMPLE").astype(dtype)
    if kind == "smooth":
        field = sndi.gaussian_filter(rng.standard_normal(shape), 1.5, mode="wrap")
        lab = sndi.label(field > 0.3 * field.std())[0]
    elif kind == "noise":
        lab = sndi.label(rng.random(shape) < 0.3)[0]
    elif kind == "scatter":
        lab = np.where(rng.random(shape) < 0.6, rng.integers(1, 701, size=shape), 0)
    elif kind == "odd":
        lab = sndi.label(rng.random(shape) < 0.25)[0] * 3              # gaps: labels 3, 6, 9, ...
        lab[rng.random(shape) < 0.05] = -2                              # negative values belong to no region
        lab[rng.random(shape) < 0.03] = -(2 ** 31) if np.dtype(dtype).itemsize >= 4 else -7
        frame = np.zeros(shape, bool)                                   # one region touching every face
        for d in range(len(shape)):
            idx = [slice(None)] * len(shape)
            for edge in (0, -1):
                idx[d] = edge
                frame[tuple(idx)] = True
        lab[frame] = 2
        lab.reshape(-1)[lab.size // 2] = 1                              # a one-voxel region with the smallest label
    elif kind == "full":
        lab = np.full(shape, 4)
    else:
        raise ValueError(kind)
    info = np.iinfo(dtype)
    assert lab.max() <= info.max and lab.min() >= info.min, (shape, kind, dtype, lab.min(), lab.max())
    return lab.astype(dtype)


def intensity(shape, dtype):
    rng = np.random.default_rng(sum(shape) + 17)
    if np.dtype(dtype).kind == "f":
        return (rng.random(shape) * 4 + 0.25).astype(dtype)
    return rng.integers(1, 200, size=shape).astype(dtype)


# (id, shape, label kind, label dtype, intensity dtype or None)
TABLE_CASES = [
    ("kat-10x18", (10, 18), "kat", np.int64, np.int64),
    ("smooth-37x70", (37, 70), "smooth", np.uint8, np.uint8),
    ("scatter-37x70", (37, 70), "scatter", np.int32, None),
    ("odd-37x70", (37, 70), "odd", np.int64, np.float64),
    ("noise-5x131", (5, 131), "noise", np.uint16, np.float32),
    ("full-5x131", (5, 131), "full", np.int32, None),
    ("smooth-40x9", (40, 9), "smooth", np.int32, np.float64),
    ("odd-40x9", (40, 9), "odd", np.int32, None),
    ("smooth-9x10x11", (9, 10, 11), "smooth", np.uint8, np.float32),
    ("odd-9x10x11", (9, 10, 11), "odd", np.int64, np.uint8),
    ("noise-3x40x67", (3, 40, 67), "noise", np.uint16, None),
    ("smooth-3x40x67", (3, 40, 67), "smooth", np.int32, np.float64),
    ("smooth-2x3x300", (2, 3, 300), "smooth", np.int64, np.uint8),
    ("full-2x3x300", (2, 3, 300), "full", np.uint8, None),
]
# find_objects and remove_small_objects also on the other ranks
ALL_LABEL_CASES = [(c[0], c[1], c[2], c[3]) for c in TABLE_CASES] + [
    ("smooth-7", (7,), "noise", np.int32), ("odd-7", (7,), "odd", np.int64), ("noise-4x5x6x7", (4, 5, 6, 7), "noise", np.uint16),
    ("odd-4x5x6x7", (4, 5, 6, 7), "odd", np.int32), ("full-4x5x6x7", (4, 5, 6, 7), "full", np.uint8),
]


def properties(ndim, weighted):
    """every supported column of a rank, in one table call"""
    p = ["label", "area", "bbox", "bbox_area", "centroid", "local_centroid", "extent", "equivalent_diameter", "moments", "moments_central",
         "moments_normalized", "inertia_tensor", "inertia_tensor_eigvals", "major_axis_length", "minor_axis_length"]
    if ndim == 2:
        p += ["moments_hu", "eccentricity", "orientation"]
    if weighted:
        p += ["min_intensity", "max_intensity", "mean_intensity", "weighted_centroid", "weighted_local_centroid", "weighted_moments",
              "weighted_moments_central", "weighted_moments_normalized"]
        if ndim == 2:
            p += ["weighted_moments_hu"]
    return p


def bound_rows(areas, limit=6):
    """the rows whose central tables are held to the rational bound: the largest regions, the smallest, and some in between"""
    order = np.argsort(areas, kind="stable")
    pick = list(order[-2:]) + list(order[:2]) + list(order[len(order) // 2:len(order) // 2 + 2])
    return sorted(set(int(i) for i in pick))[:limit]
