"""The host reference the GPU reconstruction tests compare against (tests/helpers/reconstruct_ref.py) is itself right:
it reproduces every literal vector of the reference's test_reconstruction.py (tests/golden/reconstruction_kat.json), equals
scipy.ndimage.binary_propagation on {0, 1} images, obeys the erosion / dilation duality, and its serpentine builder makes
a corridor whose length is known by construction.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import reconstruct_ref as rr

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reconstruction_kat.json")))["cases"]


@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_helper_reproduces_reference_vectors(case):
    seed = np.array(case["seed"], dtype=case["dtype"])
    mask = np.array(case["mask"], dtype=case["dtype"])
    selem = None if case["selem"] is None else np.array(case["selem"])
    got = rr.reconstruct(seed, mask, method=case["method"], selem=selem, offset=case["offset"])
    assert got.dtype == seed.dtype
    assert np.array_equal(got, np.array(case["expected"], dtype=case["dtype"]))


def test_helper_vector_names():
    assert [c["name"] for c in KAT] == ["zeros", "image_equals_mask", "image_less_than_mask", "one_image_peak", "two_image_peaks",
                                        "zero_image_one_mask", "fill_hole", "offset_not_none"]


def test_helper_equals_binary_propagation():
    rng = rr.rng_for("binary", (24, 40, 64))
    mask = rng.random((24, 40, 64)) < 0.55
    seed = mask & (rng.random(mask.shape) < 0.01)
    cross = sndi.generate_binary_structure(3, 1)
    got = rr.reconstruct(seed.astype(np.uint8), mask.astype(np.uint8), selem=cross)
    ref = sndi.binary_propagation(seed, mask=mask)
    assert ref.sum() > seed.sum()
    assert np.array_equal(got.astype(bool), ref)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_erosion_is_negated_dilation_of_negated_inputs(dtype):
    rng = rr.rng_for("duality", np.dtype(dtype).name)
    shape = (9, 14, 20)
    mask = rng.integers(-50, 50, size=shape).astype(dtype)
    seed = np.maximum(mask, rng.integers(-50, 50, size=shape).astype(dtype))      # erosion: seed >= mask
    selem = rng.random((3, 3, 3)) < 0.5
    offset = [1, 0, 2]
    ero = rr.reconstruct(seed, mask, method="erosion", selem=selem, offset=offset)
    dil = rr.reconstruct(-seed, -mask, method="dilation", selem=selem, offset=offset)
    assert np.array_equal(ero, -dil)
    assert (ero != seed).any()
    # the reference's offset vector, negated: the one-sided element propagates to the right only
    s = -np.array([0, 3, 6, 2, 1, 1, 1, 4, 2, 0], dtype)
    m = -np.array([0, 8, 6, 8, 8, 8, 8, 4, 4, 0], dtype)
    assert np.array_equal(rr.reconstruct(s, m, method="erosion", selem=np.ones(3), offset=[0]),
                          -np.array([0, 3, 6, 6, 6, 6, 6, 4, 4, 0], dtype))


def test_serpentine_path_length_is_the_corridor():
    seed, mask, path = rr.serpentine((6, 40, 72))
    assert len(path) == 1460 == len(set(path)) == int((mask == 200).sum())
    steps = np.abs(np.diff(np.array(path), axis=0)).sum(1)
    assert (steps == 1).all()                                   # consecutive voxels are face neighbours ...
    corridor = mask == 200
    nb = sndi.convolve(corridor.astype(np.int32), sndi.generate_binary_structure(3, 1).astype(np.int32), mode="constant") - 1
    assert sorted(nb[corridor].tolist()) == [1, 1] + [2] * 1458  # ... and no others are: one way through, no shortcut
    assert int((seed != 0).sum()) == 1 and seed[path[0]] == 150
    got = rr.reconstruct(seed, mask, selem=sndi.generate_binary_structure(3, 1))
    assert int((got == 150).sum()) == 1460 and np.array_equal(got == 150, corridor) and (got[~corridor] == 0).all()
