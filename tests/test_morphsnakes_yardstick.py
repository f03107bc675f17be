"""The host transcription of tests/helpers/morphsnakes_ref.py is what the GPU tests hold the device to, so it is checked here
first (no GPU): it reproduces every known answer of the reference's own tests (tests/golden/morphsnakes_kat.json) and their
properties, and every MorphACWE input of the GPU tests meets the condition that makes a bit-exact comparison legitimate:
every masked sum of every iteration is independent of the summation order, so the device's fixed-order double sums and
NumPy's sums in the image dtype are the same numbers."""
import json
import os

import numpy as np
import pytest

from helpers import morphsnakes_ref as ms

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "morphsnakes_kat.json")) as f:
        return json.load(f)


def test_gac_known_answer(kat):
    c = kat["gac_simple_shape"]
    shape = tuple(c["shape"])
    img = ms.disk_level_set(shape, **c["image_disk"]).astype(float)
    gimg = ms.inverse_gaussian_gradient(img, alpha=c["alpha"], sigma=c["sigma"])
    ls = ms.disk_level_set(shape, **c["level_set_disk"])
    got = ms.geodesic_active_contour(gimg, c["iterations"], ls, balloon=c["balloon"])
    assert got.dtype == np.int8
    assert np.array_equal(got, np.array(c["expected"], np.int8))


def test_initial_level_sets(kat):
    c = kat["init_level_sets"]
    image = np.zeros(tuple(c["shape"]))
    assert np.array_equal(ms.chan_vese(image, 0, "checkerboard"), np.array(c["checkerboard"], np.int8))
    assert np.array_equal(ms.geodesic_active_contour(image, 0, "disk"), np.array(c["disk"], np.int8))


def test_black_image(kat):
    c = kat["black"]
    img = np.zeros(tuple(c["shape"]))
    ls = ms.disk_level_set(img.shape, **c["level_set_disk"])
    acwe = ms.chan_vese(img, c["iterations"], ls)
    gac = ms.geodesic_active_contour(img, c["iterations"], ls)
    b = c["gac_balloon"]
    gac2 = ms.geodesic_active_contour(img, c["iterations"], ls, balloon=b["balloon"], threshold=b["threshold"], smoothing=b["smoothing"])
    assert np.array_equal(acwe, np.full(img.shape, c["acwe"], np.int8))
    assert np.array_equal(gac, np.full(img.shape, c["gac"], np.int8))
    assert np.array_equal(gac2, np.full(img.shape, b["expected"], np.int8))
    assert acwe.dtype == gac.dtype == gac2.dtype == np.int8


def test_evolution_3d_shrinks(kat):
    c = kat["evolution_3d"]
    sums = []
    ls = ms.chan_vese(np.zeros(tuple(c["shape"])), c["iterations"], c["init_level_set"], iter_callback=lambda x: sums.append(int(x.sum())))
    assert len(sums) == c["iterations"] + 1
    assert sums[0] == c["first_sum"] and int(ls.sum()) == c["last_sum"]
    assert all(a >= b for a, b in zip(sums[:-1], sums[1:]))


def test_two_disks_converge_to_the_same_set(kat):
    c = kat["acwe_simple_shape"]
    h = c["blob_half_width"]
    coords = np.mgrid[-h:h + 1, -h:h + 1]
    img = np.exp(-(coords ** 2).sum(0) / c["blob_scale"])
    a, b = (ms.chan_vese(img, c["iterations"], ms.disk_level_set(img.shape, center=tuple(c["center"]), radius=r)) for r in c["radii"])
    assert np.array_equal(a, b)
    assert a.dtype == b.dtype == np.int8
    assert 0 < a.sum() < a.size


def test_border_rule_of_sup_inf():
    """an element that reaches outside the image erodes to 0: corners never survive sup_inf, an edge voxel only through the
    elements that lie along its edge"""
    for shape in ((5, 6), (4, 5, 6)):
        out = ms.sup_inf(np.ones(shape, np.int8))
        corner = tuple([0] * len(shape))
        assert out[corner] == 0 and out[tuple(s - 1 for s in shape)] == 0
        assert out[(0,) * (len(shape) - 1) + (2,)] == (1 if len(shape) == 2 else 0)      # 3-D: an edge lies in no whole plane
        assert out[(0, 2, 2)[3 - len(shape):]] == 1                                     # a face / edge voxel survives
        assert np.array_equal(ms.inf_sup(np.zeros(shape, np.int8)), np.zeros(shape, np.int8))


def test_alternation_is_per_call():
    img = ms.exact_image((13, 21), np.float64, 1)
    a = ms.chan_vese(img, 3, "checkerboard", smoothing=1)
    b = ms.chan_vese(img, 3, "checkerboard", smoothing=1)
    assert np.array_equal(a, b)
    u = ms.mask((13, 21), 0.5)
    assert not np.array_equal(ms.curvature(u, 0), ms.curvature(u, 1))


@pytest.mark.parametrize("case", ms.ACWE_CASES, ids=lambda c: "{}-{}-{}".format("x".join(map(str, c[0])), c[1], c[2]))
def test_acwe_inputs_have_order_independent_sums(case):
    shape, dtype, seed = case
    img = ms.exact_image(shape, dtype, seed)
    if np.dtype(dtype) == np.float32:
        assert img.size <= 65000
    perm = ms.rng_for("perm", shape).permutation(img.size)
    seen = []

    def on_sums(*arrays):
        for a in arrays[:2]:
            flat = a.ravel()
            s = flat.sum()
            assert s.dtype == a.dtype
            assert float(s) == float(flat[perm].sum()) == float(flat[::-1].sum()) == float(flat.astype(np.float64).sum())
            assert float(s) == float(np.cumsum(flat)[-1])                        # a plain left-to-right accumulation too
        seen.append(1)

    for smoothing in (1, 2, 3):
        changes = []
        last = [None]

        def cb(u):
            if last[0] is not None:
                changes.append(int((u != last[0]).sum()))
            last[0] = u

        ms.chan_vese(img, 7, "checkerboard", smoothing=smoothing, iter_callback=cb, on_sums=on_sums)
        # not trivial: every one of the first 6 iterations changes voxels
        assert len(changes) == 7 and min(changes[:6]) > 0, changes
    assert len(seen) == 21
