"""skimage.morphology.reconstruction on the device (csrc/reconstruct.hip, mi_grey_reconstruction_step; the reference runs its
inner loop on the host, greyreconstruct.py:227-231): bit-identical to the host fixed-point iteration of
tests/helpers/reconstruct_ref.py and to the reference's literal vectors (tests/golden/reconstruction_kat.json) -- block
seams (forced small blocks), the generic one-step kernel against the block-wise one, both methods, box and cross elements,
every dtype, long propagation across launches, arbitrary elements and offsets, the error cases."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import reconstruct_ref as rr

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reconstruction_kat.json")))["cases"]
CROSS = {2: sndi.generate_binary_structure(2, 1), 3: sndi.generate_binary_structure(3, 1)}
SETTINGS = [(0, 0, 0), (4, 5, 0), (0, 0, 1)]        # the planner's blocks, small blocks (many seams), the generic kernel


@pytest.fixture(scope="module")
def morph(gpu):
    from cupyimg_amd.skimage import morphology
    return morphology


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_reconstruct
    fn.argtypes = [ctypes.c_int] * 3
    yield fn
    fn(0, 0, 0)


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_reference_vectors(gpu, morph, knob, case):
    seed = np.array(case["seed"], dtype=case["dtype"])
    mask = np.array(case["mask"], dtype=case["dtype"])
    selem = None if case["selem"] is None else np.array(case["selem"])
    offset = None if case["offset"] is None else np.array(case["offset"])
    want = np.array(case["expected"], dtype=case["dtype"])
    for dtype in (case["dtype"], "float32", "uint8"):
        for setting in SETTINGS:
            knob(*setting)
            got = morph.reconstruction(gpu.asarray(seed.astype(dtype)), gpu.asarray(mask.astype(dtype)), method=case["method"],
                                       selem=selem, offset=offset).get()
            assert got.dtype == np.dtype(dtype)
            assert np.array_equal(got, want.astype(dtype)), (dtype, setting)


def test_reference_error_cases(gpu, morph):
    seed = gpu.asarray(np.ones((5, 5)))
    mask = gpu.asarray(np.ones((5, 5)))
    with pytest.raises(ValueError):
        morph.reconstruction(gpu.asarray(np.ones((5, 5)) * 2), mask, method="dilation")
    with pytest.raises(ValueError):
        morph.reconstruction(gpu.asarray(np.ones((5, 5)) * 0.5), mask, method="erosion")
    with pytest.raises(ValueError):
        morph.reconstruction(seed, mask, selem=np.ones((4, 4)))
    with pytest.raises(ValueError):
        morph.reconstruction(seed, mask, selem=np.ones((3, 4)))
    assert np.array_equal(morph.reconstruction(seed, mask, selem=np.ones((3, 3))).get(), np.ones((5, 5)))
    line_seed = gpu.asarray(np.array([0, 8, 8, 8, 8, 8, 8, 8, 8, 0]))
    line_mask = gpu.asarray(np.array([0, 3, 6, 2, 1, 1, 1, 4, 2, 0]))
    with pytest.raises(ValueError):
        morph.reconstruction(line_seed, line_mask, method="foo")
    two = next(c for c in KAT if c["name"] == "two_image_peaks")
    with pytest.raises(ValueError):
        morph.reconstruction(gpu.asarray(np.array(two["seed"])), gpu.asarray(np.array(two["mask"])), method="dilation",
                             selem=np.ones((3, 3)), offset=np.array([3, 0]))
    with pytest.raises(ValueError):
        morph.reconstruction(seed, gpu.asarray(np.ones((5, 6))))
    # a single voxel out of order, far from the first block, in a volume the block-wise kernel takes
    big_mask = np.full((20, 37, 64), 5, np.uint8)
    big_seed = np.full((20, 37, 64), 3, np.uint8)
    big_seed[19, 36, 63] = 6
    with pytest.raises(ValueError):
        morph.reconstruction(gpu.asarray(big_seed), gpu.asarray(big_mask))
    with pytest.raises(ValueError):
        morph.reconstruction(gpu.asarray(big_mask), gpu.asarray(big_seed), method="erosion")


# ---------------------------------------------------------------- shapes and seams
SHAPES = [(20, 37, 64), (9, 50, 130), (33, 18, 257), (70, 96), (5, 1040), (3, 3, 3), (1, 1, 7)]


@pytest.mark.parametrize("kind", ["plateau", "hdome"])
@pytest.mark.parametrize("dtype", ["uint8", "int16", "uint16", "float32"])
@pytest.mark.parametrize("elem", ["box", "cross"])
@pytest.mark.parametrize("method", ["dilation", "erosion"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_blocks_seams_and_generic_agree_with_host(gpu, morph, knob, shape, method, elem, dtype, kind):
    from cupyimg_amd import last_kernel
    rng = rr.rng_for(shape, method, elem, dtype, kind)
    seed, mask = (rr.plateau_input if kind == "plateau" else rr.hdome_input)(shape, dtype, method, rng)
    selem = None if elem == "box" else CROSS[len(shape)]
    want = rr.reconstruct(seed, mask, method=method, selem=selem)
    assert (want != seed).any()
    sd, md = gpu.asarray(seed), gpu.asarray(mask)
    for setting in SETTINGS:
        knob(*setting)
        got = morph.reconstruction(sd, md, method=method, selem=selem)
        name = last_kernel()
        assert ("greyrec_generic_kernel" if setting[2] else "greyrec3_kernel<{},{}>".format(dtype, method)) in name, name
        if not setting[2]:
            assert ("box" if elem == "box" else "cross") in name, name
        assert got.dtype == np.dtype(dtype)
        assert np.array_equal(got.get(), want), (setting, name)
    assert np.array_equal(sd.get(), seed) and np.array_equal(md.get(), mask)


# ---------------------------------------------------------------- long propagation across launches
@pytest.mark.parametrize("axes", [(0, 1, 2), (2, 1, 0)], ids=["along_x", "along_z"])
@pytest.mark.parametrize("setting", [(2, 3, 0), (0, 0, 0)], ids=["small_blocks", "planner"])
def test_serpentine(gpu, morph, knob, setting, axes):
    from cupyimg_amd import last_kernel
    seed, mask, path = rr.serpentine((6, 40, 72))
    assert len(path) == 1460
    seed, mask = np.ascontiguousarray(seed.transpose(axes)), np.ascontiguousarray(mask.transpose(axes))
    knob(*setting)
    got = morph.reconstruction(gpu.asarray(seed), gpu.asarray(mask), selem=CROSS[3]).get()
    assert "greyrec3_kernel<uint8,dilation>" in last_kernel()
    launches = morph.last_reconstruction_launches()
    print("serpentine", setting, axes, "launches", launches)
    assert int((got == 150).sum()) == 1460
    assert np.array_equal(got, np.where(mask == 200, 150, 0).astype(np.uint8))
    assert 1 < launches < len(path)                 # a launch carries information further than one voxel


# ---------------------------------------------------------------- the generic route
def _check(gpu, morph, seed, mask, **kw):
    want = rr.reconstruct(seed, mask, **kw)
    got = morph.reconstruction(gpu.asarray(seed), gpu.asarray(mask), **kw)
    assert got.dtype == want.dtype == np.promote_types(seed.dtype, mask.dtype)
    assert np.array_equal(got.get(), want)
    return want


@pytest.mark.parametrize("method", ["dilation", "erosion"])
def test_generic_ranks_and_dtypes(gpu, morph, method):
    from cupyimg_amd import last_kernel
    for shape in [(10,), (3, 4, 5, 6)]:
        for dtype in ("float64", "int32", "int8", "uint32"):
            rng = rr.rng_for("generic", shape, dtype, method)
            seed, mask = rr.plateau_input(shape, dtype, method, rng)
            mask.flat[:2] = 5
            seed.flat[0] = 5
            want = _check(gpu, morph, seed, mask, method=method)
            assert "greyrec_generic_kernel" in last_kernel()
            assert (want != seed).any()
    # 64-bit integers beyond what float64 holds: neighbouring values differ in their lowest bits only
    for dtype, base in (("int64", 2 ** 62), ("uint64", 2 ** 63 + 2 ** 60), ("int64", -2 ** 62)):
        rng = rr.rng_for("wide", dtype, base, method)
        mask = rng.integers(0, 8, size=(7, 9, 11)).astype(dtype) + np.array(base, dtype)
        seed = np.full(mask.shape, base - 5 if method == "dilation" else base + 12, dtype)
        pick = rng.random(mask.shape) < 0.05
        seed[pick] = mask[pick]
        want = _check(gpu, morph, seed, mask, method=method)
        assert (want != seed).any() and len(np.unique(want)) > 3
    # float16 keeps its dtype
    rng = rr.rng_for("half", method)
    seed, mask = rr.hdome_input((6, 20, 33), np.float32, method, rng)
    _check(gpu, morph, seed.astype(np.float16), mask.astype(np.float16), method=method)


def test_generic_bool_and_mixed_dtypes(gpu, morph):
    rng = rr.rng_for("bool")
    mask = rng.random((12, 30, 40)) < 0.6
    seed = mask & (rng.random(mask.shape) < 0.02)
    want = _check(gpu, morph, seed, mask, selem=CROSS[3])
    assert want.dtype == np.bool_ and np.array_equal(want, sndi.binary_propagation(seed, mask=mask))
    _check(gpu, morph, ~seed | ~mask, ~mask, method="erosion")
    for sdt, mdt in (("uint8", "int16"), ("int16", "float32"), ("uint8", "float64"), ("bool", "uint8"), ("int32", "int64"),
                     ("float32", "uint8")):
        m = rng.integers(0, 8, size=(9, 21, 35))
        s = np.where(rng.random(m.shape) < 0.03, m, 0)
        if sdt == "bool":
            s = np.minimum(s, 1)
        want = _check(gpu, morph, s.astype(sdt), m.astype(mdt))
        assert want.dtype == np.promote_types(sdt, mdt)


@pytest.mark.parametrize("method", ["dilation", "erosion"])
def test_generic_elements_and_offsets(gpu, morph, method):
    from cupyimg_amd import last_kernel
    rng = rr.rng_for("elements", method)
    shape = (14, 25, 31)
    seed, mask = rr.plateau_input(shape, np.int16, method, rng)
    selem = rng.random((3, 5, 3)) < 0.45
    assert not np.array_equal(selem, selem[::-1, ::-1, ::-1])
    want = _check(gpu, morph, seed, mask, method=method, selem=selem, offset=np.array([2, 1, 0]))
    assert "greyrec_generic_kernel" in last_kernel() and (want != seed).any()
    _check(gpu, morph, seed, mask, method=method, selem=selem.astype(np.uint8), offset=[0, 4, 1])
    # one-sided element, corner offset: values move towards larger indices only (the reference's offset test in 3-D)
    want = _check(gpu, morph, seed, mask, method=method, selem=np.ones((2, 2, 2)), offset=[0, 0, 0])
    one = np.full(shape, rr.extreme(np.int16, method), np.int16)
    one[5, 9, 11] = 4
    flat = np.full(shape, 4, np.int16)
    got = _check(gpu, morph, one, flat, method=method, selem=np.ones((2, 2, 2)), offset=[0, 0, 0])
    reached = got == 4
    assert reached[5:, 9:, 11:].all() and reached.sum() == reached[5:, 9:, 11:].size
    # the cross off its centre and an element that is its centre alone
    _check(gpu, morph, seed, mask, method=method, selem=CROSS[3], offset=[0, 1, 1])
    assert "greyrec_generic_kernel" in last_kernel()
    assert np.array_equal(_check(gpu, morph, seed, mask, method=method, selem=np.ones((1, 1, 1))), seed)


def test_views_host_inputs_and_device_selem(gpu, morph):
    from cupyimg_amd import last_kernel
    rng = rr.rng_for("views")
    seed, mask = rr.plateau_input((20, 24, 70), np.uint8, "dilation", rng)
    want = rr.reconstruct(seed[::2, :, 3:67], mask[::2, :, 3:67], selem=CROSS[3])
    sd, md = gpu.asarray(seed), gpu.asarray(mask)
    got = morph.reconstruction(sd[::2, :, 3:67], md[::2, :, 3:67], selem=gpu.asarray(CROSS[3].astype(np.uint8)))
    assert "greyrec3_kernel" in last_kernel() and np.array_equal(got.get(), want)
    got = morph.reconstruction(seed[::2, :, 3:67], mask[::2, :, 3:67], selem=CROSS[3])          # NumPy inputs
    assert isinstance(got, gpu.ndarray) and np.array_equal(got.get(), want)
    tr = morph.reconstruction(sd.transpose(2, 1, 0), md.transpose(2, 1, 0))
    assert np.array_equal(tr.get(), rr.reconstruct(seed.transpose(2, 1, 0), mask.transpose(2, 1, 0)))
    assert np.array_equal(sd.get(), seed) and np.array_equal(md.get(), mask)


# ---------------------------------------------------------------- binary cross-check, aliasing
def test_binary_volume_equals_binary_propagation(gpu, morph):
    from cupyimg_amd import last_kernel
    rng = rr.rng_for("binary", (64, 96, 128))
    mask = sndi.gaussian_filter(rng.standard_normal((64, 96, 128)), 2.0) > 0.0
    seed = mask & (rng.random(mask.shape) < 0.0005)
    ref = sndi.binary_propagation(seed, mask=mask)
    assert seed.sum() < ref.sum() < mask.sum()
    got = morph.reconstruction(gpu.asarray(seed.astype(np.uint8)), gpu.asarray(mask.astype(np.uint8)), selem=CROSS[3])
    assert "greyrec3_kernel<uint8,dilation>" in last_kernel()
    print("binary 64x96x128: launches", morph.last_reconstruction_launches())
    assert got.dtype == np.uint8 and np.array_equal(got.get(), ref.astype(np.uint8))


@pytest.mark.parametrize("shape", [(12, 20, 70), (9,)])
def test_seed_is_mask(gpu, morph, shape):
    rng = rr.rng_for("alias", shape)
    x = rng.integers(0, 200, size=shape).astype(np.uint8)
    xd = gpu.asarray(x)
    for method in ("dilation", "erosion"):
        got = morph.reconstruction(xd, xd, method=method)
        assert got is not xd and got.ptr != xd.ptr
        assert np.array_equal(got.get(), x)
        got.fill(0)
        assert np.array_equal(xd.get(), x)
