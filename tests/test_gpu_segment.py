"""find_boundaries, mark_boundaries, relabel_sequential, join_segmentations, map_array / ArrayMap and core.unique on the device
(csrc/segment.hip) against the host references of tests/helpers/segment_ref.py and NumPy, bit for bit: the known answers of
tests/golden/segment_kat.json through the public functions; the boundaries on the shared case table over every route
(planner, small tiles, generic); map_array on every forced route; unique against numpy.unique; and one case of each kernel on
poisoned pool memory."""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import segment_ref as R
from helpers.dirty_pool import FILLS, pool_fill
from test_segment_yardstick import (BOUNDARY_DTYPES, BOUNDARY_MODES, BOUNDARY_SHAPES, KAT_CASES, KAT_IDS, boundary_reference, boundary_settings,
                                    check_kat, label_image, same_bits, shape_id, variants)

pytestmark = pytest.mark.gpu

# (small tiles, forced generic route)
SETTINGS = [(0, 0), (1, 0), (0, 1)]


@pytest.fixture(scope="module")
def seg(gpu):
    from cupyimg_amd.skimage import segmentation
    return segmentation


@pytest.fixture(scope="module")
def util(gpu):
    from cupyimg_amd.skimage import util
    return util


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_boundaries
    fn.argtypes = [ctypes.c_int] * 2
    yield fn
    fn(0, 0)


@pytest.fixture()
def route(gpu):
    from cupyimg_amd.skimage.util import _map_array
    yield _map_array.set_route
    _map_array.set_route("auto")


def host(v):
    return v.get() if hasattr(v, "get") and hasattr(v, "ptr") else np.asarray(v)


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("case", KAT_CASES, ids=KAT_IDS)
def test_known_answers(gpu, seg, util, case):
    check_kat(case, seg.find_boundaries, seg.mark_boundaries, seg.relabel_sequential, seg.join_segmentations, util.map_array, util.ArrayMap, host,
              gpu.asarray)


# ---------------------------------------------------------------- find_boundaries
@pytest.mark.parametrize("dtype", BOUNDARY_DTYPES)
@pytest.mark.parametrize("shape", BOUNDARY_SHAPES, ids=shape_id)
def test_find_boundaries_every_route_bit_for_bit(gpu, seg, knob, shape, dtype):
    tiled = len(shape) in (2, 3)
    for variant in variants(dtype):
        labels = label_image(shape, dtype, variant)
        x = gpu.asarray(labels)
        for connectivity, mode, background in boundary_settings(len(shape)):
            want = boundary_reference(shape, dtype, variant, connectivity, mode, background)
            for small, generic in (SETTINGS if tiled else SETTINGS[:1]):
                knob(small, generic)
                got = seg.find_boundaries(x, connectivity, mode, background)
                name = gpu.last_kernel()
                assert ("bd_tile_kernel" if tiled and not generic else "bd_generic_kernel") in name, name
                if tiled:
                    assert seg.last_boundary_launches() == 1
                got = got.get()
                assert same_bits(got, want), (variant, connectivity, mode, background, small, generic, int((got != want).sum()))
                assert set(np.unique(got.view(np.uint8)).tolist()) <= {0, 1}
            knob(0, 0)


def test_small_tiles_put_seams_along_every_axis(gpu, seg, knob):
    """the planner's small boxes are 3 x 5 pixels and 2 x 3 x 5 voxels: (37, 41) and (11, 12, 13) span several along every axis"""
    knob(1, 0)
    for shape, box in (((37, 41), "box=1x3x5"), ((11, 12, 13), "box=2x3x5")):
        seg.find_boundaries(gpu.asarray(label_image(shape, "int32", "plain")))
        assert box in gpu.last_kernel()
        assert all(s > t for s, t in zip(shape, (2, 3, 5)[-len(shape):]))


@pytest.mark.parametrize("dtype", BOUNDARY_DTYPES)
@pytest.mark.parametrize("shape", [s for s in BOUNDARY_SHAPES if len(s) <= 3], ids=shape_id)
def test_find_boundaries_subpixel(gpu, seg, shape, dtype):
    for variant in variants(dtype):
        want = boundary_reference(shape, dtype, variant, 1, "subpixel", 0)
        got = seg.find_boundaries(gpu.asarray(label_image(shape, dtype, variant)), mode="subpixel").get()
        assert "bd_subpixel_kernel" in gpu.last_kernel() and seg.last_boundary_launches() == 1
        assert same_bits(got, want), (variant, int((got != want).sum()))
        assert set(np.unique(got.view(np.uint8)).tolist()) <= {0, 1}


def test_find_boundaries_on_views_offsets_and_host_input(gpu, seg, knob):
    big = label_image((22, 26, 30), "int16", "negative")
    dev = gpu.asarray(big)
    view, hview = dev[::2, 1:25:2, 3::3], big[::2, 1:25:2, 3::3]
    assert not view.flags.c_contiguous
    flat = np.concatenate([np.zeros(1, np.int32), label_image((6, 67), "int32", "max").ravel()])
    offset = gpu.asarray(flat)[1:].reshape(6, 67)
    assert offset.ptr % 16 == 4 and offset.flags.c_contiguous
    bytes_ = np.concatenate([np.zeros(1, np.uint8), label_image((9, 10, 70), "uint8", "plain").ravel()])
    odd = gpu.asarray(bytes_)[1:].reshape(9, 10, 70)
    assert odd.ptr % 2 == 1
    for small, generic in SETTINGS:
        knob(small, generic)
        for mode in BOUNDARY_MODES:
            assert same_bits(seg.find_boundaries(view, 2, mode, -3).get(), R.find_boundaries(hview, 2, mode, -3))
            assert same_bits(seg.find_boundaries(offset, 1, mode, 1).get(), R.find_boundaries(flat[1:].reshape(6, 67), 1, mode, 1))
            assert same_bits(seg.find_boundaries(odd, 3, mode).get(), R.find_boundaries(bytes_[1:].reshape(9, 10, 70), 3, mode))
    knob(0, 0)
    assert same_bits(seg.find_boundaries(view, mode="subpixel").get(), R.find_boundaries_subpixel(hview))
    assert same_bits(seg.find_boundaries(hview.tolist(), mode="outer").get(), R.find_boundaries(hview.astype(np.int64), mode="outer"))
    # a background that is no value of the dtype: no voxel is background
    u8 = label_image((9, 7), "uint8", "plain")
    for mode in BOUNDARY_MODES:
        assert same_bits(seg.find_boundaries(gpu.asarray(u8), 1, mode, 300).get(), R.closed_form_boundaries(u8, 1, mode, 300))


# ---------------------------------------------------------------- map_array
def _map_case(kind, nvals, rng):
    """(keys, voxels): dense keys 0 .. n - 1 shuffled, or int64 keys scattered up to 2^40 (negative ones among them); both with
    duplicate keys, and voxels that have no key"""
    if kind == "dense":
        keys = rng.permutation(nvals).astype(np.int32) - (3 if nvals > 4 else 0)
    else:
        keys = rng.integers(-2 ** 40, 2 ** 40, size=nvals, dtype=np.int64)
    if nvals >= 5:
        keys[nvals // 2] = keys[1]                   # a duplicate: the first wins
        keys[nvals - 1] = keys[0]
    missing = np.array([keys.max() + 7, keys.min() - 2, 12345] if nvals else [-2, 0, 9], keys.dtype)
    missing = missing[~np.isin(missing, keys)]
    voxels = missing[rng.integers(0, len(missing), size=(64, 67))]
    if nvals:                                        # three voxels in four carry a key
        voxels = np.where(rng.random((64, 67)) < 0.75, keys[rng.integers(0, nvals, size=(64, 67))], voxels)
    return keys, voxels


@pytest.mark.parametrize("out_dtype", ["uint8", "int32", "float32", "float64"])
@pytest.mark.parametrize("kind", ["dense", "scattered"])
@pytest.mark.parametrize("nvals", [0, 1, 5, 3000, 70000])
def test_map_array_every_route(gpu, util, route, nvals, kind, out_dtype):
    rng = np.random.default_rng([nvals, len(kind), len(out_dtype)])
    keys, voxels = _map_case(kind, nvals, rng)
    vals = (rng.integers(1, 250, size=nvals) if out_dtype != "float64" else rng.standard_normal(nvals) + 3).astype(out_dtype)
    want = R.map_array(voxels, keys, vals)
    assert not nvals or ((want == 0).any() and (want != 0).any())
    x, k, v = gpu.asarray(voxels), gpu.asarray(keys), gpu.asarray(vals)
    span = int(keys.max()) - int(keys.min()) + 1 if nvals else 0
    routes = ["auto", "search"] + (["table"] if 0 < span <= 2 ** 24 else []) + (["table_lds"] if 0 < span <= 16384 else [])
    for r in routes:
        route(r)
        got = util.map_array(x, k, v)
        name = gpu.last_kernel()
        if nvals and r != "auto":
            assert {"search": "map_search_kernel", "table": "map_gather_kernel<global>", "table_lds": "map_gather_kernel<lds>"}[r] in name, (r, name)
        assert same_bits(got.get(), want), (r, int((got.get() != want).sum()))
    route("auto")
    out = gpu.empty(voxels.shape, out_dtype)
    assert util.map_array(x, k, v, out=out) is out and same_bits(out.get(), want)
    if span > 2 ** 24:                               # the rule's own choice for a range no table is built for
        assert "map_search_kernel" in gpu.last_kernel()
    # keys and values of other dtypes are cast as the reference casts them; a strided input
    if nvals == 5:
        got = util.map_array(x[::2, 1::3], gpu.asarray(keys.astype(np.float64)), gpu.asarray(vals.astype(np.int64)), out=gpu.empty((32, 22), out_dtype))
        assert same_bits(got.get(), R.map_array(voxels[::2, 1::3], keys, vals.astype(np.int64), out_dtype))
        if kind == "scattered":                      # a forced table route refuses a range it cannot hold
            route("table_lds")
            with pytest.raises(ValueError):
                util.map_array(x, k, v)


def test_arraymap_indexing(gpu, util):
    keys, vals = np.array([0, 10, 3, 7], np.int64), np.array([0.25, 1.0, 0.5, 2.0])
    m = util.ArrayMap(gpu.asarray(keys), gpu.asarray(vals))
    dense = R.dense_map(keys, vals)
    assert len(m) == 11 and m.dtype == np.float64 and same_bits(np.asarray(m), dense)
    assert m[10] == 1.0 and m[4] == 0.0
    idx = np.array([[0, 0, 10], [3, 9, 7]])
    assert same_bits(m[gpu.asarray(idx)].get(), dense[idx]) and same_bits(m(gpu.asarray(idx.astype(np.int32))).get(), dense[idx])
    assert same_bits(m[2:9:2].get(), dense[2:9:2]) and same_bits(m[:].get(), dense)
    mask = np.arange(11) % 3 == 1
    assert same_bits(m[gpu.asarray(mask)].get(), dense[mask])
    assert str(m).split("\n") == ["ArrayMap:", "  0 → 0.25", "  10 → 1.0", "  3 → 0.5", "  7 → 2.0"] and repr(m).startswith("ArrayMap(array([")
    with pytest.raises(NotImplementedError):
        m[3] = 1.0
    with pytest.raises(TypeError):
        m[gpu.asarray(np.array([0.5, 1.0]))]


# ---------------------------------------------------------------- unique
FLAGS = list(itertools.product((False, True), repeat=3))


@pytest.fixture()
def small_select(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_select
    fn.argtypes = [ctypes.c_int]
    yield fn
    fn(0)


@pytest.mark.parametrize("dtype", ["uint8", "int16", "int32", "int64", "bool"])
@pytest.mark.parametrize("n", [0, 1, 1000, 200000])
def test_unique_matches_numpy(gpu, small_select, n, dtype):
    # 200 000 elements in tiles of 64 and scan blocks of 64: 3125 tiles, three levels of the scan
    small_select(int(n == 200000))
    rng = np.random.default_rng([n, len(dtype)])
    if dtype == "bool":
        a = rng.random(n) < 0.3
    else:
        info = np.iinfo(dtype)
        a = rng.integers(max(info.min, -700), min(info.max, 700) + 1, size=n).astype(dtype)
        if n > 2:
            a[[0, n // 2]] = info.max, info.min
    x = gpu.asarray(a)
    for index, inverse, counts in FLAGS:
        want = np.unique(a, return_index=index, return_inverse=inverse, return_counts=counts)
        got = gpu.unique(x, return_index=index, return_inverse=inverse, return_counts=counts)
        if not (index or inverse or counts):
            want, got = (want,), (got,)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert same_bits(g.get(), w), (index, inverse, counts, g.dtype, w.dtype)


def test_unique_flattens_any_shape_and_views(gpu):
    a = np.random.default_rng(8).integers(-5, 6, size=(7, 9, 11)).astype(np.int32)
    x = gpu.asarray(a)
    for src, ref in ((x, a), (x[::2, :, 1::3], a[::2, :, 1::3]), (x.transpose(2, 0, 1), a.transpose(2, 0, 1))):
        got = gpu.unique(src, True, True, True)
        want = np.unique(ref, True, True, True)
        for g, w in zip(got, want):
            assert same_bits(g.get(), w)
    assert same_bits(gpu.unique([[3, 1], [1, 3]]).get(), np.array([1, 3]))


# ---------------------------------------------------------------- relabel_sequential
def _maps_hold(gpu, labels, relab, fw, inv):
    assert same_bits(fw[gpu.asarray(labels)].get(), relab.get()) and same_bits(inv[relab].get(), labels)
    assert fw.dtype == relab.dtype and inv.dtype == labels.dtype


def test_relabel_sequential_dtypes_and_identities(gpu, seg):
    u8 = (np.arange(24).reshape(4, 6) % 12 * 20).astype(np.uint8)          # 0 and 11 labels: 250 + 10 does not fit uint8
    relab, fw, inv = seg.relabel_sequential(gpu.asarray(u8), offset=250)
    want = R.relabel_sequential(u8, 250)
    assert relab.dtype == np.uint16 and same_bits(relab.get(), want[0]) and int(relab.get().max()) == 260
    _maps_hold(gpu, u8, relab, fw, inv)
    i32 = np.random.default_rng(9).choice(np.array([0, 5, 9, 70000, 2 ** 31 - 1], np.int32), size=(11, 12, 13))
    for offset in (1, 5):
        relab, fw, inv = seg.relabel_sequential(gpu.asarray(i32), offset=offset)
        want = R.relabel_sequential(i32, offset)
        assert relab.dtype == np.int32 and same_bits(relab.get(), want[0])
        assert same_bits(fw.in_values.get(), want[1]) and same_bits(fw.out_values.get(), want[2])
        _maps_hold(gpu, i32, relab, fw, inv)
    # a strided view, and a field without 0
    view = gpu.asarray(i32)[:, ::2, 1::2]
    assert same_bits(seg.relabel_sequential(view)[0].get(), R.relabel_sequential(i32[:, ::2, 1::2])[0])
    no0 = np.array([7, 7, 2, 9], np.uint16)
    assert same_bits(seg.relabel_sequential(gpu.asarray(no0))[0].get(), np.array([2, 2, 1, 3], np.uint16))
    with pytest.raises(ValueError):
        seg.relabel_sequential(gpu.asarray(np.array([1, -5, 3])))


def test_relabel_closes_the_gaps_small_object_removal_leaves(gpu, seg):
    from cupyimg_amd.scipy import ndimage as ndi
    from cupyimg_amd.skimage import morphology
    mask = R.sndi.binary_dilation(np.random.default_rng(10).random((40, 50)) < 0.04)
    labels, n = ndi.label(gpu.asarray(mask))
    kept = morphology.remove_small_objects(labels, 6)
    kept_h = kept.get()
    present = np.unique(kept_h)
    assert 1 < len(present) < n + 1                             # some objects went, some stayed: the numbering has holes
    relab, fw, inv = seg.relabel_sequential(kept)
    got = relab.get()
    assert relab.dtype == kept.dtype and same_bits(got, R.relabel_sequential(kept_h)[0])
    assert np.array_equal(np.unique(got), np.arange(len(present))) and np.array_equal(got == 0, kept_h == 0)
    _maps_hold(gpu, kept_h, relab, fw, inv)


# ---------------------------------------------------------------- join_segmentations
def test_join_segmentations_in_int64(gpu, seg):
    rng = np.random.default_rng(11)
    s1 = rng.integers(0, 50, size=(11, 12, 13)).astype(np.uint8) * 5
    s2 = rng.integers(0, 70, size=(11, 12, 13)).astype(np.uint8) * 3
    got = seg.join_segmentations(gpu.asarray(s1), gpu.asarray(s2))
    assert "map_" in gpu.last_kernel()
    got = got.get()
    want = R.join_segmentations(s1, s2, int64=True)
    assert want.dtype == np.uint16 and same_bits(got, want)
    pairs = set(zip(s1.ravel().tolist(), s2.ravel().tolist()))
    triples = set(zip(s1.ravel().tolist(), s2.ravel().tolist(), got.ravel().tolist()))
    assert len(pairs) == len(triples) == len(np.unique(got)) > 256
    # where the reference's key does not wrap, its values and dtype
    a, b = (s1 // 50).astype(np.int16), (s2 // 70).astype(np.uint8)
    got = seg.join_segmentations(gpu.asarray(a), gpu.asarray(b)).get()
    assert same_bits(got, R.join_segmentations(a, b)) and got.dtype == np.int16


# ---------------------------------------------------------------- mark_boundaries
def test_mark_boundaries_modes_images_and_subpixel(gpu, seg):
    labels = label_image((37, 41), "int32", "plain")
    rng = np.random.default_rng(12)
    for image in (rng.random((37, 41)), rng.random((37, 41, 3)).astype(np.float32), rng.integers(0, 256, size=(37, 41)).astype(np.uint8),
                  rng.integers(0, 65536, size=(37, 41, 3)).astype(np.uint16)):
        flt = image.astype(np.float64) * (1.0 / np.iinfo(image.dtype).max) if image.dtype.kind == "u" else image      # img_as_float
        rgb = flt if flt.ndim == 3 else np.repeat(flt[..., None], 3, axis=-1)
        for mode, outline in (("outer", None), ("inner", (0.5, 0.25, 2.0)), ("thick", (0, 0, 1))):
            want = rgb.copy()
            bd = R.find_boundaries(labels, mode=mode)
            if outline is not None:
                want[R.sndi.grey_dilation(bd.astype(np.uint8), size=(3, 3)).astype(bool)] = outline
            want[bd] = (1, 1, 0)
            got = seg.mark_boundaries(gpu.asarray(image), gpu.asarray(labels), outline_color=outline, mode=mode)
            assert "paint_kernel" in gpu.last_kernel()
            assert same_bits(got.get(), want.astype(rgb.dtype))
    image = rng.random((9, 7)) * 0.9
    labels = label_image((9, 7), "uint8", "plain")
    marked = seg.mark_boundaries(gpu.asarray(image), gpu.asarray(labels), color=(7, 7, 7), mode="subpixel").get()
    assert marked.shape == (17, 13, 3)
    assert np.array_equal((marked == 7).all(axis=-1), R.find_boundaries_subpixel(labels)) and np.isfinite(marked).all()


# ---------------------------------------------------------------- poisoned pool
def _poisoned(gpu, inputs, call):
    dev = [gpu.asarray(a) for a in inputs]
    gpu.synchronize()
    outs = []
    for byte in FILLS:
        with pool_fill(gpu, byte):
            outs.append(call(*dev))
    return outs


def test_poisoned_pool_boundaries_and_paint(gpu, seg, knob):
    labels = label_image((11, 12, 13), "int16", "negative")
    image2 = label_image((37, 41), "uint16", "max")
    gray = np.random.default_rng(13).random((37, 41))
    for setting, name in (((0, 0), "bd_tile_kernel"), ((1, 0), "bd_tile_kernel"), ((0, 1), "bd_generic_kernel")):
        knob(*setting)
        for got in _poisoned(gpu, [labels, image2], lambda x, y: (seg.find_boundaries(x, 2, "outer", -3).get(), gpu.last_kernel(),
                                                                 seg.find_boundaries(y, 1, "inner", 1).get())):
            assert name in got[1] and same_bits(got[0], R.find_boundaries(labels, 2, "outer", -3)) and same_bits(got[2], R.find_boundaries(image2, 1, "inner", 1))
    knob(0, 0)
    bd = R.find_boundaries(image2, mode="thick")
    want = np.repeat(gray[..., None], 3, axis=-1)
    want[R.sndi.grey_dilation(bd.astype(np.uint8), size=(3, 3)).astype(bool)] = (0, 1, 0)
    want[bd] = (1, 1, 0)
    for got in _poisoned(gpu, [labels, image2, gray], lambda x, y, g: (seg.find_boundaries(x, mode="subpixel").get(),
                                                                      seg.mark_boundaries(g, y, outline_color=(0, 1, 0), mode="thick").get())):
        assert same_bits(got[0], R.find_boundaries_subpixel(labels)) and same_bits(got[1], want)


def test_poisoned_pool_map_array_unique_relabel_join(gpu, seg, util, route):
    rng = np.random.default_rng(14)
    keys, voxels = _map_case("dense", 3000, rng)
    vals = rng.standard_normal(3000).astype(np.float32)
    want = R.map_array(voxels, keys, vals)
    for r in ("table_lds", "table", "search"):
        route(r)
        for got in _poisoned(gpu, [voxels, keys, vals], lambda x, k, v: util.map_array(x, k, v).get()):
            assert same_bits(got, want), r
    route("auto")
    a = rng.integers(-40, 40, size=(50, 90)).astype(np.int16)
    s1, s2 = (np.abs(a) // 4).astype(np.uint8), (a % 7).astype(np.uint8)
    want_u = np.unique(a, return_index=True, return_inverse=True, return_counts=True)
    want_r, want_j = R.relabel_sequential(s1 * 3, 2)[0], R.join_segmentations(s1, s2, int64=True)
    for got in _poisoned(gpu, [a, s1 * 3, s1, s2], lambda x, f, p, q: ([g.get() for g in gpu.unique(x, True, True, True)],
                                                                      seg.relabel_sequential(f, 2)[0].get(), seg.join_segmentations(p, q).get())):
        assert all(same_bits(g, w) for g, w in zip(got[0], want_u))
        assert same_bits(got[1], want_r) and same_bits(got[2], want_j)
