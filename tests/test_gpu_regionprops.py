"""find_objects, regionprops / regionprops_table and remove_small_objects / remove_small_holes on the device
(csrc/regionprops.hip) against the NumPy transcription of the reference (tests/helpers/regionprops_ref.py), on both routes of
mi_debug_set_regionprops (run heads to per-workgroup LDS copies where the tables fit, or straight to global memory).

The contract, column by column:
  * exact: find_objects, label, area, bbox, bbox_area, slice, image, remove_small_*;
  * bit for bit with the transcription: centroid, local_centroid (quotients of exact integers), the unweighted raw moments and
    the weighted ones of integer intensities (every term and partial sum an integer below 2**53), extent, and
    equivalent_diameter in 2-D;
  * central tables (and float-weighted raw ones): |got - exact| <= (area + 16) 2**-53 sum|term| per entry, `exact` and the sum
    in rational arithmetic about the device's own float64 centre;
  * derived columns against the transcription applied to the device's own tables read back: bit for bit where a column is
    made of + - x / and sqrt; eigenvalues within 8 eps |T|_F of numpy.linalg.eigvalsh; the columns through pow or atan2
    (equivalent_diameter in 3-D, moments_normalized, orientation) within ULP_BOUND units in the last place.

ULP_BOUND: twice the largest distance measured over this file's cases on an MI355X, rounded up (device and host libm differ
by design); the measured figure is in DESIGN 4.18.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as sndi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from helpers import dirty_pool
from helpers import regionprops_cases as cases
from helpers import regionprops_ref as ref

pytestmark = pytest.mark.gpu

ULP_BOUND = 4                   # measured: 2 (moments_normalized), 1 (orientation), 1 (equivalent_diameter in 3-D)
EPS = np.finfo(np.float64).eps
KAT = cases.kat()
MEASURED = {}                   # column family -> largest ulp distance seen (printed by the last test)


def _lib():
    from cupyimg_amd import _lib as L
    return L.load()


@pytest.fixture(params=(0, 1), ids=("lds", "global"))
def route(gpu, request):
    lib = _lib()
    assert lib.mi_debug_set_regionprops(ctypes.c_int(request.param)) == 0
    try:
        yield request.param
    finally:
        lib.mi_debug_set_regionprops(ctypes.c_int(0))


_INPUTS = {}
_WANT = {}


def _inputs(case):
    name, shape, kind, ldt, idt = case
    if name not in _INPUTS:
        lab = cases.labels(shape, kind, ldt)
        inten = None if idt is None else cases.intensity(shape, idt)
        lab.setflags(write=False)
        if inten is not None:
            inten.setflags(write=False)
        _INPUTS[name] = (lab, inten)
    return _INPUTS[name]


def _want(case):
    """the transcription's table and regions of a case: computed once, shared, left unchanged"""
    name = case[0]
    if name not in _WANT:
        lab, inten = _inputs(case)
        props = cases.properties(lab.ndim, inten is not None)
        table = ref.regionprops_table(lab, inten, properties=props)
        for v in table.values():
            v.setflags(write=False)
        _WANT[name] = (props, table, ref.regionprops(lab, inten))
    return _WANT[name]


def _host(table):
    return {k: (v.get() if hasattr(v, "get") else v) for k, v in table.items()}


def _stack(table, prop, shape):
    """(K,) + shape array of a property's columns"""
    cols =[table[n] for n in table if n == prop or n.startswith(prop + "-")]
    return np.stack(cols, axis=1).reshape((len(cols[0]),) + tuple(shape))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))))


def _note(family, ulps):
    MEASURED[family] = max(MEASURED.get(family, 0), ulps)
    print("ulp distance, {}: {}".format(family, ulps))


def check_table(got, case, weighted_exact):
    """one device table (host arrays) against the contract"""
    props, want, regions = _want(case)
    lab, inten = _inputs(case)
    nd = lab.ndim
    assert list(got) == list(want)
    K = len(regions)
    for name in want:
        assert got[name].shape == (K,), name
        assert got[name].dtype == want[name].dtype, (name, got[name].dtype, want[name].dtype)
    # ---- exact columns
    for name in want:
        p = name.split("-")[0]
        if p in ("label", "area", "bbox", "bbox_area", "min_intensity", "max_intensity"):
            assert np.array_equal(got[name], want[name]), name
        elif p in ("centroid", "local_centroid", "moments", "extent") or (p == "equivalent_diameter" and nd == 2) or \
                (p == "weighted_moments" and weighted_exact):
            assert _same_bits(got[name], want[name]), name
        elif p == "mean_intensity":
            if weighted_exact:
                assert _same_bits(got[name], want[name]), name
            else:
                # positive intensities: each of the two float64 sums carries at most area - 1 roundings, then a division each
                areas = np.array([r.area for r in regions], np.float64)
                assert np.all(np.abs(got[name] - want[name]) <= (2 * areas + 2) * 2.0 ** -53 * np.abs(want[name])), name
    if nd == 3:
        d = ref.ulp_distance(got["equivalent_diameter"], want["equivalent_diameter"])
        _note("equivalent_diameter-3d", d)
        assert d <= ULP_BOUND
    # ---- central tables within the rational bound about the device's own centre
    T = (4,) * nd
    sets = [("", "moments_central", "local_centroid", lambda r: r.image)]
    if inten is not None:
        sets.append(("weighted_", "weighted_moments_central", "weighted_local_centroid", lambda r: r.intensity_image))
    areas = [r.area for r in regions]
    for pre, central, centre, weights in sets:
        mu = _stack(got, central, T)
        ctr = _stack(got, centre, (nd,))
        if pre:
            # the weighted centre is the quotient of the device's own raw table's entries
            raw = _stack(got, "weighted_moments", T)
            for d in range(nd):
                idx = (slice(None),) + tuple(1 if a == d else 0 for a in range(nd))
                with np.errstate(all="ignore"):
                    assert _same_bits(ctr[:, d], raw[idx] / raw[(slice(None),) + (0,) * nd]), (centre, d)
        # every row against the transcription about the device's own centre: each of the two is within the bound of the exact
        # table, so they are within twice the bound of each other (sum|term| in float64 here, 1 + 1e-9 for its own rounding)
        for row, r in enumerate(regions):
            w = np.asarray(weights(r))
            want_mu = ref.moments_central(w, ctr[row])
            room = 2 * (r.area + 16) * 2.0 ** -53 * ref.central_sumabs(w, ctr[row]) * (1 + 1e-9)
            assert np.all(np.abs(mu[row] - want_mu) <= room), (central, row)
        # and the largest, smallest and middle rows against rational arithmetic itself
        for row in cases.bound_rows(areas):
            r = regions[row]
            worst = ref.within_central_bound(mu[row], weights(r), ctr[row], r.area)
            assert worst <= 1.0, (central, row, worst)
            if pre and not weighted_exact:
                worst = ref.within_central_bound(raw[row], weights(r), (0.0,) * nd, r.area)
                assert worst <= 1.0, ("weighted_moments", row, worst)
        # ---- derived columns against the transcription applied to the device's own tables
        nu = _stack(got, pre + "moments_normalized", T)
        want_nu = np.stack([ref.moments_normalized(m) for m in mu])
        d = ref.ulp_distance(nu, want_nu)
        _note("moments_normalized", d)
        assert d <= ULP_BOUND
        if nd == 2:
            hu = _stack(got, pre + "moments_hu", (7,))
            assert _same_bits(hu, np.stack([ref.moments_hu(n) for n in nu])), pre + "moments_hu"
        if pre:
            continue
        it = _stack(got, "inertia_tensor", (nd, nd))
        assert _same_bits(it, np.stack([ref.inertia_tensor(m) for m in mu])), "inertia_tensor"
        ev = _stack(got, "inertia_tensor_eigvals", (nd,))
        for row in range(K):
            if np.all(np.isfinite(it[row])):
                lam = np.sort(np.clip(np.linalg.eigvalsh(it[row]), 0, None))[::-1]
                assert np.all(np.abs(ev[row] - lam) <= 8 * EPS * np.linalg.norm(it[row])), (row, ev[row], lam)
                assert np.all(ev[row] >= 0) and np.all(np.diff(ev[row]) <= 0)
        with np.errstate(all="ignore"):
            assert _same_bits(got["major_axis_length"], 4 * np.sqrt(ev[:, 0]))
            assert _same_bits(got["minor_axis_length"], 4 * np.sqrt(ev[:, -1]))
        if nd == 2:
            drv = [ref.derived(2, r.area, r.slice, None, mu[k], eigvals=ev[k], T=it[k], nu=nu[k]) for k, r in enumerate(regions)]
            assert _same_bits(got["eccentricity"], np.array([d["eccentricity"] for d in drv]))
            d = ref.ulp_distance(got["orientation"], np.array([d["orientation"] for d in drv]))
            _note("orientation", d)
            assert d <= ULP_BOUND


def _table(gpu, case, **kw):
    from cupyimg_amd.skimage import measure
    lab, inten = _inputs(case)
    dl = gpu.asarray(lab)
    di = None if inten is None else gpu.asarray(inten)
    props = cases.properties(lab.ndim, inten is not None)
    got = _host(measure.regionprops_table(dl, di, properties=props, **kw))
    assert np.array_equal(dl.get(), lab) and (di is None or np.array_equal(di.get(), inten))          # inputs come back untouched
    return got


@pytest.mark.parametrize("case", cases.TABLE_CASES, ids=[c[0] for c in cases.TABLE_CASES])
def test_table_against_the_transcription(gpu, route, case):
    inten = _inputs(case)[1]
    check_table(_table(gpu, case), case, inten is not None and inten.dtype.kind in "iu")


EXACT_PROPS = ("label", "area", "bbox", "bbox_area", "centroid", "local_centroid", "moments", "extent", "equivalent_diameter",
               "min_intensity", "max_intensity")


@pytest.mark.parametrize("case", cases.TABLE_CASES, ids=[c[0] for c in cases.TABLE_CASES])
def test_routes_agree_bit_for_bit_on_the_exact_columns(gpu, case):
    lib = _lib()
    tables = []
    try:
        for knob in (0, 1):
            assert lib.mi_debug_set_regionprops(ctypes.c_int(knob)) == 0
            tables.append(_table(gpu, case))
    finally:
        lib.mi_debug_set_regionprops(ctypes.c_int(0))
    for name in tables[0]:
        if name.split("-")[0] in EXACT_PROPS:
            a, b = tables[0][name], tables[1][name]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


def test_the_knob_selects_the_route(gpu):
    from cupyimg_amd.scipy import ndimage as ndi
    lib = _lib()
    lab = gpu.asarray(cases.labels((37, 70), "smooth", np.int32))
    try:
        ndi.find_objects(lab)
        assert "rp_extent_kernel" in gpu.last_kernel() and "LDS atomics" in gpu.last_kernel(), gpu.last_kernel()
        lib.mi_debug_set_regionprops(ctypes.c_int(1))
        ndi.find_objects(lab)
        assert "global atomics" in gpu.last_kernel(), gpu.last_kernel()
    finally:
        lib.mi_debug_set_regionprops(ctypes.c_int(0))
    ndi.find_objects(gpu.asarray(cases.labels((37, 70), "scatter", np.int32)))
    assert "global atomics" in gpu.last_kernel(), gpu.last_kernel()          # 700 rows x 7 columns: above the LDS slots


# ------------------------------------------------------------------ find_objects
@pytest.mark.parametrize("case", cases.ALL_LABEL_CASES, ids=[c[0] for c in cases.ALL_LABEL_CASES])
def test_find_objects_is_scipys(gpu, route, case):
    from cupyimg_amd.scipy import ndimage as ndi
    _, shape, kind, dtype = case
    lab = cases.labels(shape, kind, dtype)
    dev = gpu.asarray(lab)
    pos = np.where(lab > 0, lab, 0)
    top = int(lab.max())
    for max_label in (0, max(top - 2, 1), top, top + 3):            # below, at and above the maximum
        assert ndi.find_objects(dev, max_label) == sndi.find_objects(pos, max_label), max_label
    assert np.array_equal(dev.get(), lab)


def test_find_objects_other_inputs(gpu, route):
    from cupyimg_amd.scipy import ndimage as ndi
    rng = np.random.default_rng(5)
    mask = rng.random((9, 33)) < 0.5
    assert ndi.find_objects(gpu.asarray(mask)) == sndi.find_objects(mask.astype(np.int8))
    assert ndi.find_objects(mask) == sndi.find_objects(mask.astype(np.int8))                    # a host array is uploaded
    for dtype in (np.int8, np.uint32, np.uint64, np.int16):
        lab = rng.integers(0, 9, size=(6, 7, 8)).astype(dtype)
        assert ndi.find_objects(gpu.asarray(lab)) == sndi.find_objects(lab.astype(np.int64)), dtype
    assert ndi.find_objects(gpu.asarray(np.zeros((4, 5), np.int32))) == []
    assert ndi.find_objects(gpu.asarray(np.full((4, 5), -3, np.int32))) == []
    assert ndi.find_objects(gpu.asarray(np.zeros((4, 5), np.int32)), 2) == [None, None]
    big = np.zeros((3, 4), np.uint64)
    big[1, 2] = 2 ** 63
    with pytest.raises(ValueError, match="2\\*\\*63"):
        ndi.find_objects(gpu.asarray(big))
    lab = cases.labels((37, 70), "smooth", np.int32)
    view = gpu.asarray(lab)[::2, 1::3]                                                       # a strided view is compacted first
    assert ndi.find_objects(view) == sndi.find_objects(lab[::2, 1::3])


# ------------------------------------------------------------------ regionprops
def _value(region, prop):
    v = region[prop] if prop[0].isupper() else getattr(region, prop)
    return v.get() if hasattr(v, "get") and hasattr(v, "ptr") else v


@pytest.mark.parametrize("case", KAT["props"], ids=[c["name"] for c in KAT["props"]])
def test_regionprops_meets_the_known_answers(gpu, route, case):
    from cupyimg_amd.skimage import measure
    from make_regionprops_kat import check_props
    lab = cases.kat_array(KAT, case["labels"])
    inten = None if case["intensity"] is None else cases.kat_array(KAT, case["intensity"])
    regions = measure.regionprops(gpu.asarray(lab), None if inten is None else gpu.asarray(inten))
    check_props(case, regions, get=_value)


def test_regionprops_objects(gpu, route):
    from cupyimg_amd.skimage import measure
    lab = cases.kat_array(KAT, "SAMPLE_MULTIPLE")
    inten = cases.kat_array(KAT, "INTENSITY_SAMPLE_MULTIPLE")
    dl, di = gpu.asarray(lab), gpu.asarray(inten)
    regions = measure.regionprops(dl, di)
    want = ref.regionprops(lab, inten)
    assert [r.label for r in regions] == [1, 2] and all(isinstance(r, measure.RegionProperties) for r in regions)
    for r, w in zip(regions, want):
        assert r.slice == w.slice and r.bbox == w.bbox and r.area == w.area and r.bbox_area == w.bbox_area
        assert isinstance(r.image, gpu.ndarray) and r.image.dtype == bool and np.array_equal(r.image.get(), w.image)
        assert r.intensity_image.dtype == inten.dtype and np.array_equal(r.intensity_image.get(), w.intensity_image)
        assert r.centroid == w.centroid and r.local_centroid == tuple(w.local_centroid)
        assert np.array_equal(r.moments, w.moments) and np.array_equal(r.weighted_moments, w.weighted_moments)
        assert r.min_intensity == w.min_intensity and r.max_intensity == w.max_intensity and r.mean_intensity == w.mean_intensity
        assert r["Area"] == r.area and r["BoundingBox"] == r.bbox and np.array_equal(r["Moments"], r.moments) and r["area"] == r.area
        assert "area" in list(r) and "coords" not in list(r) and "weighted_moments" in list(r)
        with pytest.raises(NotImplementedError, match="convex_area"):
            r.convex_area
        with pytest.raises(AttributeError):
            r.no_such_property
    assert "weighted_moments" not in list(measure.regionprops(dl)[0])
    with pytest.raises(AttributeError, match="No intensity image"):
        measure.regionprops(dl)[0].intensity_image
    again = measure.regionprops(dl, di)
    assert regions[0] == again[0] and regions[0] != again[1] and regions[0] != "region"
    r3 = measure.regionprops(gpu.asarray(cases.kat_array(KAT, "SAMPLE_3D")))[0]
    for prop in ("eccentricity", "moments_hu", "orientation"):
        with pytest.raises(NotImplementedError, match="3D"):
            getattr(r3, prop)
    assert r3.moments.shape == (4, 4, 4) and r3.inertia_tensor.shape == (3, 3) and len(r3.inertia_tensor_eigvals) == 3
    assert measure.regionprops(gpu.asarray(np.zeros((0, 4), np.int32))) == []


def test_table_layout_zero_regions_and_object_columns(gpu, route):
    from cupyimg_amd.skimage import measure
    lab = cases.kat_array(KAT, "SAMPLE_MULTIPLE")
    inten = cases.kat_array(KAT, "INTENSITY_SAMPLE_MULTIPLE").astype(np.float32)
    props = ("label", "area", "bbox", "centroid", "inertia_tensor", "min_intensity", "slice", "image", "intensity_image")
    got = measure.regionprops_table(gpu.asarray(lab), gpu.asarray(inten), properties=props)
    want = ref.regionprops_table(lab, inten, properties=props)
    assert list(got) == list(want)
    for name in want:
        if want[name].dtype == object:
            assert isinstance(got[name], np.ndarray) and got[name].dtype == object and len(got[name]) == 2
        else:
            assert isinstance(got[name], gpu.ndarray) and got[name].dtype == want[name].dtype, name
    assert list(got["slice"]) == list(want["slice"])
    for k in range(2):
        assert np.array_equal(got["image"][k].get(), want["image"][k])
        assert np.array_equal(got["intensity_image"][k].get(), want["intensity_image"][k])
    assert list(measure.regionprops_table(gpu.asarray(lab), properties=("moments",), separator="_"))[:2] == ["moments_0_0", "moments_0_1"]
    for empty in (np.zeros((4, 5), np.int32), np.full((4, 5), -1, np.int64), np.zeros((0, 5), np.int32)):
        z = measure.regionprops_table(gpu.asarray(empty), gpu.asarray(np.zeros(empty.shape, np.float32)),
                                      properties=("label", "centroid", "max_intensity", "image"))
        assert list(z) == ["label", "centroid-0", "centroid-1", "max_intensity", "image"]
        assert [v.shape for v in z.values()] == [(0,)] * 5
        assert [v.dtype for v in z.values()] == [np.int64, np.float64, np.float64, np.float32, object]
    # float16 intensity is computed in float32 and its extrema come back as float16
    t = _host(measure.regionprops_table(gpu.asarray(lab), gpu.asarray(inten.astype(np.float16)), properties=("max_intensity", "mean_intensity")))
    assert t["max_intensity"].dtype == np.float16 and t["max_intensity"].tolist() == [2.0, 4.0] and t["mean_intensity"].tolist() == [2.0, 4.0]


def test_strided_label_and_intensity_views(gpu, route):
    from cupyimg_amd.skimage import measure
    lab = cases.labels((37, 70), "smooth", np.int32)
    inten = cases.intensity((37, 70), np.uint8)
    props = ("label", "area", "bbox", "centroid", "moments", "weighted_moments", "max_intensity")
    got = _host(measure.regionprops_table(gpu.asarray(lab)[1::2, ::3], gpu.asarray(inten)[1::2, ::3], properties=props))
    want = ref.regionprops_table(lab[1::2, ::3], inten[1::2, ::3], properties=props)
    assert list(got) == list(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name


def test_launch_count_does_not_depend_on_the_number_of_regions(gpu, route):
    from cupyimg_amd.skimage import measure
    lib = _lib()
    few = np.zeros((64, 96), np.int32)
    few[2:9, 3:11], few[20:30, 40:70], few[50:60, 5:90] = 1, 2, 3
    many = np.arange(1, 3001, dtype=np.int32).repeat(2)[:64 * 96 - 144].reshape(-1)
    many = np.concatenate([many, np.zeros(64 * 96 - many.size, np.int32)]).reshape(64, 96)
    assert len(np.unique(few)) - 1 == 3 and len(np.unique(many)) - 1 == 3000
    inten = cases.intensity((64, 96), np.float32)
    counts = []
    for lab in (few, many):
        dl, di = gpu.asarray(lab), gpu.asarray(inten)
        before = lib.mi_debug_regionprops_launches() + lib.mi_debug_select_launches()
        t = measure.regionprops_table(dl, di, properties=cases.properties(2, True))
        counts.append(lib.mi_debug_regionprops_launches() + lib.mi_debug_select_launches() - before)
        assert t["label"].shape == (len(np.unique(lab)) - 1,)
    assert counts[0] == counts[1] and 0 < counts[0] <= 40, counts


# ------------------------------------------------------------------ remove_small_objects / remove_small_holes
@pytest.mark.parametrize("case", KAT["misc"], ids=[c["name"] for c in KAT["misc"]])
def test_remove_small_meets_the_known_answers(gpu, route, case):
    import warnings
    from cupyimg_amd.skimage import morphology
    image = np.array(case["image"], case["dtype"])
    dev = gpu.asarray(image)
    fn = getattr(morphology, case["fn"])
    if case["warns"]:
        with pytest.warns(UserWarning, match=case["warns"]):
            got = fn(dev, **case["kwargs"])
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = fn(dev, **case["kwargs"])
    want = np.array(case["expected"], case["expected_dtype"])
    assert got.dtype == want.dtype and np.array_equal(got.get(), want)
    assert got is not dev and np.array_equal(dev.get(), image)


@pytest.mark.parametrize("case", cases.ALL_LABEL_CASES, ids=[c[0] for c in cases.ALL_LABEL_CASES])
def test_remove_small_objects_is_the_transcription(gpu, route, case):
    import warnings
    from cupyimg_amd.skimage import morphology
    _, shape, kind, dtype = case
    lab = cases.labels(shape, kind, dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                  # "only one label" of the "full" cases
        if lab.min() < 0:
            with pytest.raises(ValueError, match="Negative value labels"):
                morphology.remove_small_objects(gpu.asarray(lab), 3)
            lab = np.where(lab > 0, lab, 0).astype(dtype)
        dev = gpu.asarray(lab)
        for min_size in (0, 1, 3, 50, lab.size + 1):
            got = morphology.remove_small_objects(dev, min_size)
            want = ref.remove_small_objects(lab, min_size)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.get(), want), min_size
        assert np.array_equal(dev.get(), lab)
        mask = lab > 0
        for conn in range(1, lab.ndim + 1):
            got = morphology.remove_small_objects(gpu.asarray(mask), 4, connectivity=conn)
            assert got.dtype == bool and np.array_equal(got.get(), ref.remove_small_objects(mask, 4, conn)), conn
            got = morphology.remove_small_holes(gpu.asarray(mask), 5, connectivity=conn)
            assert got.dtype == bool and np.array_equal(got.get(), ref.remove_small_holes(mask, 5, conn)), conn


def test_remove_small_in_place_and_views(gpu, route):
    import warnings
    from cupyimg_amd.skimage import morphology
    lab = cases.labels((37, 70), "noise", np.uint16)
    mask = lab > 0
    for arr, fn, rfn in ((lab, morphology.remove_small_objects, ref.remove_small_objects), (mask, morphology.remove_small_objects, ref.remove_small_objects),
                         (mask, morphology.remove_small_holes, ref.remove_small_holes)):
        dev = gpu.asarray(arr)
        assert fn(dev, 3, in_place=True) is dev and np.array_equal(dev.get(), rfn(arr, 3))
        base = gpu.asarray(arr)
        view = base[::2, 1::3]
        assert fn(view, 3, in_place=True) is view
        want = arr.copy()
        want[::2, 1::3] = rfn(arr[::2, 1::3], 3)
        assert np.array_equal(base.get(), want)                       # only the view's elements were written
        out = fn(gpu.asarray(arr)[::2, 1::3], 3)
        assert np.array_equal(out.get(), rfn(arr[::2, 1::3], 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        ints = (lab > 0).astype(np.int32) * 2
        dev = gpu.asarray(ints)
        assert morphology.remove_small_holes(dev, 3, in_place=True) is dev and dev.dtype == np.int32
        # the reference, step by step: an integer image negated in its own dtype is a 0 / 1 label image
        inv = (ints == 0).astype(np.int32)
        inv = ref.remove_small_objects(inv, 3)
        assert np.array_equal(dev.get(), (inv == 0).astype(np.int32))
    assert morphology.remove_small_objects(gpu.asarray(np.zeros((3, 0), bool))).shape == (3, 0)


# ------------------------------------------------------------------ dirty pool memory
DIRTY = [c for c in cases.TABLE_CASES if c[0] in ("kat-10x18", "noise-5x131", "odd-9x10x11", "noise-3x40x67")]


@pytest.mark.parametrize("case", DIRTY, ids=[c[0] for c in DIRTY])
def test_tables_do_not_depend_on_what_the_pool_hands_out(gpu, route, case):
    from cupyimg_amd.scipy import ndimage as ndi
    from cupyimg_amd.skimage import measure, morphology
    lab, inten = _inputs(case)
    dl = gpu.asarray(lab)
    di = None if inten is None else gpu.asarray(inten)
    pos = gpu.asarray(np.where(lab > 0, lab, 0).astype(lab.dtype))
    gpu.synchronize()
    props = cases.properties(lab.ndim, inten is not None)
    first = None
    import warnings
    for byte in dirty_pool.FILLS:
        with dirty_pool.pool_fill(gpu, byte), warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            table = _host(measure.regionprops_table(dl, di, properties=props))
            objects = ndi.find_objects(dl)
            kept = morphology.remove_small_objects(pos, 3).get()
            holes = morphology.remove_small_holes(pos, 3).get()
        check_table(table, case, inten is not None and inten.dtype.kind in "iu")
        if first is None:
            first = (table, objects, kept, holes)
            continue
        assert objects == first[1] and np.array_equal(kept, first[2]) and np.array_equal(holes, first[3])
        for name in table:
            if name.split("-")[0] in EXACT_PROPS:
                assert table[name].tobytes() == first[0][name].tobytes(), (name, byte)
    assert first[1] == sndi.find_objects(np.where(lab > 0, lab, 0))
    assert np.array_equal(first[2], ref.remove_small_objects(np.where(lab > 0, lab, 0).astype(lab.dtype), 3))


def test_zz_report_the_measured_ulp_distances(gpu):
    """not a check of its own: prints what the tests above measured, for DESIGN 4.18"""
    print("largest ulp distances to NumPy over this file's cases:", dict(sorted(MEASURED.items())))
    assert all(v <= ULP_BOUND for v in MEASURED.values())
