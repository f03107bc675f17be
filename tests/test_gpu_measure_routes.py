"""The labelled reductions (csrc/measure.hip) on both sides of every route switch, on wave-run layouts, at full size on
the LDS route, and the SciPy divergences fixed with them; judged against the host references of
tests/helpers/measure_ref.py (exact on integer-valued data)."""
import functools
import time

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import measure_ref as mr
from helpers import value_ranges as vr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ndi(gpu):
    from cupyimg_amd.scipy import ndimage
    return ndimage


def _dev(gpu, a):
    return gpu.asarray(np.ascontiguousarray(a))


def _host(r):
    return np.asarray(r.get() if hasattr(r, "get") else r)


def _exact_all(gpu, ndi, x, lab, index, funcs=("sum_labels", "mean", "minimum", "maximum", "minimum_position",
                                                 "maximum_position", "center_of_mass")):
    """every function in `funcs` equal to the host reference (integer-valued x: sums exact), with the route note"""
    ref = mr.Ref(x, lab, index)
    rows = ref.rows
    xd, ld = _dev(gpu, x), (None if lab is None else _dev(gpu, lab))
    idx = index if not isinstance(index, np.ndarray) else gpu.asarray(index.astype(np.int64))
    notes = {}
    s, _, exact, _, _ = ref.sums()
    assert exact
    mn, mx, pmn, pmx, _ = ref.extrema(nan_min_propagates=mr.index_form(index) != "seq")
    for fn in funcs:
        got = getattr(ndi, fn)(xd, ld, idx)
        notes[fn] = gpu.last_kernel()
        if fn == "sum_labels":
            np.testing.assert_array_equal(_host(got).ravel(), s[rows], err_msg=fn)
        elif fn == "mean":
            np.testing.assert_array_equal(_host(got).ravel(), ref.mean()[0][rows], err_msg=fn)
        elif fn in ("variance", "standard_deviation"):
            r, b = ref.variance() if fn == "variance" else ref.std()
            assert mr.ratio(_host(got).ravel(), r[rows], b[rows]) <= 1.0, fn
        elif fn == "minimum":
            np.testing.assert_array_equal(_host(got).ravel(), mn[rows], err_msg=fn)
        elif fn == "maximum":
            np.testing.assert_array_equal(_host(got).ravel(), mx[rows], err_msg=fn)
        elif fn in ("minimum_position", "maximum_position"):
            p = (pmn if fn == "minimum_position" else pmx)[rows]
            want = [tuple(int(c) for c in np.unravel_index(int(q), x.shape)) for q in p]
            assert (got if isinstance(got, list) else [got]) == want, fn
        elif fn == "center_of_mass":
            c, _ = ref.com()
            g = np.asarray(got if isinstance(got, list) else [got], np.float64)
            np.testing.assert_array_equal(g, c[rows], err_msg=fn)
    return notes


def _runs_labels(n, K, seed, lengths=(1, 2, 3, 63, 64, 65, 255, 256, 257)):
    rng = np.random.default_rng(seed)
    out = np.empty(n, np.int64)
    i = 0
    while i < n:
        L = int(rng.choice(lengths))
        out[i:i + L] = int(rng.integers(1, K + 1))
        i += L
    return out


# ------------------------------------------------------------------ route table
@pytest.mark.parametrize("K,route", [(1024, "LDS atomics"), (1025, "global atomics")])
def test_route_lds_slots(gpu, ndi, K, route):
    """kLdsSlots = 1024: sums, variance and extrema through LDS up to 1024 slots, through global atomics above"""
    n = 300007
    lab = _runs_labels(n, K, K)
    lab[:K] = np.arange(1, K + 1)                       # every slot present
    x = np.random.default_rng(1).integers(-3000, 3000, n).astype(np.float64)
    index = np.arange(1, K + 1)
    notes = _exact_all(gpu, ndi, x, lab, index, ("sum_labels", "variance", "minimum", "maximum_position"))
    other = "global atomics" if route == "LDS atomics" else "LDS atomics"
    for fn in ("sum_labels", "variance", "minimum"):
        assert route in notes[fn] and other not in notes[fn] and "lut" in notes[fn], (fn, notes[fn])
    assert "M_SSD" in notes["variance"] and "M_POS" in notes["maximum_position"]


@pytest.mark.parametrize("shape,K,route", [((40, 60, 130), 682, "LDS atomics"), ((40, 60, 130), 683, "global atomics"),
                                           ((500, 613), 1024, "LDS atomics"), ((500, 613), 1025, "global atomics")])
def test_route_center_of_mass_slots(gpu, ndi, shape, K, route):
    """center_of_mass uses LDS while slots x ndim <= kLdsCom = 2048"""
    n = int(np.prod(shape))
    lab = _runs_labels(n, K, K + len(shape)).reshape(shape)
    lab.ravel()[:K] = np.arange(1, K + 1)
    x = np.random.default_rng(2).integers(0, 4096, shape).astype(np.int32)
    notes = _exact_all(gpu, ndi, x, lab, list(range(1, K + 1)), ("center_of_mass",))
    assert "M_COM" in notes["center_of_mass"] and route in notes["center_of_mass"], notes


@pytest.mark.parametrize("extra,route", [(65535, "lut"), (65536, "search")])
def test_route_lut_vs_search(gpu, ndi, extra, route):
    """a lookup table while imax - imin < 4 K + 65536, binary search from there on (index with a duplicate)"""
    K = 40
    vals = [100 + i for i in range(K - 2)] + [100 + 4 * K + extra]
    index = vals[:K // 2] + [vals[-1], vals[3]] + vals[K // 2:-1]     # K entries, one duplicate
    assert len(index) == K and max(index) - min(index) == 4 * K + extra
    n = 200003
    rng = np.random.default_rng(3)
    lab = np.asarray(vals, np.int64)[rng.integers(0, len(vals), n)]
    x = rng.integers(-1024, 3072, n).astype(np.int16)
    for form in (index, np.asarray(index)):
        notes = _exact_all(gpu, ndi, x, lab, form)
        for fn, note in notes.items():
            assert route in note, (fn, note)


# ------------------------------------------------------------------ wave-run layouts
def _layouts():
    out = {}
    for L in (1, 2, 63, 64, 65, 255, 256, 257):
        n = 64 * 97 + 13
        out["runs%d" % L] = (np.arange(n) // L) % 7 + 1
    n = 64 * 300 + 5
    lab = np.full(n, 3)
    lab[63::64] = 5                                     # one-voxel runs on lane 63
    lab[63 + 128::256] = 4                              # runs starting on lane 63 and crossing into the next wave
    lab[64 + 128::256] = 4
    out["lane63"] = lab
    n = 64 * 200 + 31
    alt = np.where(np.arange(n) % 2 == 0, 2, 99)        # present / absent on alternating lanes (99 not in the index)
    alt[::3] = 1
    out["alternating"] = alt
    out["whole"] = np.ones(64 * 1000 + 17, np.int64)    # one slot covering the whole array
    out["n1"] = np.ones(1, np.int64)
    out["n1000"] = (np.arange(1000) // 37) % 5 + 1
    out["n257"] = np.full(257, 2)
    # the grid-stride step is 256 x 16 x (CUs): runs straddling every multiple of 256 x 16 x 32 up to 2**22, the step
    # of any device whose CU count is a multiple of 32
    n = (1 << 22) + 4099
    g = (np.arange(n) + 5) // 11 % 6 + 1
    for step in range(256 * 16 * 32, n, 256 * 16 * 32):
        g[step - 70:step + 70] = 6
    out["grid_stride"] = g
    return out


@pytest.mark.parametrize("name", sorted(_layouts()))
@pytest.mark.parametrize("many", [False, True])
def test_wave_run_layouts(gpu, ndi, name, many):
    """sums, counts (mean), extrema, positions, centres and histograms exact on label streams built to hit every
    boundary of the segmented wave reduction; `many`: 1500 index values (global atomics) instead of a few (LDS)"""
    lab = _layouts()[name]
    n = lab.size
    x = ((np.arange(n) * 7919) % 4001 - 2000).astype(np.float32)
    index = list(range(1, 8)) if not many else list(range(1, 1501))
    notes = _exact_all(gpu, ndi, x, lab, index)
    want = "global atomics" if many else "LDS atomics"
    assert want in notes["sum_labels"], notes["sum_labels"]
    edges_kw = dict(min=-2000, max=2000, bins=97)
    got = ndi.histogram(_dev(gpu, x), edges_kw["min"], edges_kw["max"], edges_kw["bins"], _dev(gpu, lab), index[:9])
    ref = mr.Ref(x, lab, index[:9])
    h, present = ref.histogram(np.linspace(-2000, 2000, 98))
    for k, g in zip(ref.rows, got):
        if present[k]:
            np.testing.assert_array_equal(g.get(), h[k])
        else:
            assert g is None
    # no index: the one region of labels > 0
    np.testing.assert_array_equal(_host(ndi.sum_labels(_dev(gpu, x), _dev(gpu, lab))), x[lab > 0].astype(np.float64).sum())


# ------------------------------------------------------------------ full size, LDS route
@functools.lru_cache(maxsize=None)
def _volume(kind, n):
    """the 512^3 test volumes, generated once per module (read-only)"""
    x = vr.ct_hu((n,) * 3, 3) if kind == "ct_i16" else vr.mr_u12((n,) * 3, 4, dtype=np.float32) if kind == "mr_f32" \
        else vr.offset_1e4((n,) * 3, 5)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def _organs(n, nlab, seed):
    """organ-like label map: a coarse random grid of labels 0 .. nlab blown up to n^3 (nearest), ~1/8 background"""
    cells = 8 if nlab <= 6 else 16
    rng = np.random.default_rng(seed)
    small = rng.integers(1, nlab + 1, (cells,) * 3).astype(np.int32)
    small[rng.random(small.shape) < 0.125] = 0
    small.ravel()[:nlab] = np.arange(1, nlab + 1)       # every label present
    r = n // cells
    lab = small.repeat(r, 0).repeat(r, 1).repeat(r, 2)
    lab.flags.writeable = False
    return lab


def _bincount_refs(x, lab, K):
    fl = lab.ravel()
    v = x.ravel().astype(np.float64)
    cnt = np.bincount(fl, minlength=K + 1)[1:]
    s = np.bincount(fl, weights=v, minlength=K + 1)[1:]
    a = np.bincount(fl, weights=np.abs(v), minlength=K + 1)[1:]
    return v, cnt, s, a


@pytest.mark.parametrize("kind", ["ct_i16", "mr_f32"])
@pytest.mark.parametrize("nlab", [6, 1000])
def test_full_size_lds_route(gpu, ndi, kind, nlab):
    from cupyimg_amd.scipy.ndimage import measurements as meas
    n = 512
    shape = (n,) * 3
    x = _volume(kind, n)
    lab = _organs(n, nlab, nlab)
    xd, ld = _dev(gpu, x), _dev(gpu, lab)
    index = gpu.asarray(np.arange(1, nlab + 1, dtype=np.int64))
    v, cnt, s, a = _bincount_refs(x, lab, nlab)
    assert np.all(a < 2.0 ** 53)                        # integer data: float64 sums are exact
    np.testing.assert_array_equal(ndi.sum_labels(xd, ld, index).get(), s)
    assert "LDS atomics" in gpu.last_kernel() and "lut" in gpu.last_kernel(), gpu.last_kernel()
    np.testing.assert_array_equal(ndi.mean(xd, ld, index).get(), s / cnt)
    fl = lab.ravel()
    m = s / cnt
    d = v - np.concatenate([[0.0], m])[fl]
    D = np.bincount(fl, weights=d * d, minlength=nlab + 1)[1:]
    var = D / cnt
    k = cnt + 8.0
    bound = (k + 4 + cnt + 3) * mr.U * var                 # device bound plus the float64 bincount's own error
    assert mr.ratio(ndi.variance(xd, ld, index).get(), var, bound) <= 1.0
    com = meas._reduce(meas._OPS["com"], xd, ld, index)[0].get()
    assert "LDS atomics" in gpu.last_kernel() if nlab * 3 <= 2048 else "global atomics" in gpu.last_kernel()
    for dax in range(3):
        c = np.broadcast_to(np.arange(n, dtype=np.float64).reshape([-1 if j == dax else 1 for j in range(3)]), shape).ravel()
        T = np.bincount(fl, weights=v * c, minlength=nlab + 1)[1:]
        np.testing.assert_array_equal(com[:, dax], T / s)
        del c
    t0 = time.perf_counter()
    out, pos = meas._reduce(meas._OPS["extrema"], xd, ld, index, positions=True)[:2]
    out, pos = out.get(), pos.get()
    t_ext = time.perf_counter() - t0
    sel = fl > 0
    for col, ufunc, init in ((0, np.minimum, np.inf), (1, np.maximum, -np.inf)):
        ext = np.full(nlab + 1, init)
        ufunc.at(ext, fl[sel], v[sel])
        np.testing.assert_array_equal(out[:, col], ext[1:].astype(x.dtype))
        hit = np.flatnonzero(sel & (v == ext[fl]))
        labs, first = np.unique(fl[hit], return_index=True)
        assert labs.size == nlab
        np.testing.assert_array_equal(pos[:, col], hit[first])
        ties = np.bincount(fl[hit], minlength=nlab + 1)[1:]
        if col == 0 and kind == "ct_i16":
            print("extrema + positions, %d labels, up to %d tied minima per label: %.1f ms" % (nlab, ties.max(), t_ext * 1e3))
    hist = ndi.histogram(xd, -1024, 3071, 4096, ld, index)
    edges = np.linspace(-1024, 3071, 4097)
    b = np.searchsorted(edges, v, side="right") - 1
    b[v == edges[-1]] = 4095
    ok = sel & (v >= edges[0]) & (v <= edges[-1])
    h = np.bincount(fl[ok].astype(np.int64) * 4096 + b[ok], minlength=(nlab + 1) * 4096).reshape(nlab + 1, 4096)[1:]
    got = np.stack([r.get() for r in hist])
    np.testing.assert_array_equal(got, h)


def test_full_size_variance_offset_1e4(gpu, ndi):
    """two-pass variance of 1e4 + N(0, 1) per organ: the bound scales with the spread, not with 1e4"""
    n = 512
    x = _volume("offset_1e4", n)
    lab = _organs(n, 6, 6)
    v, cnt, s, a = _bincount_refs(x, lab, 6)
    fl = lab.ravel()
    m = s / cnt
    d = v - np.concatenate([[0.0], m])[fl]
    var = np.bincount(fl, weights=d * d, minlength=7)[1:] / cnt
    em = (2 * cnt + 8) * mr.U * a / cnt + mr.U * np.abs(m)   # the mean's error: device and reference sums
    bound = (2 * cnt + 15) * mr.U * var + em ** 2 * 2
    got = ndi.variance(_dev(gpu, x), _dev(gpu, lab), list(range(1, 7)))
    assert "LDS atomics" in gpu.last_kernel()
    assert mr.ratio(_host(got), var, bound) <= 1.0
    assert np.all(np.abs(var - 1.0) < 0.01)


# ------------------------------------------------------------------ regressions: divergences from SciPy 1.15
def test_signed_zero_extrema_positions(gpu, ndi):
    """-0.0 and +0.0 are one value: the position of the first of them"""
    a = np.array([0.0, -0.0, 1.0])
    b = np.array([-0.0, 0.0, -1.0])
    assert ndi.minimum_position(_dev(gpu, a)) == (0,) == tuple(sndi.minimum_position(a))
    assert ndi.maximum_position(_dev(gpu, b)) == (0,) == tuple(sndi.maximum_position(b))
    lab = np.array([1, 1, 1])
    assert ndi.minimum_position(_dev(gpu, a), _dev(gpu, lab), 1) == (0,)
    assert ndi.maximum_position(_dev(gpu, b), _dev(gpu, lab), 1) == (0,)
    for dt in (np.float32, np.float64):
        big = np.ones(1000, dt)
        big[3], big[7] = 0.0, -0.0                     # +0.0 first: ordering -0.0 below it would answer (7,)
        mn, mx, pmn, pmx = ndi.extrema(_dev(gpu, big), _dev(gpu, np.ones(1000, np.int32)), [1])
        assert pmn == [(3,)] and float(_host(mn)[0]) == 0.0


def test_uint64_labels_without_index(gpu, ndi):
    """labels of 2**63 and more are positive: SciPy keeps labels > 0"""
    x = np.arange(4.0)
    lab = np.array([0, 1, 2 ** 63 + 1, 2 ** 64 - 1], np.uint64)
    xd, ld = _dev(gpu, x), _dev(gpu, lab)
    assert float(_host(ndi.sum_labels(xd, ld))) == 6.0 == sndi.sum_labels(x, lab)
    assert float(_host(ndi.mean(xd, ld))) == 2.0
    assert float(_host(ndi.maximum(xd, ld))) == 3.0
    assert float(_host(ndi.minimum(xd, ld))) == 1.0
    assert "nonzero" in gpu.last_kernel()
    np.testing.assert_array_equal(_host(ndi.histogram(xd, 0, 4, 4, ld)), sndi.histogram(x, 0, 4, 4, lab))
    # a negative index value names no uint64 label (as int64 it would equal 2**64 - 1)
    np.testing.assert_array_equal(_host(ndi.sum_labels(xd, ld, [-1, 1])), [0.0, 1.0])
    np.testing.assert_array_equal(_host(ndi.sum_labels(xd, ld, [2 ** 64 - 1, 1, 2 ** 63 + 1])), [3.0, 1.0, 2.0])
    np.testing.assert_array_equal(_host(ndi.sum_labels(xd, ld, np.array([-1, 1]))), sndi.sum_labels(x, lab, [-1, 1]))
    np.testing.assert_array_equal(_host(ndi.sum_labels(xd, ld, gpu.asarray(np.array([-1, 1])))), [0.0, 1.0])


def test_histogram_min_above_max_raises(gpu, ndi):
    x = np.arange(4.0)
    with pytest.raises(ValueError):
        sndi.histogram(x, 3, 1, 4)
    with pytest.raises(ValueError):
        ndi.histogram(_dev(gpu, x), 3, 1, 4)
    lab = np.array([1, 1, 2, 2])
    with pytest.raises(ValueError):
        ndi.histogram(_dev(gpu, x), 3, 1, 4, _dev(gpu, lab), [1, 7])
    assert ndi.histogram(_dev(gpu, x), 3, 1, 4, _dev(gpu, lab), [7]) == [None] == sndi.histogram(x, 3, 1, 4, lab, [7])


def test_float16_extrema_dtype(gpu, ndi):
    h = np.array([1, 2, 3], np.float16)
    for fn in ("minimum", "maximum"):
        got = getattr(ndi, fn)(_dev(gpu, h))
        assert got.dtype == np.float16 and got.dtype == np.asarray(getattr(sndi, fn)(h)).dtype
    mn, mx, _, _ = ndi.extrema(_dev(gpu, h), _dev(gpu, np.array([1, 1, 2])), [1, 2])
    assert mn.dtype == mx.dtype == np.float16
    np.testing.assert_array_equal(mx.get(), np.array([2, 3], np.float16))


def test_nan_minimum_without_index(gpu, ndi):
    """no index or a scalar one: SciPy's minimum is NaN where the region holds a NaN (a sequence index skips NaN)"""
    x = np.array([3.0, np.nan, 1.0, np.nan, 5.0])
    lab = np.array([1, 1, 1, 1, 2])
    assert np.isnan(float(_host(ndi.minimum(_dev(gpu, x))))) and np.isnan(sndi.minimum(x))
    assert np.isnan(float(_host(ndi.minimum(_dev(gpu, x), _dev(gpu, lab), 1)))) and np.isnan(sndi.minimum(x, lab, 1))
    assert float(_host(ndi.minimum(_dev(gpu, x), _dev(gpu, lab), 2))) == 5.0
    np.testing.assert_array_equal(_host(ndi.minimum(_dev(gpu, x), _dev(gpu, lab), [1, 2])), sndi.minimum(x, lab, [1, 2]))
    mn, mx, _, _ = ndi.extrema(_dev(gpu, x.astype(np.float32)))
    assert np.isnan(float(_host(mn))) and np.isnan(float(_host(mx)))


def test_device_index_beyond_2_53(gpu, ndi):
    """a device index whose values doubles cannot hold: the lookup table spans the exact range"""
    base = 2 ** 60
    lab = np.array([base + 1, base + 3, base + 3, base + 200, 5], np.int64)
    x = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    idx = np.array([base + 3, base + 1, base + 200, base + 2], np.int64)
    got = ndi.sum_labels(_dev(gpu, x), _dev(gpu, lab), gpu.asarray(idx))
    np.testing.assert_array_equal(got.get(), [6.0, 1.0, 8.0, 0.0])
    np.testing.assert_array_equal(got.get(), sndi.sum_labels(x, lab, idx))


def test_scipy_result_forms_found_by_fuzzing(gpu, ndi):
    """found by `fuzz_vs_scipy.py --measure`: SciPy raises on the extrema of an empty region with no index or a scalar
    one; histogram answers a sequence index with an object array and refuses index values the labels' dtype cannot
    hold"""
    x = np.array([4.0, 1.0, 7.0, 2.0])
    lab = np.array([1, 1, 2, 0], np.uint8)
    xd, ld = _dev(gpu, x), _dev(gpu, lab)
    for fn in ("minimum", "maximum", "minimum_position", "maximum_position", "extrema"):
        with pytest.raises(ValueError):
            getattr(sndi, fn)(x, lab, 9)
        with pytest.raises(ValueError):
            getattr(ndi, fn)(xd, ld, 9)
        with pytest.raises(ValueError):
            getattr(ndi, fn)(xd, _dev(gpu, np.zeros(4, np.int32)))          # no label > 0
    assert ndi.maximum_position(xd, ld, [9, 2]) == [(0,), (2,)]              # an absent entry of a sequence: (0,)
    got = ndi.histogram(xd, 0, 8, 4, ld, [1, 9])
    ref = sndi.histogram(x, 0, 8, 4, lab, [1, 9])
    assert isinstance(got, np.ndarray) and got.dtype == object and got.shape == ref.shape == (2,)
    np.testing.assert_array_equal(got[0].get(), ref[0])
    assert got[1] is None and ref[1] is None
    with pytest.raises(ValueError):
        sndi.histogram(x, 0, 8, 4, lab, [1, -1])
    with pytest.raises(ValueError):
        ndi.histogram(xd, 0, 8, 4, ld, [1, -1])


def test_plain_extrema_take_no_position_pass(gpu, ndi):
    """minimum / maximum with no index or a scalar one learn whether the region is empty from the extrema pass: the
    position pass (one atomic per voxel tied at the extreme) runs only for the position functions and extrema()"""
    x = vr.ct_hu((64, 96, 96), 3)                     # the padding value is the minimum of many voxels
    lab = (np.arange(x.size).reshape(x.shape) % 3).astype(np.int32)
    xd, ld = _dev(gpu, x), _dev(gpu, lab)
    for call in (lambda: ndi.minimum(xd), lambda: ndi.maximum(xd, ld), lambda: ndi.minimum(xd, ld, 2)):
        call()
        assert "M_EXT" in gpu.last_kernel() and "M_POS" not in gpu.last_kernel(), gpu.last_kernel()
    assert int(_host(ndi.minimum(xd, ld, 2))) == int(x[lab == 2].min())
    with pytest.raises(ValueError):
        ndi.maximum(xd, ld, 7)
    ndi.minimum_position(xd, ld, 2)
    assert "M_POS" in gpu.last_kernel()


def test_unmatched_index_entries_are_absent_rows(gpu, ndi):
    """index values no label can hold (negative for uint64 labels) are left out of the reduction and answered as
    absent, without reading the labels back"""
    x = np.arange(6.0)
    lab = np.array([0, 1, 2 ** 63 + 1, 2 ** 64 - 1, 5, 5], np.uint64)
    xd, ld = _dev(gpu, x), _dev(gpu, lab)
    for idx in ([-1, 5, -7, 1], np.array([-1, 5, -7, 1]), gpu.asarray(np.array([-1, 5, -7, 1]))):
        np.testing.assert_array_equal(_host(ndi.sum_labels(xd, ld, idx)), [0.0, 9.0, 0.0, 1.0])
        np.testing.assert_array_equal(_host(ndi.mean(xd, ld, idx)), [np.nan, 4.5, np.nan, 1.0])
        np.testing.assert_array_equal(_host(ndi.maximum(xd, ld, idx)), [0.0, 5.0, 0.0, 1.0])
        assert ndi.maximum_position(xd, ld, idx) == [(0,), (5,), (0,), (1,)]
    # histogram follows SciPy's labeled_comprehension, which converts the index to the labels' dtype first
    for idx in ([-1, 5, -7], np.array([-1, 5, -7]), gpu.asarray(np.array([-1, 5, -7]))):
        h = ndi.histogram(xd, 0, 6, 3, ld, idx)
        r = sndi.histogram(x, 0, 6, 3, lab, [-1, 5, -7])
        assert len(h) == len(r) == 3 and h[2] is None and r[2] is None
        np.testing.assert_array_equal(h[0].get(), r[0])
        np.testing.assert_array_equal(h[1].get(), r[1])
    assert float(_host(ndi.sum_labels(xd, ld, -1))) == 0.0 == sndi.sum_labels(x, lab, -1)
    with pytest.raises(ValueError):
        ndi.minimum(xd, ld, -1)
    with pytest.raises(ValueError):
        sndi.minimum(x, lab, -1)
