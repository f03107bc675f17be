"""Device compaction (count_nonzero, flatnonzero, nonzero, argwhere), gather (take) and the stable radix sort (argsort, sort)
against NumPy, exact, under both settings of mi_debug_set_select: the planner's tiles, and tiles of 64 elements with scan
blocks of 64 entries, where a few thousand elements span many tiles and more than one level of the scan."""
import ctypes

import numpy as np
import pytest

from helpers import dirty_pool

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097, 70001)
SHAPES = ((7, 9), (5, 6, 7), (2, 3, 4, 5))
DTYPES = ("bool", "uint8", "int16", "int32", "int64", "float32", "float64")
DENSITIES = ("none", "all", "first", "last", "1%", "50%")


@pytest.fixture(params=[0, 1], ids=["planner-tiles", "small-tiles"])
def tiles(request, gpu):
    from cupyimg_amd import _lib
    lib = _lib.load()
    lib.mi_debug_set_select.argtypes = [ctypes.c_int]
    assert lib.mi_debug_set_select(request.param) == 0
    try:
        yield 64 if request.param else None
    finally:
        lib.mi_debug_set_select(0)


def _selected(shape, dtype, density, seed=0):
    """an array of `dtype` whose nonzero elements follow `density`; floats get NaN among the nonzero and -0.0 among the zero"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if density == "none":
        mask = np.zeros(n, bool)
    elif density == "all":
        mask = np.ones(n, bool)
    elif density in ("first", "last"):
        mask = np.zeros(n, bool)
        if n:
            mask[0 if density == "first" else -1] = True
    else:
        mask = rng.random(n) < (0.01 if density == "1%" else 0.5)
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        a = mask.copy()
    elif dtype.kind == "f":
        a = np.where(mask, rng.standard_normal(n) + 3.0, 0.0).astype(dtype)
        nz, z = np.flatnonzero(mask), np.flatnonzero(~mask)
        a[nz[::5]] = np.nan
        a[z[::3]] = -0.0
    else:
        a = np.where(mask, rng.integers(1, 100, size=n), 0).astype(dtype)
        if dtype.kind == "i":
            a[np.flatnonzero(mask)[::2]] *= -1
    return a.reshape(shape)


def _check_compaction(gpu, a, tiles):
    d = gpu.asarray(a)
    want = np.flatnonzero(a)
    assert gpu.count_nonzero(d) == want.size
    if a.size:
        assert "sel_count_kernel<nonzero,{}>".format(a.dtype) in gpu.last_kernel()
        assert "tile={} ".format(tiles or 2048) in gpu.last_kernel()
    got = gpu.flatnonzero(d)
    assert got.dtype == np.int64 and np.array_equal(got.get(), want)
    if a.size and want.size:
        assert "sel_write_kernel<nonzero,{}> tile={} ".format(a.dtype, tiles or 2048) in gpu.last_kernel()
    if a.ndim:
        got = gpu.argwhere(d)
        assert got.dtype == np.int64 and got.shape == (want.size, a.ndim) and np.array_equal(got.get(), np.argwhere(a))
        got = gpu.nonzero(d)
        assert isinstance(got, tuple) and len(got) == a.ndim
        for g, w in zip(got, np.nonzero(a)):
            assert g.dtype == np.int64 and np.array_equal(g.get(), w)
    assert np.array_equal(d.get(), a, equal_nan=a.dtype.kind == "f")           # the input comes back unchanged


@pytest.mark.parametrize("density", DENSITIES)
def test_compaction_sizes_and_densities(gpu, tiles, density):
    for k, n in enumerate(SIZES):
        _check_compaction(gpu, _selected((n,), DTYPES[k % len(DTYPES)], density, seed=k), tiles)


@pytest.mark.parametrize("dtype", DTYPES)
def test_compaction_dtypes_and_shapes(gpu, tiles, dtype):
    for k, shape in enumerate(SHAPES + ((4097,), (70001,))):
        _check_compaction(gpu, _selected(shape, dtype, "50%" if k % 2 else "1%", seed=10 + k), tiles)


def test_compaction_of_a_strided_view(gpu, tiles):
    a = _selected((40, 66), "float32", "50%", seed=3)
    d = gpu.asarray(a)
    for view, host in ((d[::2, 1::3], a[::2, 1::3]), (d.T, a.T), (d[5:, ::-1], a[5:, ::-1])):
        assert not view.flags.c_contiguous
        assert np.array_equal(gpu.flatnonzero(view).get(), np.flatnonzero(host))
        assert np.array_equal(gpu.argwhere(view).get(), np.argwhere(host))
        assert gpu.count_nonzero(view) == np.count_nonzero(host)


def test_take_and_its_index_error(gpu, tiles):
    rng = np.random.default_rng(5)
    for dtype in DTYPES:
        a = _selected((5, 6, 7), dtype, "50%", seed=6)
        idx = rng.integers(-a.size, a.size, size=333)
        got = gpu.take(gpu.asarray(a), gpu.asarray(idx))
        assert got.dtype == a.dtype and np.array_equal(got.get(), np.take(a, idx), equal_nan=a.dtype.kind == "f")
        assert "take_kernel<{}>".format(a.dtype) in gpu.last_kernel()
    a = np.arange(100, dtype=np.float32)
    d = gpu.asarray(a)
    assert gpu.take(d, gpu.asarray(np.zeros(0, np.int64))).shape == (0,)
    assert np.array_equal(gpu.take(d, gpu.asarray(np.array([[99, -100], [0, -1]]))).get(), np.take(a, [[99, -100], [0, -1]]))
    for bad in (100, -101, 2 ** 40, -2 ** 62):
        with pytest.raises(IndexError):
            gpu.take(d, gpu.asarray(np.array([3, bad, 5], dtype=np.int64)))
    assert np.array_equal(gpu.take(d, gpu.asarray(np.array([3, 5]))).get(), [3.0, 5.0])         # and the device still answers
    assert np.array_equal(d.get(), a)


def _sort_data(n, dtype, kind, seed):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        a = rng.random(n) < 0.5
    elif kind == "ties":
        a = rng.integers(0, 3, size=n).astype(dtype)
        if dtype.kind != "u":
            a = a - np.asarray(1, dtype)
    elif dtype.kind == "f":
        a = rng.standard_normal(n).astype(dtype)
        a[rng.random(n) < 0.05] = 0.0
    else:
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    if dtype.kind == "f" and n:
        specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, np.nan], dtype)
        where = rng.permutation(n)[:specials.size]
        a[where] = specials[:where.size]
    if kind == "sorted":
        a = np.sort(a, kind="stable")
    elif kind == "reversed":
        a = np.sort(a, kind="stable")[::-1].copy()
    return a.astype(dtype)


def _check_sort(gpu, a, tiles):
    d = gpu.asarray(a)
    isf = a.dtype.kind == "f"
    got = gpu.argsort(d)
    assert got.dtype == np.int64 and got.shape == a.shape
    assert np.array_equal(got.get(), np.argsort(a, kind="stable"))
    if a.size:
        note = gpu.last_kernel()
        assert "sort_scatter_kernel<{},ascending>".format(a.dtype) in note, note
        if tiles:
            assert "tile=64 " in note and "scan_block=64" in note, note
        else:
            assert "tile=4096 " in note and "scan_block=1024" in note, note
    with np.errstate(over="ignore"):
        negated = ~a if a.dtype == np.bool_ else -a
    assert np.array_equal(gpu.argsort(d, descending=True).get(), np.argsort(negated, kind="stable"))
    got = gpu.sort(d)
    assert got.dtype == a.dtype and np.array_equal(got.get(), np.sort(a, kind="stable"), equal_nan=isf)
    assert np.array_equal(d.get(), a, equal_nan=isf)


@pytest.mark.parametrize("dtype", DTYPES)
def test_argsort_and_sort_sizes(gpu, tiles, dtype):
    for k, n in enumerate(SIZES):
        _check_sort(gpu, _sort_data(n, dtype, "random", 20 + k), tiles)


@pytest.mark.parametrize("kind", ("ties", "sorted", "reversed"))
def test_argsort_ties_sorted_and_reversed(gpu, tiles, kind):
    for k, dtype in enumerate(DTYPES):
        for n in (257, 4097):
            _check_sort(gpu, _sort_data(n, dtype, kind, 40 + k), tiles)


def test_nan_signs_zero_signs_and_infinities(gpu, tiles):
    a = np.array([np.nan, 1.0, -0.0, 0.0, -np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -1.0], np.float32)
    a = np.concatenate([a, a[::-1], a])
    _check_sort(gpu, a, tiles)
    _check_sort(gpu, a.astype(np.float64), tiles)
    order = gpu.argsort(gpu.asarray(a)).get()
    nans = order[-9:]
    assert np.isnan(a[nans]).all() and np.array_equal(nans, np.sort(nans))                  # every NaN last, in the original order
    zeros = order[a[order] == 0]
    assert np.array_equal(zeros, np.sort(zeros))                                            # -0.0 and +0.0 are one key


def test_refusals(gpu, tiles):
    with pytest.raises(TypeError):
        gpu.argsort(gpu.asarray(np.zeros(4, np.float16)))
    with pytest.raises(TypeError):
        gpu.flatnonzero(gpu.asarray(np.zeros(4, np.float16)))
    with pytest.raises(ValueError):
        gpu.argsort(gpu.asarray(np.zeros((3, 4), np.float32)))
    with pytest.raises(IndexError):
        gpu.take(gpu.asarray(np.zeros(0, np.float32)), gpu.asarray(np.array([0])))


@pytest.mark.parametrize("byte", dirty_pool.FILLS)
def test_every_entry_on_a_poisoned_pool(gpu, tiles, byte):
    """the work block, the histograms, the scan tables and the pair buffers come from the pool uninitialised"""
    a = _selected((37, 71), "float32", "50%", seed=7)
    keys = _sort_data(4097, "float32", "random", 8)
    idx = np.random.default_rng(9).integers(0, a.size, size=100)
    d, dk, di = gpu.asarray(a), gpu.asarray(keys), gpu.asarray(idx)
    gpu.synchronize()
    with dirty_pool.pool_fill(gpu, byte):
        assert gpu.count_nonzero(d) == np.count_nonzero(a)
        assert np.array_equal(gpu.flatnonzero(d).get(), np.flatnonzero(a))
        assert np.array_equal(gpu.argwhere(d).get(), np.argwhere(a))
        for g, w in zip(gpu.nonzero(d), np.nonzero(a)):
            assert np.array_equal(g.get(), w)
        assert np.array_equal(gpu.take(d, di).get(), np.take(a, idx), equal_nan=True)
        assert np.array_equal(gpu.argsort(dk).get(), np.argsort(keys, kind="stable"))
        assert np.array_equal(gpu.argsort(dk, descending=True).get(), np.argsort(-keys, kind="stable"))
        assert np.array_equal(gpu.sort(dk).get(), np.sort(keys, kind="stable"), equal_nan=True)
