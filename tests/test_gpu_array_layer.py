"""The array layer against NumPy: the 12 x 12 cast matrix of `mi_copy` (contiguous, strided, into a view), its
round-half-even form, strided copies at ranks 0 to 8, the grid-stride loops beyond the launch cap, fills, basic
indexing and assignment (overlapping assignments included), `shares_memory` and `arrays_differ`.

Inputs and expectations come from tests/helpers/array_cases.py (held against NumPy by tests/test_array_cases_yardstick.py).
Floats are compared bit for bit with NaNs by place (`ac.same`), everything else with np.array_equal."""
import ctypes

import numpy as np
import pytest

from helpers import array_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core(gpu):
    from cupyimg_amd import core
    assert tuple(core._DTYPE_CODES) == ac.DTYPES
    return core


def _mi_copy(core, src, dst, rhe=0):
    from cupyimg_amd import _lib
    a, b = src._desc(), dst._desc()
    _lib.check(_lib.load().mi_copy(ctypes.byref(a), ctypes.byref(b), int(rhe), None))


def _sentinel(n, dtype):
    """host array no copy is expected to produce by accident: bytes 0xA5 (bool: True)"""
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        return np.ones(n, bool)
    return np.full(n * dtype.itemsize, 0xA5, np.uint8).view(dtype)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _dev(gpu, host):
    """device copy of a host array of any rank (asarray makes a 0-d input one-dimensional: index it back)"""
    host = np.asarray(host)
    return gpu.asarray(host.reshape(1))[0] if host.ndim == 0 else gpu.asarray(host)


_SOURCES = {}


def _source_values(dtype):
    if dtype not in _SOURCES:
        _SOURCES[dtype] = ac.f16_all() if dtype == np.float16 else ac.ladder(dtype)
    return _SOURCES[dtype]


# ---------------------------------------------------------------- cast matrix
@pytest.mark.parametrize("src", ac.DTYPES, ids=str)
def test_cast_matrix(gpu, core, src):
    vals = _source_values(src)
    for dst in ac.DTYPES:
        v = vals[ac.admitted(vals, dst)]
        want = ac.expected_cast(v, dst)
        n = v.size
        # contiguous: copy_linear, or the memcpy when the types agree
        got = gpu.asarray(v).astype(dst).get()
        assert ac.same(got, want), "contiguous {} -> {}: {} of {} differ, first at value {!r}".format(
            src, dst, *_first_difference(got, want, v))
        # strided on both sides: copy_strided / copy16_strided
        sbase = np.zeros(2 * n, src)
        sbase[::2] = v
        dbase = gpu.asarray(_sentinel(n, dst))
        _mi_copy(core, gpu.asarray(sbase)[::2], dbase[::-1])
        got = dbase.get()[::-1]
        assert ac.same(got, want), "strided {} -> {}: {} of {} differ, first at value {!r}".format(
            src, dst, *_first_difference(got, want, v))
        # dst[...] = src into a strided view of a larger array; the rest of the array keeps its sentinel
        big_host = _sentinel(3 * n + 5, dst)
        big = gpu.asarray(big_host)
        view = big[2:2 + 3 * n:3]
        view[...] = gpu.asarray(v)
        after = big.get()
        assert ac.same(after[2:2 + 3 * n:3], want), "into a view {} -> {}: {} of {} differ, first at value {!r}".format(
            src, dst, *_first_difference(after[2:2 + 3 * n:3], want, v))
        keep = np.ones(3 * n + 5, bool)
        keep[2:2 + 3 * n:3] = False
        assert np.array_equal(_raw(after[keep]), _raw(big_host[keep])), "{} -> {}: wrote outside the view".format(src, dst)


def _first_difference(got, want, v):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind == "f":
        u = np.dtype("u{}".format(got.dtype.itemsize))
        bad = (np.isnan(got) != np.isnan(want)) | (~np.isnan(want) & (got.view(u) != want.view(u)))
    else:
        bad = got != want
    i = int(np.flatnonzero(bad)[0])
    return int(bad.sum()), bad.size, (v[i].item(), got[i].item(), want[i].item())


@pytest.mark.parametrize("name", ["up", "down", "neg_up", "neg_down", "subnormal", "top"])
def test_float64_to_float16_rounds_once(gpu, name):
    """convert16 in csrc/copy.hip is written as double -> float -> half, which would round twice; the compiler merges the
    two truncations into one direct conversion, so the device rounds once.  This test guards that it stays so."""
    x = ac.f16_witnesses()[name]
    want = ac.expected_cast(x, np.float16)
    got = gpu.asarray(x).astype(np.float16).get()
    bad = got.view(np.uint16) != want.view(np.uint16)
    i = int(np.flatnonzero(bad)[0]) if bad.any() else 0
    assert not bad.any(), "float64 -> float16 rounded twice: {} of {} witnesses differ, e.g. {!r} gives bits {:#06x}, NumPy {:#06x}".format(
        int(bad.sum()), bad.size, float(x[i]), int(got.view(np.uint16)[i]), int(want.view(np.uint16)[i]))
    # the strided kernel is the same conversion
    base = gpu.asarray(np.repeat(x, 2))
    got = base[::2].astype(np.float16).get()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


def test_float64_to_float16_examples(gpu):
    x = np.array([1 + 2.0 ** -11 + 2.0 ** -30, 65519.999, -65519.999, 65520.0])
    got = gpu.asarray(x).astype(np.float16).get().view(np.uint16).tolist()
    assert got == [0x3c01, 0x7bff, 0xfbff, 0x7c00], [hex(g) for g in got]


# ---------------------------------------------------------------- round_half_even = 1
@pytest.mark.parametrize("src", [np.dtype(np.float32), np.dtype(np.float64)], ids=str)
def test_copy_round_half_even(gpu, core, src):
    vals = np.concatenate([ac.ladder(src), ac.rint_ties(src)])
    for dst in ac.DTYPES:
        if dst.kind not in "iu":
            continue
        v = vals[ac.rint_admitted(vals, dst) & ac.admitted(vals, dst)]
        want = np.rint(v).astype(dst)
        out = gpu.empty(v.shape, dst)
        _mi_copy(core, gpu.asarray(v), out, rhe=1)
        got = out.get()
        assert np.array_equal(got, want), "{} -> {} half-even: {} of {} differ, first {!r}".format(src, dst, *_first_difference(got, want, v))
        base = gpu.asarray(np.repeat(v, 2))
        out = gpu.empty((2 * v.size,), dst)
        _mi_copy(core, base[::2], out[1::2], rhe=1)
        assert np.array_equal(out.get()[1::2], want), (src, dst, "strided")


# ---------------------------------------------------------------- layouts
def _layout_source(base_shape, dtype, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(base_shape, dtype=np.int64))
    if np.dtype(dtype).kind == "f":
        return (rng.integers(-32768 * 4, 32767 * 4, size=n) * 0.25).astype(dtype).reshape(base_shape)       # quarters: the cast truncates
    return rng.integers(0, 65536, size=n).astype(dtype).reshape(base_shape)


@pytest.mark.parametrize("shape", ac.RANK_SHAPES, ids=lambda s: "rank{}".format(len(s)))
def test_layouts(gpu, core, shape):
    for k, (base_shape, view) in enumerate(ac.layouts(shape)):
        for src, dst in ((np.float32, np.int16), (np.uint16, np.uint16)):
            hb = _layout_source(base_shape, src, 100 + k)
            db = _dev(gpu, hb)
            hv, dv = view(hb), view(db)
            tag = (view, np.dtype(src).name)
            assert dv.shape == hv.shape and dv.dtype == hv.dtype, tag
            lo, hi = core._bounds(dv)
            assert db.ptr <= lo and hi <= db.ptr + db.nbytes, tag            # the view lies inside its allocation
            assert dv.strides == hv.strides or 1 in hv.shape or hv.size <= 1, tag
            assert np.array_equal(dv.get(), hv), tag                          # get() of a view
            c = dv.copy()
            assert c._is_c_contiguous() and np.array_equal(c.get(), hv), tag
            assert np.array_equal(dv.astype(dst).get(), hv.astype(dst)), tag
            assert np.array_equal(core.ascontiguousarray(dv).get(), hv), tag
            # set() on a (possibly strided) target: the base changes exactly where NumPy's does
            tb_host = _layout_source(base_shape, dst, 300 + k)
            tb = _dev(gpu, tb_host)
            new = _layout_source(hv.shape, dst, 500 + k)
            view(tb).set(new)
            view(tb_host)[...] = new
            assert np.array_equal(tb.get(), tb_host), tag
            # cast into a strided target
            view(tb)[...] = dv
            view(tb_host)[...] = hv.astype(dst)
            assert np.array_equal(tb.get(), tb_host), tag
            # reshape / ravel of a view (a copy when it is not contiguous), transposes
            assert np.array_equal(dv.ravel().get(), hv.ravel()), tag
            assert np.array_equal(dv.reshape(-1, 1).get(), hv.reshape(-1, 1)), tag
            if hv.ndim < ac.MAX_NDIM:
                assert np.array_equal(dv.reshape((1,) + hv.shape[::-1]).get(), hv.reshape((1,) + hv.shape[::-1])), tag
            assert np.array_equal(dv.T.get(), hv.T) and dv.T.shape == hv.T.shape, tag
            if hv.ndim >= 2:
                axes = tuple(range(-1, -hv.ndim - 1, -1))
                assert np.array_equal(dv.transpose(*axes).get(), hv.transpose(*axes)), tag
                axes = (-1,) + tuple(range(hv.ndim - 1))
                assert np.array_equal(dv.transpose(axes).get(), hv.transpose(axes)), tag
                with pytest.raises(ValueError):
                    dv.transpose(*([0] * hv.ndim))


def test_reshape_errors_and_rank_limit(gpu):
    a = gpu.asarray(np.arange(24, dtype=np.int32))
    assert a.reshape(2, -1, 3).shape == (2, 4, 3)
    with pytest.raises(ValueError):
        a.reshape(5, 5)
    with pytest.raises(ValueError):
        a.reshape(-1, -1)
    with pytest.raises(ValueError):
        gpu.empty((1,) * 9, np.uint8)
    with pytest.raises(TypeError):
        gpu.empty((2,), np.complex64)


# ---------------------------------------------------------------- grid-stride loops
BIG = 2 ** 21 + 4099            # grid_for caps a launch at 8192 blocks of 256 threads = 2**21 threads


def test_grid_stride_contiguous_cast(gpu):
    x = (np.arange(BIG, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint8)
    assert np.array_equal(gpu.asarray(x).astype(np.float32).get(), x.astype(np.float32))


def test_grid_stride_strided_copy(gpu):
    x = (np.arange(2 * BIG, dtype=np.uint32) * 2654435761 >> 11).astype(np.uint8)
    got = gpu.asarray(x)[::2].copy()
    assert got.shape == (BIG,) and np.array_equal(got.get(), x[::2])


def test_grid_stride_strided_fill(gpu):
    host = _sentinel(2 * BIG, np.uint8)
    a = gpu.asarray(host)
    a[::2].fill(7)
    got = a.get()
    assert (got[::2] == 7).all() and (got[1::2] == 0xA5).all()


# ---------------------------------------------------------------- fill / full / ones / zeros
_FILL_VALUES = [0, -0.0, 1, -1, 255, 256, 1.5]


def _fill_expectation(value, dtype):
    """(admitted, expected scalar array) for `value` filled into `dtype`: the cast rule applied to the float64 value"""
    v = np.array([float(value)])
    if dtype.kind in "iu" and not ac.admitted(v, dtype)[0]:
        return False, None
    return True, ac.expected_cast(v, dtype)


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=str)
def test_fill_values(gpu, dtype):
    values = list(_FILL_VALUES)
    if dtype.kind in "fb":
        values.append(float("nan"))
    n = 37
    for value in values:
        ok, want = _fill_expectation(value, dtype)
        if not ok:
            continue
        if dtype.kind == "b":
            assert want[0] == bool(value)                   # the truth value (NaN is True, -0.0 is False)
        want_all = np.repeat(want, n)
        a = gpu.asarray(_sentinel(n, dtype))
        a.fill(value)
        assert ac.same(a.get(), want_all), "fill({!r}) into {}: got {!r}, want {!r}".format(value, dtype, a.get()[0], want[0])
        f = gpu.full((n,), value, dtype)
        assert f.dtype == dtype and ac.same(f.get(), want_all), "full({!r}, {}): got {!r}".format(value, dtype, f.get()[0])
        host = _sentinel(2 * n + 1, dtype)
        b = gpu.asarray(host)
        b[1::2].fill(value)
        got = b.get()
        assert ac.same(got[1::2], want_all), "strided fill({!r}) into {}: got {!r}".format(value, dtype, got[1])
        assert np.array_equal(_raw(got[::2]), _raw(host[::2])), (value, dtype, "wrote outside the view")
        c = gpu.asarray(host)
        c[1::2] = value                                       # __setitem__ with a scalar is a fill
        assert ac.same(c.get()[1::2], want_all), (value, dtype)
    ones, zeros = gpu.ones((3, 5), dtype), gpu.zeros((3, 5), dtype)
    assert ac.same(ones.get(), np.ones((3, 5), dtype)) and ac.same(zeros.get(), np.zeros((3, 5), dtype))
    assert ac.same(gpu.zeros_like(ones).get(), np.zeros((3, 5), dtype))
    assert gpu.full((0, 3), 1, dtype).get().shape == (0, 3)


def test_fill_keeps_the_sign_of_zero(gpu):
    for dtype in (np.float16, np.float32, np.float64):
        a = gpu.full((9,), -0.0, dtype).get()
        assert np.signbit(a).all() and (a == 0).all(), "fill(-0.0) into {} stored {!r}: the sign of zero is lost".format(
            np.dtype(dtype).name, a[0])
        assert not np.signbit(gpu.full((9,), 0.0, dtype).get()).any()


@pytest.mark.parametrize("dtype,value", [(np.int64, 2 ** 53 + 1), (np.int64, 2 ** 63 - 1), (np.int64, -2 ** 63),
                                         (np.int64, -2 ** 53 - 1), (np.uint64, 2 ** 53 + 1), (np.uint64, 2 ** 63 - 1),
                                         (np.uint64, 2 ** 64 - 1)])
def test_fill_64bit_integers_exactly(gpu, dtype, value):
    want = np.full((11,), value, dtype)
    a = gpu.full((11,), value, dtype).get()
    assert np.array_equal(a, want), "full({}, {}) stored {}".format(value, np.dtype(dtype).name, int(a[0]))
    host = np.zeros(23, dtype)
    b = gpu.asarray(host)
    b[1::2].fill(np.array(value, dtype)[()])                  # a NumPy scalar, into a strided view
    host[1::2] = value
    assert np.array_equal(b.get(), host), "strided fill({}) stored {}".format(value, int(b.get()[1]))
    c = gpu.zeros((4, 3), dtype)
    c[1:3, ::2] = value
    host = np.zeros((4, 3), dtype)
    host[1:3, ::2] = value
    assert np.array_equal(c.get(), host)


# ---------------------------------------------------------------- __getitem__ / __setitem__
_KEYS = [
    Ellipsis, (Ellipsis, 1), (1, Ellipsis), (None,), (None, 2), (Ellipsis, None), (1, None, Ellipsis, None, 2),
    -1, (-1, -2, -3), (slice(None), -1), (slice(None, None, -1),), (slice(4, 0, -2), Ellipsis, slice(None, None, 3)),
    (slice(-2, None), slice(None, -1), slice(-5, -1, 2)), (slice(1, 4), 2, slice(None, None, -2)),
    (slice(3, 3),), (slice(4, 1),), (Ellipsis, slice(0, 0)), (slice(10, 20),), (slice(None, None, -7), slice(-100, 100)),
    (2, slice(None, None, -1), slice(6, None, -1)), (),
]


def test_getitem_matches_numpy(gpu):
    h = np.arange(5 * 6 * 7, dtype=np.int32).reshape(5, 6, 7)
    d = gpu.asarray(h)
    for key in _KEYS:
        want = h[key]
        got = d[key]
        assert got.shape == want.shape, key
        assert np.array_equal(got.get(), want), key
        if want.size > 1 and 1 not in want.shape:
            assert got.strides == want.strides, key
    for key in (5, -6, (0, 6), (0, 0, -8), (Ellipsis, 7)):
        with pytest.raises(IndexError):
            h[key]
        with pytest.raises(IndexError):
            d[key]
    with pytest.raises(IndexError):
        d[0, 0, 0, 0]
    assert d[1, 2, 3].shape == () and d[1, 2, 3].get() == h[1, 2, 3]
    assert len(d) == 5 and d.T.shape == (7, 6, 5) and d.size == 210 and d.nbytes == 840


def test_setitem_matches_numpy(gpu):
    base = np.arange(5 * 6 * 7, dtype=np.int32).reshape(5, 6, 7)
    rng = np.random.default_rng(0)
    for key in _KEYS:
        shape = base[key].shape
        values = [
            7, -3.9, np.int16(-5), np.array(11), np.array(2.5, np.float32),            # scalars and 0-d arrays
            rng.integers(-99, 99, size=shape).astype(np.int32),                           # a host array
            rng.integers(-99, 99, size=shape).astype(np.float64) * 0.5,                   # ... of another dtype
            rng.integers(-99, 99, size=shape).tolist(),                                   # a list
        ]
        for value in values:
            if isinstance(value, list) and 0 in shape:
                continue                                        # [] carries no shape of its own
            h = base.copy()
            d = gpu.asarray(base)
            h[key] = value
            d[key] = value
            assert np.array_equal(d.get(), h), (key, type(value))
        # a device array, contiguous and as a strided view of another dtype
        src = rng.integers(-99, 99, size=shape).astype(np.int16)
        h = base.copy()
        d = gpu.asarray(base)
        h[key] = src
        d[key] = gpu.asarray(np.repeat(src.reshape(shape + (1,)), 2, axis=-1))[..., 1]
        assert np.array_equal(d.get(), h), key
    # a 0-d device array is a value like any other array of one element
    d = gpu.asarray(base)
    d[2, 3, 4] = gpu.asarray(np.array(-1, np.int32))
    h = base.copy()
    h[2, 3, 4] = -1
    assert np.array_equal(d.get(), h)


def test_setitem_shapes(gpu):
    target = np.zeros((4, 6), np.float32)
    for shape in [(6, 4), (24,), (2, 12), (3, 8), (4, 3, 2), (1, 24), (6, 1, 4)]:
        src = np.arange(24, dtype=np.float32).reshape(shape)
        with pytest.raises(ValueError):
            target[...] = src
        for value in (src, gpu.asarray(src)):
            d = gpu.zeros((4, 6), np.float32)
            with pytest.raises(ValueError, match="could not broadcast"):
                d[...] = value
            assert not d.get().any(), shape                     # and nothing was written
    with pytest.raises(ValueError):
        gpu.zeros((4, 6), np.float32)[1:3] = gpu.zeros((3, 6), np.float32)
    # shapes that agree once unit axes are dropped are accepted
    src = np.arange(24, dtype=np.float32).reshape(4, 6)
    for shape in [(1, 4, 6), (4, 1, 6), (4, 6, 1), (1, 4, 1, 6, 1)]:
        d = gpu.zeros((4, 6), np.float32)
        d[...] = gpu.asarray(src.reshape(shape))
        assert np.array_equal(d.get(), src), shape
        d = gpu.zeros(shape, np.float32)
        d[...] = gpu.asarray(src)
        assert np.array_equal(d.get(), src.reshape(shape)), shape
    d = gpu.zeros((4, 6), np.float32)
    d[None, :, None] = gpu.asarray(src)                         # unit axes on the target side
    assert np.array_equal(d.get(), src)


def _shifted(core, gpu, host, dst_key, src_key):
    d = gpu.asarray(host)
    want = host.copy()
    want[dst_key] = host[src_key].copy()                        # NumPy assigns as if from a copy
    d[dst_key] = d[src_key]
    return d.get(), want


def test_overlapping_assignment_1d(gpu, core):
    n = 2 ** 16 + 3
    host = (np.arange(n, dtype=np.uint32) * 2654435761).astype(np.int32)
    for dst_key, src_key in [(slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None)),
                             (slice(None), slice(None, None, -1)), (slice(7, None), slice(None, -7)),
                             (slice(None, -1, 2), slice(1, None, 2)), (slice(2, None, 2), slice(1, -1, 2))]:
        got, want = _shifted(core, gpu, host, dst_key, src_key)
        bad = got != want
        assert not bad.any(), "a[{}] = a[{}] on {} elements: {} differ from NumPy, first at index {}".format(
            dst_key, src_key, n, int(bad.sum()), int(np.flatnonzero(bad)[0]))


def test_overlapping_assignment_3d(gpu, core):
    shape = (48, 40, 36)                                        # 69120 elements
    host = np.random.default_rng(1).integers(0, 2 ** 31, size=shape).astype(np.float32)
    full = slice(None)
    for axis in range(3):
        for dst_s, src_s in [(slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None))]:
            dst_key = (full,) * axis + (dst_s,)
            src_key = (full,) * axis + (src_s,)
            got, want = _shifted(core, gpu, host, dst_key, src_key)
            bad = got != want
            assert not bad.any(), "3-D shift along axis {} ({} <- {}): {} of {} elements differ from NumPy".format(
                axis, dst_s, src_s, int(bad.sum()), bad.size)


def test_same_view_assignment_is_a_noop(gpu):
    host = np.arange(1000, dtype=np.float64)
    d = gpu.asarray(host)
    d[...] = d
    d[::3] = d[::3]
    d[::-1] = d[::-1]
    assert np.array_equal(d.get(), host)


def test_writes_drop_the_host_hint(gpu, core):
    h = np.arange(12, dtype=np.uint8).reshape(3, 4)

    def hinted():
        return core.with_host_hint(gpu.asarray(h), h)

    writes = [
        lambda a: a.__setitem__(Ellipsis, 1),
        lambda a: a.__setitem__((slice(1, None), slice(None, None, 2)), np.array([[9, 8], [7, 6]], np.uint8)),
        lambda a: a.__setitem__(slice(1, None), a[:-1]),
        lambda a: a.__setitem__(0, gpu.asarray(np.array([5, 5, 5, 5], np.uint8))),
        lambda a: a.fill(3),
        lambda a: a.set(h[::-1]),
        lambda a: a[1:].fill(2),
        lambda a: a.T.set(np.zeros((4, 3), np.uint8)),
        lambda a: a[:, 1].__setitem__(Ellipsis, 0),
        lambda a: core._copy(gpu.asarray(h + 1), a),
        lambda a: core._copy(gpu.asarray(h[0] + 1), a[2]),
    ]
    for k, write in enumerate(writes):
        a = hinted()
        assert a._hc is not None and np.array_equal(core.host_copy(a), h)
        write(a)
        assert a._hc is None, k
        assert np.array_equal(core.host_copy(a), a.get()) and not np.array_equal(a.get(), h), k


# ---------------------------------------------------------------- shares_memory / arrays_differ
def test_shares_memory(gpu, core):
    a = gpu.zeros((100,), np.float32)
    b = gpu.zeros((100,), np.float32)
    sm = core.shares_memory
    assert sm(a, a) and sm(a, a[10:20]) and sm(a[:50], a[49:]) and not sm(a, b)
    assert not sm(a[:50], a[50:])                               # disjoint halves of one allocation
    assert sm(a[::2], a[1::2])                                  # interleaved: the bounds overlap (MAY_SHARE_BOUNDS)
    assert sm(a[::-1], a) and sm(a[::-1][:50], a[50:]) and not sm(a[::-1][:50], a[:50])        # negative strides
    assert sm(a[99:49:-1], a[50:]) and not sm(a[49::-1], a[50:])
    assert not sm(a[:0], a) and not sm(a, a[5:5]) and not sm(gpu.empty((0,)), gpu.empty((0,)))   # empty arrays
    assert not sm(a, np.zeros(3)) and not sm(None, a)
    m = gpu.zeros((8, 8), np.uint8)
    assert sm(m[:, :4], m[:, 4:]) and not sm(m[:4], m[4:]) and sm(m.T, m)
    h = np.zeros(100, np.float32)
    for x, y in [(slice(None, 50), slice(50, None)), (slice(None, None, 2), slice(1, None, 2)),
                 (slice(None, None, -1), slice(None))]:
        assert sm(a[x], a[y]) == np.may_share_memory(h[x], h[y])


def test_arrays_differ(gpu, core):
    for dtype in ac.DTYPES:
        x = ac.exact_array(dtype, (3, 1025), 5)
        a, b = gpu.asarray(x), gpu.asarray(x)
        assert core.arrays_differ(a, b) is False, dtype
        y = x.copy()
        if dtype.kind == "f":
            y[2, 1024] += dtype.type(1)
        else:
            y[2, 1024] ^= dtype.type(1)                          # the last bit of the last element
        assert core.arrays_differ(a, gpu.asarray(y)) is True, dtype
        assert core.arrays_differ(a.T, gpu.asarray(np.ascontiguousarray(x.T))) is False, dtype       # views are compacted first
    for dtype in (np.float16, np.float32, np.float64):
        nan = gpu.asarray(np.full(300, np.nan, dtype))
        assert core.arrays_differ(nan, nan.copy()) is False                       # equal NaNs are equal bytes
        assert core.arrays_differ(gpu.zeros((300,), dtype), gpu.full((300,), -0.0, dtype)) is True      # +0.0 and -0.0 are not
    assert "byte" in core.arrays_differ.__doc__
    assert core.arrays_differ(gpu.empty((0, 4)), gpu.empty((0, 4))) is False
    with pytest.raises(ValueError):
        core.arrays_differ(gpu.zeros((3,)), gpu.zeros((4,)))
    with pytest.raises(ValueError):
        core.arrays_differ(gpu.zeros((3,), np.int32), gpu.zeros((3,), np.float32))
