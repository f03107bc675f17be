"""The Hessian family on the device (csrc/ridges.hip: mi_hessian_matrix, mi_symmetric_eigvals, mi_ridge_scale) against the
host transcription tests/helpers/ridge_ref.py.

1. hessian_matrix: bit-identical to numpy.gradient applied twice to the device's own smoothed array, tile and per-voxel
   routes, every mode, cval != 0, both orders.
2. eigenvalues: 2-D bit-identical to the transcribed closed form; larger matrices within 8 eps(dtype) ||H||_F of float64
   eigvalsh of the same elements (16 x what float32 LAPACK needs, tests/test_ridge_yardstick.py), in the right order.
3. responses: the transcribed response applied in the same dtype to the device's own ordered eigenvalues against the device
   response of one scale: frangi absolute 16 eps (three factors in [0, 1], each behind an exp), sato relative 8 eps,
   meijering absolute 8 eps with the device minimum equal to aux.min() exactly.
4. whole functions against the transcription on SciPy's Gaussian within 1e-6 max|reference| (wiring), routes bit for bit.
5. burst: the last of 20 back-to-back calls equals the first.

Figures of the first run on an MI355X, in the units of the bounds: eigenvalues float32 at most 1.64 (bound 8), float64 at
most 6.80 -- there the float64 LAPACK reference carries most of it (in emulation it is itself up to 7.7 from a 40-digit
solution where the device solver stays below 1); frangi at most 1.5 (bound 16); sato and meijering 0 (bound 8)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from helpers import ridge_ref as rr

pytestmark = pytest.mark.gpu

# (tile rows, tile planes, per-voxel kernels): the planner's tiles, small tiles (seams on every axis), the unfused route
SETTINGS = [(0, 0, 0), (3, 2, 0), (0, 0, 1)]
SMALL = [(2, 2), (2, 3, 2), (3, 5), (5, 4, 3)]
RAGGED = [(9, 67), (7, 9, 67)]
SEAMS = [(19, 23, 70)]
RANK4 = [(4, 5, 6, 7)]
DTYPES = ["float32", "float64"]
MODES = ["constant", "reflect", "wrap", "nearest", "mirror"]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.fixture(scope="module")
def mods(gpu):
    from cupyimg_amd.skimage import feature, filters
    return feature, filters


@pytest.fixture()
def knob(gpu):
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_ridges
    fn.argtypes = [ctypes.c_int] * 3
    yield fn
    fn(0, 0, 0)


@functools.lru_cache(maxsize=None)
def _image(shape, dtype, seed=1):
    x = rr.volume(shape, np.dtype(dtype), seed)
    x.setflags(write=False)
    return x


def _smoothed(gpu, x, sigma, mode="reflect", cval=0):
    from cupyimg_amd.scipy import ndimage as ndi
    return ndi.gaussian_filter(gpu.asarray(x), sigma=sigma, mode=mode, cval=cval).get()


# ---------------------------------------------------------------- 1. hessian_matrix
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SMALL + RAGGED + SEAMS + RANK4, ids=_ids(SMALL + RAGGED + SEAMS + RANK4))
def test_hessian_matrix_is_numpy_gradient_twice_bit_for_bit(gpu, mods, knob, shape, dtype):
    feature, _ = mods
    x = _image(shape, dtype)
    xd = gpu.asarray(x)
    for mode, cval in [(m, 0) for m in MODES] + [("constant", 0.75)]:
        g = _smoothed(gpu, x, 1.0, mode, cval)
        assert g.dtype == np.dtype(dtype)
        for order in ("rc", "xy"):
            want = rr.hessian_from_smoothed(g, order)
            for setting in SETTINGS:
                knob(*setting)
                got = feature.hessian_matrix(xd, sigma=1.0, mode=mode, cval=cval, order=order)
                assert len(got) == len(want)
                for e, (a, b) in enumerate(zip(got, want)):
                    assert a.shape == shape and a.dtype == np.dtype(dtype)
                    assert np.array_equal(a.get(), b), (mode, order, setting, e)


def test_hessian_matrix_routes(gpu, mods, knob):
    from cupyimg_amd import last_kernel
    feature, _ = mods
    xd = gpu.asarray(_image((19, 23, 70), "float32"))
    feature.hessian_matrix(xd)
    assert "ridge_tile_kernel<float32,3,hessian-rc>" in last_kernel() and "tile=8x8x64" in last_kernel()
    knob(3, 2, 0)
    feature.hessian_matrix(xd, order="xy")
    assert "ridge_tile_kernel<float32,3,hessian-xy>" in last_kernel() and "tile=2x3x16" in last_kernel()
    knob(0, 0, 1)
    feature.hessian_matrix(xd)
    assert "hessian_generic_kernel<float32>" in last_kernel()
    knob(0, 0, 0)
    feature.hessian_matrix(gpu.asarray(_image((4, 5, 6, 7), "float64")))
    assert "hessian_generic_kernel<float64>" in last_kernel() and "rank 4" in last_kernel()


def test_hessian_matrix_docstring_example_and_integer_input(gpu, mods):
    feature, _ = mods
    square = np.zeros((5, 5))
    square[2, 2] = 4
    Hrr, Hrc, Hcc = feature.hessian_matrix(gpu.asarray(square), sigma=0.1, order="rc")
    want = np.array([[0, 0, 0, 0, 0], [0, 1, 0, -1, 0], [0, 0, 0, 0, 0], [0, -1, 0, 1, 0], [0, 0, 0, 0, 0]], float)
    assert np.allclose(Hrc.get(), want, atol=1e-12)
    eigs = feature.hessian_matrix_eigvals([Hrr, Hrc, Hcc])
    want = np.array([[0, 0, 2, 0, 0], [0, 1, 0, 1, 0], [2, 0, -2, 0, 2], [0, 1, 0, 1, 0], [0, 0, 2, 0, 0]], float)
    assert np.allclose(eigs.get()[0], want, atol=1e-12)
    u8 = (np.arange(35).reshape(5, 7) * 7 % 256).astype(np.uint8)
    got = feature.hessian_matrix(gpu.asarray(u8), sigma=1.0)
    want = rr.hessian_matrix(u8, sigma=1.0)
    for a, b in zip(got, want):
        assert a.dtype == np.float64 and np.allclose(a.get(), b, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        feature.hessian_matrix(gpu.asarray(np.zeros((1, 5))))


# ---------------------------------------------------------------- 2. eigenvalues
def _check_eigs(got, elems, dtype, sorting="none"):
    """got: (n, ...) device eigenvalues of the matrices with upper triangles `elems` (host arrays of `dtype`)"""
    n = got.shape[0]
    assert got.dtype == np.dtype(dtype)
    if n == 2:
        want = rr.order_eigenvalues(np.stack(rr.eigvals22(*[e.copy() for e in elems])), sorting)
        assert np.array_equal(got, want)
        return
    e64 = [e.astype(np.float64) for e in elems]
    ref = rr.hessian_matrix_eigvals(e64, np.float64)                    # decreasing
    fro = np.sqrt((rr.symmetric_image(e64) ** 2).sum((-1, -2)))
    bound = 8 * np.finfo(dtype).eps * fro
    g = got.astype(np.float64)
    # the order: as asked, on the device's own values
    if sorting == "none":
        assert np.all(np.diff(g, axis=0) <= 0)
    elif sorting == "val":
        assert np.all(np.diff(g, axis=0) >= 0)
    else:
        assert np.all(np.diff(np.abs(g), axis=0) >= 0)
    err = np.abs(np.sort(g, axis=0)[::-1] - ref).max(0)
    worst = (err / np.where(fro > 0, np.finfo(dtype).eps * fro, 1)).max()
    print("eigenvalue error / (eps ||H||_F):", worst)
    assert np.all(err <= bound), worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SMALL + RAGGED + SEAMS + RANK4, ids=_ids(SMALL + RAGGED + SEAMS + RANK4))
def test_eigenvalues_of_device_made_elements(gpu, mods, knob, shape, dtype):
    feature, filters = mods
    x = _image(shape, dtype)
    xd = gpu.asarray(x)
    elems = feature.hessian_matrix(xd, sigma=1.5, mode="reflect")
    host = [e.get() for e in elems]
    _check_eigs(feature.hessian_matrix_eigvals(elems).get(), host, dtype)
    s2 = np.dtype(dtype).type(1.5 ** 2)
    scaled = [s2 * e for e in host]
    first = {}
    for setting in SETTINGS:
        knob(*setting)
        for sorting in ("none", "val", "abs"):
            got = filters.compute_hessian_eigenvalues(xd, 1.5, sorting=sorting, mode="reflect").get()
            assert got.shape == (len(shape),) + shape
            _check_eigs(got, scaled, dtype, sorting)
            # every route gives the same bits
            assert np.array_equal(first.setdefault(sorting, got), got), (setting, sorting)


HAND = {
    "diagonal": [[3.0, 0, 0, -1.0, 0, 2.0], [1.0, 0, 0, 1.0, 0, 1.0], [-5.0, 0, 0, 7.0, 0, 0.0]],
    "all equal": [[2.0] * 6, [-0.3] * 6],
    "rank one": [[1.0, 2.0, 3.0, 4.0, 6.0, 9.0], [0.25, -0.5, 0.75, 1.0, -1.5, 2.25]],
    "two equal": [[2.0, 0, 0, 2.0, 0, 5.0], [3.0, 1.0, 1.0, 3.0, 1.0, 3.0]],
    "zero": [[0.0] * 6],
    "tiny off-diagonal": [[1.0, 1e-30, 0, 2.0, 1e-25, 3.0], [1.0, 1e-9, 1e-9, 1.0, 1e-9, 1.0]],
}


@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_made_matrices(gpu, mods, dtype):
    feature, _ = mods
    rows = [r for name in HAND for r in HAND[name]]
    m = len(rows)
    # a (2, 2, m) "volume" so that the rank is 3: every voxel of a column holds the same matrix
    elems = [np.broadcast_to(np.array([r[e] for r in rows], dtype), (2, 2, m)).copy() for e in range(6)]
    got = feature.hessian_matrix_eigvals([gpu.asarray(e) for e in elems]).get()
    _check_eigs(got, elems, dtype)
    assert np.array_equal(got[:, 0, 0, rows.index([0.0] * 6)], np.zeros(3))
    assert np.array_equal(got[:, 0, 0, 0], np.array([3.0, 2.0, -1.0], dtype))
    # 4 x 4 as well (rank 4, 10 elements): diag(1, -2, 3, 0.5) and the all-ones matrix
    e4 = [np.zeros((2, 2, 2, 2), dtype) for _ in range(10)]
    for idx, v in zip((0, 4, 7, 9), (1.0, -2.0, 3.0, 0.5)):
        e4[idx][0] = v
    for e in e4:
        e[1] = 1.0
    got = feature.structure_tensor_eigenvalues([gpu.asarray(e) for e in e4]).get()
    _check_eigs(got, e4, dtype)
    assert np.array_equal(got[:, 0, 0, 0, 0], np.array([3.0, 1.0, 0.5, -2.0], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_abs_ordering_ties_keep_the_decreasing_order(gpu, mods, knob, dtype):
    """G = x^2 - y^2 + z^2 / 2 away from the borders: Hessian diag(1, -2, 2) (axes z, y, x), decreasing 2, 1, -2, so the stable
    sort by magnitude gives 1, 2, -2 -- never 1, -2, 2"""
    _, filters = mods
    z, y, x = np.meshgrid(*[np.arange(9.0)] * 3, indexing="ij")
    g = (x * x - y * y + z * z / 2).astype(dtype)
    from cupyimg_amd import core
    from cupyimg_amd.skimage.filters import _ridge_scale
    for setting in SETTINGS:
        knob(*setting)
        out = core.empty((3, g.size), np.dtype(dtype))
        _ridge_scale(gpu.asarray(g), out, 0, 2, 1.0)
        got = out.get().reshape(3, 9, 9, 9)[:, 4, 4, 4]
        assert got.tolist() == [1.0, 2.0, -2.0], (setting, got)


# ---------------------------------------------------------------- 3. responses
def _response_image(shape, dtype):
    x = _image(shape, dtype).copy()
    x[tuple(slice(0, max(2, n // 2)) for n in shape)] = 0.5        # a constant block: exact-zero eigenvalues
    return x


RESP = RAGGED + SEAMS + [(3, 5), (5, 4, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", RESP, ids=_ids(RESP))
def test_responses_from_the_device_eigenvalues(gpu, mods, knob, shape, dtype):
    _, filters = mods
    eps = np.finfo(dtype).eps
    x = _response_image(shape, dtype)
    sigma = 1.0
    for setting in SETTINGS[:2] if shape in SEAMS else SETTINGS[:1] + SETTINGS[2:]:
        knob(*setting)
        for black in (True, False):
            # the filters invert before smoothing; hand the inverted image to compute_hessian_eigenvalues
            inv = rr.invert(x)
            for alpha, beta, gamma in [(0.5, 0.5, 15), (0.3, 0.8, 0.05)]:
                img = inv if black else x
                eigs = filters.compute_hessian_eigenvalues(gpu.asarray(img), sigma, sorting="abs", mode="reflect").get()
                want = rr.frangi_response(eigs, alpha, beta, gamma)
                got = filters.frangi(gpu.asarray(x), sigmas=[sigma], alpha=alpha, beta=beta, gamma=gamma, black_ridges=black,
                                     mode="reflect").get()
                assert got.dtype == np.float64
                d = np.abs(got - want.astype(np.float64)).max()
                print("frangi", setting, black, (alpha, beta, gamma), "max abs diff / eps:", d / eps)
                assert d <= 16 * eps
            img = x if black else inv
            eigs = filters.compute_hessian_eigenvalues(gpu.asarray(img), sigma, sorting="val", mode="reflect").get()
            want = rr.sato_response(eigs).astype(np.float64)
            got = filters.sato(gpu.asarray(x), sigmas=[sigma], black_ridges=black, mode="reflect").get()
            d = np.abs(got - want)
            print("sato", setting, black, "max rel diff / eps:", (d / np.where(want != 0, np.abs(want), 1)).max() / eps)
            assert np.all(d <= 8 * eps * np.abs(want))
            for alpha in (None, 0.7):
                img = inv if black else x
                a = 1.0 / len(shape) if alpha is None else alpha
                eigs = filters.compute_hessian_eigenvalues(gpu.asarray(img), sigma, sorting="abs", mode="reflect").get()
                debug = {}
                got = filters._ridge_filter(filters._ridge_input(gpu.asarray(x), black), [sigma], 3, (a, 0, 0), "reflect", 0,
                                            debug).get()
                aux = debug["aux"].get()
                assert aux.dtype == np.dtype(dtype)
                assert debug["min"][0] == aux.min()
                want_aux = rr.meijering_aux(eigs, a)
                assert np.all(np.abs(aux - want_aux) <= 4 * eps * np.abs(want_aux))
                want = rr.meijering_response(aux).astype(np.float64)
                d = np.abs(got - want).max()
                print("meijering", setting, black, a, "max abs diff / eps:", d / eps)
                assert d <= 8 * eps
                assert np.array_equal(filters.meijering(gpu.asarray(x), sigmas=[sigma], alpha=alpha, black_ridges=black).get(), got)


# ---------------------------------------------------------------- 4. whole functions
@functools.lru_cache(maxsize=None)
def _whole_ref(name, shape, black, mode, cval, kind):
    x = _whole_input(shape, kind)
    kw = dict(sigmas=(1, 2.5), black_ridges=black, mode=mode, cval=cval)
    return getattr(rr, name)(x, **kw)


def _whole_input(shape, kind):
    x = _image(shape, "float64")
    if kind == "uint8":
        return (x * 255).astype(np.uint8)
    if kind == "int16":
        return (x * 60000 - 30000).astype(np.int16)
    if kind == "bool":
        return x > 0.5
    return x


WHOLE = [(9, 67), (19, 23, 70)]


@pytest.mark.parametrize("name", ["meijering", "sato", "frangi", "hessian"])
@pytest.mark.parametrize("shape", WHOLE, ids=_ids(WHOLE))
def test_whole_functions_against_the_transcription(gpu, mods, knob, shape, name):
    from cupyimg_amd import core
    _, filters = mods
    fn = getattr(filters, name)
    cases = [("float64", True, "reflect", 0), ("float64", False, "constant", 0.25), ("uint8", True, "nearest", 0),
             ("int16", False, "mirror", 0), ("bool", True, "wrap", 0)]
    for kind, black, mode, cval in cases:
        x = _whole_input(shape, kind)
        want = _whole_ref(name, shape, black, mode, cval, kind)
        xd = gpu.asarray(x)
        results = []
        for setting in SETTINGS:
            knob(*setting)
            got = fn(xd, sigmas=(1, 2.5), black_ridges=black, mode=mode, cval=cval)
            assert got.dtype == np.float64 and got.shape == shape
            assert not core.shares_memory(got, xd)
            results.append(got.get())
        d = np.abs(results[0] - want).max()
        print(name, kind, black, mode, "max abs diff / max|ref|:", d / np.abs(want).max())
        assert d <= 1e-6 * np.abs(want).max()
        assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
        assert np.array_equal(xd.get(), x)


def test_rank4_meijering_and_float32_and_views(gpu, mods):
    _, filters = mods
    x = _image((4, 5, 6, 7), "float64")
    want = rr.meijering(x, sigmas=(1, 2.5))
    got = filters.meijering(gpu.asarray(x), sigmas=(1, 2.5)).get()
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    # a non-contiguous input
    big = _image((19, 23, 70), "float64")
    view = gpu.asarray(big)[::2, 1:, ::3]
    want = rr.frangi(big[::2, 1:, ::3], sigmas=(1, 2.5))
    got = filters.frangi(view, sigmas=(1, 2.5)).get()
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    # float32 and float16 come back as float64; float16 is computed in float32
    x32 = _image((9, 67), "float32")
    a = filters.sato(gpu.asarray(x32), sigmas=[1], mode="reflect")
    b = filters.sato(gpu.asarray(x32.astype(np.float16)), sigmas=[1], mode="reflect")
    c = filters.sato(gpu.asarray(x32.astype(np.float16).astype(np.float32)), sigmas=[1], mode="reflect")
    assert a.dtype == b.dtype == np.float64 and np.array_equal(b.get(), c.get())
    # a host input
    assert np.array_equal(filters.sato(x32, sigmas=[1], mode="reflect").get(), a.get())
    assert np.array_equal(filters.meijering(gpu.asarray(np.arange(9.0))).get(), np.zeros(9))


def test_warnings_and_errors(gpu, mods):
    _, filters = mods
    x2 = gpu.asarray(_image((9, 67), "float64"))
    for fn in (filters.sato, filters.hessian):
        with pytest.warns(FutureWarning):
            fn(x2, sigmas=[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        filters.sato(x2, sigmas=[1], mode="reflect")
        filters.frangi(x2, sigmas=[1])
    with pytest.warns(UserWarning):
        a = filters.frangi(x2, scale_range=(1, 3), scale_step=1)
    assert np.array_equal(a.get(), filters.frangi(x2, sigmas=[1, 2]).get())
    for fn in (filters.meijering, filters.sato, filters.frangi, filters.hessian):
        with pytest.raises(ValueError):
            fn(x2, sigmas=[1, -1], mode="reflect")
    x4 = gpu.asarray(_image((4, 5, 6, 7), "float64"))
    x1 = gpu.asarray(np.arange(9.0))
    for fn in (filters.sato, filters.frangi, filters.hessian):
        for bad in (x4, x1):
            with pytest.raises(ValueError):
                fn(bad, sigmas=[1], mode="reflect")
    for fn in (filters.meijering, filters.sato, filters.frangi):
        with pytest.raises(ValueError):
            fn(gpu.asarray(np.zeros((1, 9))), sigmas=[1], mode="reflect")
    with pytest.raises(ValueError):
        filters.compute_hessian_eigenvalues(gpu.asarray(np.zeros((5, 1, 5))), 1.0)


# ---------------------------------------------------------------- 5. burst
def test_burst_of_sato_calls_is_repeatable(gpu, mods):
    _, filters = mods
    xd = gpu.asarray(_image((64, 64, 64), "float32"))
    first = filters.sato(xd, mode="reflect").get()
    last = None
    for _ in range(19):
        last = filters.sato(xd, mode="reflect")
    assert np.array_equal(last.get(), first)
