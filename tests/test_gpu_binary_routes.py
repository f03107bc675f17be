"""Binary morphology outside the 1-byte rank-2 / rank-3 envelope of the bit-packed and tiled kernels, route by route and
bit-exact against the plain NumPy reference of tests/helpers/binary_ref.py: the dtype-templated kernels of csrc/binary.hip
(`binary3_kernel<T>` for ranks 1-3, `binary_erosion_kernel<T, ND>` above), "nonzero is foreground" at the values where it can
go wrong, non-bool masks, every form of `output`, binary_hit_or_miss with both structures and origins, the Minkowski-root
rewrite and its limits, and the until-stable run into an unaligned output that used to spin on the host."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import binary_ref as br

pytestmark = pytest.mark.gpu

TNAME = {"bool": "bool", "int8": "int8", "uint8": "uint8", "int16": "int16", "uint16": "uint16", "int32": "int32",
         "uint32": "uint32", "int64": "int64", "float16": "float", "float32": "float", "float64": "double"}


@pytest.fixture(scope="module")
def ndi(gpu):
    from cupyimg_amd.scipy import ndimage
    return ndimage


@pytest.fixture()
def lib(gpu):
    from cupyimg_amd import _lib
    lib = _lib.load()
    lib.mi_debug_set_bitmorph.argtypes = [ctypes.c_int] * 3
    lib.mi_debug_set_binary_tiled.argtypes = [ctypes.c_int]
    yield lib
    lib.mi_debug_set_bitmorph(1, 0, 0)
    lib.mi_debug_set_binary_tiled(1)


def _lk():
    from cupyimg_amd import last_kernel
    return last_kernel()


def _with_edges(shape, dtype, seed):
    """about half foreground; every edge value of the dtype (and small integers) spread over the foreground, and planted
    in the interior, on a face and in a corner"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    fg = rng.random(shape) < 0.5
    if dt.kind == "b":
        return fg
    values = [np.array(v).astype(dt) for _, v in br.edge_values_for(dt)] + [np.array(1, dt), np.array(3, dt)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = np.zeros(shape, dt)
        pick = rng.integers(len(values), size=shape)
        for i, v in enumerate(values):
            x[fg & (pick == i)] = v
        nd = len(shape)
        for j, v in enumerate(values[:-2]):
            corner = tuple((n - 1) if (j >> d) & 1 else 0 for d, n in enumerate(shape))
            face = (0,) + tuple(min(n - 1, 1 + j % max(1, n - 2)) for n in shape[1:])
            inner = tuple(min(n - 2, 1 + (j + d) % max(1, n - 2)) for d, n in enumerate(shape))
            for pos in (corner, face, inner):
                x[pos] = v
        if dt.kind == "f":
            x[(x == 0) & (rng.random(shape) < 0.5)] = -0.0
    return x


def _same(got, want, what):
    got = got.get()
    assert got.dtype == np.bool_ and np.array_equal(got, want), (what, int((got != want).sum()))


@pytest.mark.parametrize("shape", [(5, 7, 33), (3, 4, 5, 9)])
@pytest.mark.parametrize("dtype", br.IN_DTYPES)
def test_truth_by_dtype(gpu, ndi, lib, dtype, shape):
    x = _with_edges(shape, dtype, 5)
    assert all(np.any(x == np.array(v).astype(x.dtype)) or np.isnan(v) for _, v in br.edge_values_for(dtype))
    mask = np.random.default_rng(9).random(shape) > 0.3
    xd, md = gpu.asarray(x), gpu.asarray(mask)
    route = ("binary3_kernel<%s>" if len(shape) == 3 else "binary_erosion_kernel<%s,") % TNAME[dtype]
    for tiled in ((1, 0) if x.dtype.itemsize == 1 and len(shape) == 3 else (1,)):
        lib.mi_debug_set_binary_tiled(tiled)          # 1-byte volumes: once as dispatched, once through the generic kernel
        for name in ("erosion", "dilation"):
            for m, mdev in ((None, None), (mask, md)):
                for bv in (0, 1):
                    got = getattr(ndi, "binary_" + name)(xd, mask=mdev, border_value=bv)
                    if x.dtype.itemsize > 1 or len(shape) == 4 or not tiled:
                        assert route in _lk(), (route, _lk())
                    _same(got, getattr(br, name)(x, mask=m, border_value=bv), (name, dtype, shape, m is not None, bv, tiled))


@pytest.mark.parametrize("shape", [(37,), (3, 4, 5, 9), (2, 3, 2, 4, 7)])
def test_ranks_1_4_5(gpu, ndi, shape):
    nd = len(shape)
    rng = np.random.default_rng(nd)
    x = (rng.random(shape) < 0.6).astype(np.int16) * 256
    mask = rng.random(shape) > 0.25
    xd, md = gpu.asarray(x), gpu.asarray(mask)
    st = rng.random((3,) * (nd - 1) + (4,)) > 0.3
    origin = [1] + [0] * (nd - 2) + [-1] if nd > 1 else [-2]
    # the first iteration reads the int16 input, every later one the bool volume of the one before it
    route = {True: "binary3_kernel<int16>" if nd == 1 else "binary_erosion_kernel<int16,",
             False: "binary3_kernel<bool>" if nd == 1 else "binary_erosion_kernel<bool,"}
    for name in ("erosion", "dilation"):
        fn, ref = getattr(ndi, "binary_" + name), getattr(br, name)
        for bv in (0, 1):
            for it in (1, 3):
                for m, mdev in ((None, None), (mask, md)):
                    got = fn(xd, st, iterations=it, mask=mdev, border_value=bv, origin=origin)
                    assert route[it == 1] in _lk(), _lk()
                    _same(got, ref(x, st, it, m, bv, origin), (name, shape, bv, it, m is not None))
            # until stable: the default cross (monotone), with and without the mask
            for m, mdev in ((None, None), (mask, md)):
                got = fn(xd, iterations=-1, mask=mdev, border_value=bv)
                assert route[False] in _lk(), _lk()         # (at least two launches: the last one changes nothing)
                _same(got, ref(x, None, -1, m, bv), (name, shape, bv, "until stable", m is not None))


@pytest.mark.parametrize("dtype", ["int16", "float32", "int64"])
def test_multibyte_rank3_iterations(gpu, ndi, dtype):
    """ping-pong parity and the copy back into `final`: 2, 5 and 9 iterations, output given / not given / the input itself"""
    shape = (6, 9, 21)
    x = _with_edges(shape, dtype, 21)
    st = sndi.generate_binary_structure(3, 2)
    for name in ("erosion", "dilation"):
        fn, ref = getattr(ndi, "binary_" + name), getattr(br, name)
        _same(fn(gpu.asarray(x), st), ref(x, st), (name, dtype, 1))
        assert "binary3_kernel<%s>" % TNAME[dtype] in _lk(), _lk()
        for it in (2, 5, 9):
            want = ref(x, st, it, border_value=1 if name == "erosion" else 0)
            kw = dict(iterations=it, border_value=1 if name == "erosion" else 0)
            _same(fn(gpu.asarray(x), st, **kw), want, (name, dtype, it, "no output"))
            assert "binary3_kernel<bool>" in _lk(), _lk()         # the later iterations read the bool volume of the one before
            out = gpu.asarray(np.full(shape, 77, np.int32))
            assert fn(gpu.asarray(x), st, output=out, **kw) is out
            assert np.array_equal(out.get(), want.astype(np.int32)), (name, dtype, it, "output")
            xd = gpu.asarray(x)
            assert fn(xd, st, output=xd, **kw) is xd
            assert np.array_equal(xd.get(), want.astype(x.dtype)), (name, dtype, it, "in place")


@pytest.mark.parametrize("in_dtype", ["uint8", "float32"])
def test_output_forms(gpu, ndi, in_dtype):
    shape = (5, 8, 19)
    x = _with_edges(shape, in_dtype, 4)
    for name in ("erosion", "opening"):
        fn, want = getattr(ndi, "binary_" + name), getattr(br, name)(x, border_value=1)
        for odt in br.OUT_DTYPES:
            out = gpu.asarray(np.full(shape, 77, odt))
            assert fn(gpu.asarray(x), output=out, border_value=1) is out
            got = out.get()
            assert got.dtype == np.dtype(odt) and np.array_equal(got, want.astype(odt)), (name, odt)
            # a dtype instead of an array is ignored, as in SciPy: the result is bool
            res = fn(gpu.asarray(x), output=np.dtype(odt), border_value=1)
            assert sndi.binary_erosion(x, output=np.dtype("int16" if odt == "float16" else odt)).dtype == np.bool_
            _same(res, want, (name, "dtype", odt))
            base = gpu.asarray(np.full(shape[:-1] + (2 * shape[-1],), 77, odt))
            view = base[..., ::2]
            assert fn(gpu.asarray(x), output=view, border_value=1) is view
            host = base.get()
            assert np.array_equal(host[..., ::2], want.astype(odt)) and (host[..., 1::2] == np.full(1, 77, odt)[0]).all(), (name, "strided", odt)
        xd = gpu.asarray(x)
        assert fn(xd, output=xd, border_value=1) is xd
        assert np.array_equal(xd.get(), want.astype(x.dtype)), (name, "in place")
    # return values with an array as output: None from hit_or_miss and fill_holes, as in SciPy
    for name, ref in (("binary_hit_or_miss", br.hit_or_miss), ("binary_fill_holes", br.fill_holes)):
        host_out = np.zeros(shape, np.int16)
        assert getattr(sndi, name)(x, output=host_out) is None
        out = gpu.asarray(np.full(shape, 77, np.int16))
        assert getattr(ndi, name)(gpu.asarray(x), output=out) is None
        assert np.array_equal(out.get(), host_out) and np.array_equal(host_out != 0, ref(x)), name
        assert getattr(ndi, name)(gpu.asarray(x)).get().dtype == np.bool_


def test_non_bool_masks(gpu, ndi):
    shape = (6, 7, 23)
    rng = np.random.default_rng(8)
    on = rng.random(shape) < 0.6
    masks = {
        "uint8": (on * rng.choice([2, 128, 255], size=shape)).astype(np.uint8),
        "int32": (on * 256).astype(np.int32),
        "float32": np.where(on, np.float32(np.nan), np.float32(-0.0)).astype(np.float32),
    }
    for dtype in ("uint8", "float64"):
        x = _with_edges(shape, dtype, 2)
        for mname, m in masks.items():
            assert np.array_equal(br.truth(m), on)
            for name in ("erosion", "dilation"):
                for it in (1, 3):
                    got = getattr(ndi, "binary_" + name)(gpu.asarray(x), iterations=it, mask=gpu.asarray(m))
                    _same(got, getattr(br, name)(x, None, it, on), (name, dtype, mname, it))
            _same(ndi.binary_propagation(gpu.asarray(x), mask=gpu.asarray(m)), br.propagation(x, mask=on), ("propagation", dtype, mname))
    for fn, sfn in ((ndi.binary_erosion, sndi.binary_erosion), (ndi.binary_dilation, sndi.binary_dilation)):
        with pytest.raises(RuntimeError):
            sfn(x, mask=on[:-1])
        with pytest.raises(RuntimeError):
            fn(gpu.asarray(x), mask=gpu.asarray(on[:-1]))


@pytest.mark.parametrize("shape", [(23, 37), (6, 9, 21)])
def test_hit_or_miss_with_both_structures_and_origins(gpu, ndi, shape):
    nd = len(shape)
    rng = np.random.default_rng(nd + 40)
    for dtype in ("bool", "int32", "float32"):
        x = _with_edges(shape, dtype, nd)
        for s1shape, s2shape, o1, o2 in [((3,) * nd, (3,) * nd, 0, None), ((3,) * nd, (3,) * nd, [1] + [0] * (nd - 1), [0] * (nd - 1) + [-1]),
                                         ((2,) * nd, (4,) + (2,) * (nd - 1), -1, [-2] + [0] * (nd - 1)), ((1, 2, 3)[:nd], (5,) * nd, 0, 2)]:
            st1 = rng.random(s1shape) > 0.6
            st2 = rng.random(s2shape) > 0.8
            got = ndi.binary_hit_or_miss(gpu.asarray(x), st1, st2, origin1=o1, origin2=o2)
            want = br.hit_or_miss(x, st1, st2, o1, o2)
            assert np.array_equal(want, sndi.binary_hit_or_miss(x.astype(np.float32) if dtype == "float16" else x, st1, st2, origin1=o1, origin2=o2))
            _same(got, want, (shape, dtype, s1shape, s2shape, o1, o2))
        _same(ndi.binary_hit_or_miss(gpu.asarray(x)), br.hit_or_miss(x), (shape, dtype, "defaults"))


def _reset_last_kernel(gpu, ndi):
    ndi.binary_erosion(gpu.asarray(np.ones((2, 2, 2, 2), np.int16)))
    assert "binary_erosion_kernel" in _lk()


def test_minkowski_root_rewrite_and_its_limits(gpu, ndi, lib):
    lib.mi_debug_set_bitmorph(2, 0, 0)              # the bit kernel at this small size too
    shape = (9, 11, 80)
    rng = np.random.default_rng(64)
    x = (rng.random(shape) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8)
    sparse = (rng.random(shape) < 0.01)
    mask = rng.random(shape) > 0.2
    cube, octa = np.ones((5, 5, 5), bool), np.abs(np.indices((5, 5, 5)) - 2).sum(0) <= 2
    for st, root in ((cube, ",cube3"), (octa, ",cross")):
        for name, data in (("erosion", x), ("dilation", sparse)):
            fn, ref = getattr(ndi, "binary_" + name), getattr(br, name)
            for bv in (0, 1):
                _reset_last_kernel(gpu, ndi)
                _same(fn(gpu.asarray(data), st, border_value=bv), ref(data, st, border_value=bv), (name, root, bv))
                assert "bitmorph3_kernel" in _lk() and root in _lk(), _lk()
            # not a Minkowski power any more / an origin / a mask: taken as given
            broken = st.copy()
            broken[tuple(np.argwhere(st)[0])] = False
            for kw, mref in ((dict(structure=broken), None), (dict(structure=st, origin=(1, 0, -1)), None),
                             (dict(structure=st, mask=gpu.asarray(mask)), mask)):
                _reset_last_kernel(gpu, ndi)
                got = fn(gpu.asarray(data), **kw)
                assert root not in _lk(), (kw.keys(), _lk())
                _same(got, ref(data, kw["structure"], 1, mref, 0, kw.get("origin", 0)), (name, root, sorted(kw)))
    # iterations x r either side of the limit of 64
    for it, rewritten in ((32, True), (33, False)):
        _reset_last_kernel(gpu, ndi)
        got = ndi.binary_dilation(gpu.asarray(sparse), octa, iterations=it)
        assert (",cross" in _lk()) == rewritten, (it, _lk())
        _same(got, br.dilation(sparse, octa, it), ("limit", it))
        _same(ndi.binary_erosion(gpu.asarray(x), cube, iterations=it, border_value=1), br.erosion(x, cube, it, border_value=1), ("limit", it))


def _serpentine(shape):
    """(seed, mask): a corridor that crosses the plane y = 15 | 16 once per column pair, so that a propagation along it
    cannot be finished by a few block-wise fill launches"""
    mask = np.zeros(shape, bool)
    seed = np.zeros(shape, bool)
    cols = list(range(0, shape[2], 2))
    for i, cx in enumerate(cols):
        mask[0, 13:19, cx] = True
        if i + 1 < len(cols):
            mask[0, 18 if i % 2 == 0 else 13, cx:cx + 3] = True
    seed[0, 13, 0] = True
    return seed, mask


def test_until_stable_into_an_unaligned_output_ends(gpu, ndi, lib):
    """Regression: a C-contiguous `output` one byte into its allocation.  The first launch (src -> scratch) is taken by the
    fill / fused kernel, the second (scratch -> output) is refused for its alignment; the loop used to retry that launch for
    ever (morphology._run_until_stable now goes on with single iterations; CPU proof in tests/test_host_logic.py)."""
    lib.mi_debug_set_bitmorph(2, 0, 0)
    shape = (12, 20, 96)
    n = int(np.prod(shape))
    seed, mask = _serpentine(shape)
    count = []
    want = br.propagation(seed, mask=mask, count=count)
    assert count[0] >= 3 * 4 and want.sum() == mask.sum()         # at least three launches' worth of iterations
    buf = gpu.asarray(np.full(n + 64, 0xA5, np.uint8))
    view = buf[1:1 + n].reshape(shape)
    assert view.ptr % 16 == 1 and view._is_c_contiguous()
    assert ndi.binary_propagation(gpu.asarray(seed), mask=gpu.asarray(mask), output=view) is view
    host = buf.get()
    assert np.array_equal(host[1:1 + n].reshape(shape), want.astype(np.uint8))
    assert host[0] == 0xA5 and (host[1 + n:] == 0xA5).all()
    # the same through the fused mode: an erosion until stable
    solid = np.ones(shape, np.uint8)
    count = []
    want = br.erosion(solid, iterations=-1, count=count)
    assert count[0] > 4 and not want.any()
    buf = gpu.asarray(np.full(n + 64, 0xA5, np.uint8))
    view = buf[1:1 + n].reshape(shape)
    assert ndi.binary_erosion(gpu.asarray(solid), iterations=-1, output=view) is view
    host = buf.get()
    assert not host[1:1 + n].any() and host[0] == 0xA5 and (host[1 + n:] == 0xA5).all()


def test_empty_zero_d_and_rank_mismatch_as_scipy(gpu, ndi):
    for shape in ((0,), (3, 0), (0, 4, 5)):
        x = np.zeros(shape, np.uint8)
        for name in ("binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "binary_propagation", "binary_fill_holes"):
            want = getattr(sndi, name)(x)
            got = getattr(ndi, name)(gpu.asarray(x)).get()
            assert got.shape == want.shape and got.dtype == want.dtype, (name, shape)
    for v in (0.0, 2.5, np.nan):
        x = np.array(v)
        for name in ("binary_erosion", "binary_dilation"):
            want = getattr(sndi, name)(x)
            # (asarray of a 0-d host array gives one element of rank 1, DESIGN.md: the 0-d view is taken on the device)
            got = getattr(ndi, name)(gpu.asarray(x.reshape(1)).reshape(())).get()
            assert got.shape == () and got.dtype == want.dtype and bool(got) == bool(want), (name, v)
    x = np.ones((4, 5), np.uint8)
    for name in ("binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "binary_hit_or_miss", "binary_propagation", "binary_fill_holes"):
        for st in (np.ones(3, bool), np.ones((3, 3, 3), bool)):
            # SciPy's dilation indexes the structure's shape by the input's axes before it compares the ranks: an
            # IndexError for a structure of lower rank; here every function raises the RuntimeError
            with pytest.raises((RuntimeError, IndexError)):
                getattr(sndi, name)(x, st)
            with pytest.raises(RuntimeError):
                getattr(ndi, name)(gpu.asarray(x), st)
    with pytest.raises(RuntimeError):
        sndi.binary_erosion(x, np.ones((0, 3), bool))
    with pytest.raises(RuntimeError):
        ndi.binary_erosion(gpu.asarray(x), np.ones((0, 3), bool))
