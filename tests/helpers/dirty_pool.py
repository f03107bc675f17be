"""Poisoned pool memory (mi_debug_set_pool_fill, csrc/runtime.hip): every block the caching pool hands out -- outputs made
by `empty`, scratch made by pool_alloc, fresh or recycled -- is first filled with one byte.  A kernel that leaves part of its
output unwritten, or reads scratch before it has written it, then answers differently under different fill bytes; with the
knob off such a kernel usually finds zeros or the right answer of the call before in that memory.

`CASES` is the table tests/test_gpu_dirty_pool.py walks: one entry per kernel family, route and small shape.  The inputs of a
case are uploaded BEFORE the knob goes on (only outputs and temporaries are poisoned); `run_filled` then runs the case once
per byte of `FILLS` and returns what it produced as host arrays.

The three bytes: 0xFF is a NaN in every float format, -1 or the maximum in the integer ones and neither 0 nor 1 as a bool;
0x55 is a large positive finite value (1.47e13 as float32, 1.2e103 as float64, 85 as uint8); 0xD5 is a large negative one.
fmin / fmax swallow a NaN, and a minimum or maximum swallows garbage of one sign, so one pattern alone would not show in the
min / max and rank families.

The references and tolerances are the families' own: the CPU oracle and SciPy with the bounds of tests/test_gpu_vs_oracle.py,
and the host transcriptions of tests/helpers/*_ref.py, bit for bit where the family's module compares bit for bit."""
import contextlib
import ctypes

import numpy as np

FILLS = (0xFF, 0x55, 0xD5)


@contextlib.contextmanager
def pool_fill(gpu, byte):
    """every block the pool hands out inside the `with` is filled with `byte`; the knob is always cleared again"""
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_set_pool_fill
    fn.argtypes = [ctypes.c_int, ctypes.c_int]
    assert fn(1, int(byte)) == 0
    try:
        yield
    finally:
        fn(0, 0)
        gpu.synchronize()


def flatten(result):
    """every array and scalar a call produced, as host arrays in a fixed order (None entries are kept out)"""
    out = []

    def walk(v):
        if v is None:
            return
        if isinstance(v, dict):
            for k in sorted(v):
                walk(v[k])
        elif isinstance(v, (list, tuple)):
            for e in v:
                walk(e)
        elif isinstance(v, np.ndarray) and v.dtype == object:
            for e in v.ravel():
                walk(e)
        elif hasattr(v, "get") and hasattr(v, "ptr"):
            out.append(np.ascontiguousarray(v.get()))
        else:
            out.append(np.ascontiguousarray(np.asarray(v)))
    walk(result)
    return out


class Case:
    def __init__(self, name, inputs, call, ref, compare, knobs=(), route=None, uses_got=False, ref_key=None):
        self.name = name
        self.ref_key = name if ref_key is None else ref_key      # cases with one key share one computed reference
        self.uses_got = uses_got      # the reference is computed from part of the device's own result: ref(*host, got=[arrays])
        self.inputs = inputs          # () -> tuple of host arrays
        self.call = call              # (gpu, *device arrays) -> arrays / scalars (nested lists, tuples, dicts)
        self.ref = ref                # (*host arrays) -> the same structure, from the family's reference
        self.compare = compare        # (got array, reference array) -> None, raises; the family's own comparison, or a list
                                      # of them, one per output, where the family holds its outputs to different bounds
        self.knobs = knobs            # ((setter name, args that select the route, args that restore the default), ...)
        self.route = route            # text (or texts) last_kernel() must hold after the call, or None

    def __repr__(self):
        return self.name


@contextlib.contextmanager
def _knobs(case):
    from cupyimg_amd import _lib
    lib = _lib.load()
    try:
        for name, on, _ in case.knobs:
            assert getattr(lib, name)(*[ctypes.c_int(v) for v in on]) == 0
        yield
    finally:
        for name, _, off in case.knobs:
            getattr(lib, name)(*[ctypes.c_int(v) for v in off])


def run_filled(gpu, case):
    """({fill byte: [host arrays]}, {fill byte: last_kernel()}, host inputs) of one case"""
    host = tuple(case.inputs())
    dev = tuple(gpu.asarray(h) if isinstance(h, np.ndarray) else h for h in host)      # before the knob: inputs stay clean
    gpu.synchronize()
    outs, routes = {}, {}
    # last_kernel() keeps the name of the last launch that noted one: a tiny launch of a kernel no case ends on marks "none"
    mark = gpu.asarray(np.ones((2, 2, 2, 2), np.int16))
    with _knobs(case):
        for byte in FILLS:
            _ndi().binary_erosion(mark)
            with pool_fill(gpu, byte):
                outs[byte] = flatten(case.call(gpu, *dev))
                name = gpu.last_kernel()
                routes[byte] = "" if "binary_erosion_kernel<int16" in name else name
    return outs, routes, host


_REFERENCES = {}


def reference(case, host, got):
    """the reference's result as host arrays; computed once per `ref_key` (the cases that name the same key differ in nothing
    but their knobs: the same reference on the same inputs) and left unchanged"""
    if case.uses_got:
        return flatten(case.ref(*host, got=got))
    if case.ref_key not in _REFERENCES:
        want = flatten(case.ref(*host))
        for w in want:
            w.setflags(write=False)
        _REFERENCES[case.ref_key] = want
    return _REFERENCES[case.ref_key]


# ------------------------------------------------------------------ comparisons (the families' own)
def exact(got, want):
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want, equal_nan=got.dtype.kind == "f"):
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).ravel())
        raise AssertionError("{} of {} differ, first at {}: {} != {}".format(bad.size, got.size, bad[0], got.ravel()[bad[0]],
                                                                             want.ravel()[bad[0]]))


def exact_values(got, want):
    """equal values; the reference may come in another dtype (SciPy's int64 where the device answers in the input's)"""
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want.astype(got.dtype)), int((got != want.astype(got.dtype)).sum())


def same_bits(got, want):
    from test_gpu_edges import same_bits as sb
    assert sb(got, np.asarray(want)), "bits differ"


def maxnorm(tol):
    """max|y - ref| <= tol * max|ref| (tests/_cases.py maxnorm_rel, the bound of the fused float32 filters)"""
    def cmp(got, want):
        from _cases import maxnorm_rel
        assert got.shape == np.shape(want), (got.shape, np.shape(want))
        r = maxnorm_rel(got, np.asarray(want))
        assert r <= tol, r
    return cmp


def scaled(tol):
    """max|y - ref| <= tol * max(1, max|ref|) (the interpolation bounds of tests/test_gpu_vs_oracle.py)"""
    def cmp(got, want):
        want = np.asarray(want, np.float64)
        assert got.shape == want.shape, (got.shape, want.shape)
        err = float(np.abs(got.astype(np.float64) - want).max()) if want.size else 0.0
        assert err <= tol * max(1.0, float(np.abs(want).max()) if want.size else 0.0), err
    return cmp


def close(rtol, atol):
    def cmp(got, want):
        np.testing.assert_allclose(got, np.asarray(want), rtol=rtol, atol=atol)
    return cmp


def below(bound):
    """|got - want| < bound, for the scalars a family's module holds to `abs(got - want) < bound`"""
    def cmp(got, want):
        assert got.shape == np.shape(want), (got.shape, np.shape(want))
        err = float(np.abs(got.astype(np.float64) - np.asarray(want, np.float64)).max())
        assert err < bound, err
    return cmp


# ------------------------------------------------------------------ the table
CASES = []


def _add(name, inputs, call, ref, compare, knobs=(), route=None, uses_got=False, ref_key=None):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, inputs, call, ref, compare, tuple(knobs), route, uses_got, ref_key))


def _ndi():
    from cupyimg_amd.scipy import ndimage
    return ndimage


def _orc():
    from oracle import ndimage as orc
    return orc


def _sndi():
    import scipy.ndimage as sndi
    return sndi


def _f32(shape, seed):
    return lambda: (np.random.default_rng(seed).standard_normal(shape).astype(np.float32),)


def _f64(shape, seed):
    return lambda: (np.random.default_rng(seed).standard_normal(shape),)


def _ints(shape, seed, dtype, lo=None, hi=None):
    def make():
        info = np.iinfo(dtype)
        return (np.random.default_rng(seed).integers(info.min if lo is None else lo, (info.max if hi is None else hi) + 1,
                                                     size=shape).astype(dtype),)
    return make


def _bools(shape, seed, p=0.6):
    return lambda: (np.random.default_rng(seed).random(shape) < p,)


def _filter(name, fn, inputs, compare, knobs=(), route=None, ref_mod=_orc, **kw):
    """one ndimage filter call with keyword arguments, against the same call of the oracle (or SciPy)"""
    _add(name, inputs, lambda gpu, x: getattr(_ndi(), fn)(x, **kw), lambda x: getattr(ref_mod(), fn)(x, **kw), compare, knobs, route)


RAGGED_OFF = [("mi_debug_set_sep3d_ragged", (0,), (1,))]

# ---- separable float filters
_filter("sep/lean5-uniform", "uniform_filter", _f32((40, 37, 64), 3), maxnorm(1e-6), size=5, mode="reflect", cval=0.75)
_filter("sep/lean3-gaussian-constant", "gaussian_filter", _f32((9, 5, 8), 4), maxnorm(1e-6), sigma=0.5, mode="constant", cval=0.0)
_filter("sep/long17-gaussian", "gaussian_filter", _f32((36, 41, 96), 5), maxnorm(1e-6), route="sep3d_long", sigma=2.0, mode="mirror")
_filter("sep/long9-ragged", "uniform_filter", _f32((19, 23, 70), 6), maxnorm(1e-6), route="sep3d_long3_kernel<9,true,ragged>", size=9,
        mode="reflect")
_filter("sep/long9-extended-rows", "uniform_filter", _f32((19, 23, 70), 6), maxnorm(1e-6), knobs=RAGGED_OFF, size=9, mode="reflect")
# 11 taps: the long kernel (no running-sum box kernel exists: DESIGN.md 4.16)
_filter("sep/long11-uniform", "uniform_filter", _f32((40, 40, 40), 7), maxnorm(1e-6), size=11, mode="reflect")
_filter("sep/stream-21taps", "gaussian_filter", _f32((20, 21, 70), 8), maxnorm(1e-6), sigma=2.5, mode="wrap", cval=0.3)
_filter("sep/image2d", "gaussian_filter", _f32((96, 264), 9), maxnorm(1e-6), sigma=1.0, mode="mirror")
_filter("sep/image2d-ragged", "uniform_filter", _f32((37, 131), 10), maxnorm(1e-6), size=5, mode="nearest")
_filter("sep/lean5-ragged", "uniform_filter", _f32((19, 23, 70), 11), maxnorm(1e-6), route="ragged", size=5, mode="mirror")
_filter("sep/lean5-extended-rows", "uniform_filter", _f32((19, 23, 70), 11), maxnorm(1e-6), knobs=RAGGED_OFF, size=5, mode="mirror")
_filter("sep/lean7-ragged-constant", "gaussian_filter", _f32((9, 37, 67), 12), maxnorm(1e-6), sigma=0.7, mode="constant", cval=0.5)
_filter("sep/float64-stream", "gaussian_filter", _f64((20, 21, 37), 13), maxnorm(1e-12), sigma=1.0, mode="reflect")
_filter("sep/float64-uniform-image", "uniform_filter", _f64((33, 70), 14), maxnorm(1e-12), size=(3, 7), mode="wrap")
_filter("sep/uint8-uniform", "uniform_filter", _ints((12, 13, 37), 15, np.uint8), exact, size=3)
_filter("sep/int16-uniform-image", "uniform_filter", _ints((21, 67), 16, np.int16), exact, size=(4, 5), mode="nearest")
_filter("sep/rank4-uniform", "uniform_filter", _f32((4, 5, 6, 7), 17), maxnorm(1e-6), size=3)
_add("sep/correlate1d-float64", _f64((11, 67), 18),
     lambda gpu, x: _ndi().correlate1d(x, [1.0, -2.0, 0.5, 3.0, 1.5], axis=1, mode="mirror", dtype_mode="ndimage"),
     lambda x: _orc().correlate1d(x, [1.0, -2.0, 0.5, 3.0, 1.5], axis=1, mode="mirror"), exact)
_W131 = np.random.default_rng(19).standard_normal(131)
_add("sep/correlate1d-131taps", _f64((5, 3), 20), lambda gpu, x: _ndi().correlate1d(x, _W131, axis=1, mode="wrap", dtype_mode="ndimage"),
     lambda x: _orc().correlate1d(x, _W131, axis=1, mode="wrap"), exact)
_add("sep/correlate1d-float32-axis0", _f32((9, 37, 64), 21),
     lambda gpu, x: _ndi().correlate1d(x, [1.0, 2.0, 1.0], axis=0, mode="reflect"),
     lambda x: _orc().correlate1d(x, [1.0, 2.0, 1.0], axis=0, mode="reflect"), maxnorm(1e-6))

# ---- correlate / convolve
_W3 = np.random.default_rng(30).standard_normal((3, 3, 3))
_add("correlate/stencil3s", _f32((24, 40, 70), 31), lambda gpu, x: _ndi().correlate(x, _W3), lambda x: _orc().correlate(x, _W3).astype(np.float32),
     exact, route="stencil3s_kernel")
_add("correlate/stencil3", _f32((20, 21, 72), 31), lambda gpu, x: _ndi().correlate(x, _W3, mode="mirror"),
     lambda x: _orc().correlate(x, _W3, mode="mirror").astype(np.float32), exact, knobs=[("mi_debug_set_stencil_scatter", (0,), (1,))])
_add("convolve/stencil3s-constant", _f32((9, 10, 33), 32), lambda gpu, x: _ndi().convolve(x, _W3, mode="constant", cval=0.5),
     lambda x: _orc().convolve(x, _W3, mode="constant", cval=0.5).astype(np.float32), exact)
_add("correlate/generic-3d", _f32((9, 10, 33), 33), lambda gpu, x: _ndi().correlate(x, _W3, mode="wrap"),
     lambda x: _orc().correlate(x, _W3, mode="wrap").astype(np.float32), exact, knobs=[("mi_debug_set_stencil", (0,), (1,))])
_W4 = np.random.default_rng(34).standard_normal((2, 3, 1, 3))
_add("correlate/generic-rank4", _f32((4, 5, 6, 7), 35), lambda gpu, x: _ndi().correlate(x, _W4, mode="mirror"),
     lambda x: _orc().correlate(x, _W4, mode="mirror"), exact)
_W2 = np.array([[1, 0, 2], [0, 1, 0], [1, 0, -1]], dtype=np.float64)
_add("correlate/image-int16-to-int32", _ints((9, 67), 36, np.int16, -99, 99), lambda gpu, x: _ndi().correlate(x, _W2, output=np.dtype("int32")),
     lambda x: _orc().correlate(x, _W2, output="int32"), exact)


def _signal(name, a_shape, b_shape, dtype, mode, fn, tol):
    def inputs():
        rng = np.random.default_rng(160)
        if np.dtype(dtype).kind == "f":
            return rng.standard_normal(a_shape).astype(dtype), rng.standard_normal(b_shape).astype(dtype)
        return rng.integers(-9, 10, size=a_shape).astype(dtype), rng.integers(-9, 10, size=b_shape).astype(dtype)

    def call(gpu, a, b):
        from cupyimg_amd.scipy import signal
        return getattr(signal, fn)(a, b, mode=mode)

    def ref(a, b):
        import scipy.signal as ssig
        return getattr(ssig, fn)(a, b, mode=mode, method="direct")
    _add(name, inputs, call, ref, tol)


_signal("signal/convolve-full-float64", (17, 23), (4, 5), "float64", "full", "convolve", close(1e-12, 1e-12))
_signal("signal/correlate-same-float32", (9, 10, 11), (3, 2, 4), "float32", "same", "correlate", close(2e-6, 2e-5))
_signal("signal/convolve-valid-int32", (17, 23), (3, 3), "int32", "valid", "convolve", exact)

# ---- min / max and grey morphology (SciPy, exact)
U8_RAGGED_OFF = [("mi_debug_set_u8_ragged", (0,), (1,))]
S16_RAGGED_OFF = [("mi_debug_set_s16_ragged", (0,), (1,))]
_filter("minmax/uint8-fused-7", "grey_erosion", _ints((32, 40, 64), 40, np.uint8), exact, ref_mod=_sndi, size=7)
_filter("minmax/uint8-unfused-5", "grey_dilation", _ints((32, 40, 64), 41, np.uint8), exact, ref_mod=_sndi,
        knobs=[("mi_debug_set_u8_fused", (0,), (1,))], size=5)
_filter("minmax/uint8-ragged-5", "grey_erosion", _ints((24, 25, 70), 42, np.uint8), exact, ref_mod=_sndi, route="mm3u8_ragged_kernel", size=5,
        mode="reflect")
_filter("minmax/uint8-extended-rows-5", "grey_erosion", _ints((24, 25, 70), 42, np.uint8), exact, ref_mod=_sndi, knobs=U8_RAGGED_OFF, size=5,
        mode="reflect")
# 39420 bytes in a block of 39424: no 16 readable bytes after the array, the ragged kernel hands the rows on
_filter("minmax/uint8-ragged-block-end-3", "grey_dilation", _ints((20, 27, 73), 39, np.uint8), exact, ref_mod=_sndi, size=3)
_filter("minmax/int16-5", "grey_dilation", _ints((16, 24, 64), 43, np.int16), exact, ref_mod=_sndi, size=5)
_filter("minmax/uint16-ragged-3", "grey_erosion", _ints((24, 25, 70), 44, np.uint16), exact, ref_mod=_sndi, route="mm3s16_ragged_kernel", size=3,
        mode="mirror")
_filter("minmax/uint16-extended-rows-3", "grey_erosion", _ints((24, 25, 70), 44, np.uint16), exact, ref_mod=_sndi, knobs=S16_RAGGED_OFF, size=3,
        mode="mirror")
_filter("minmax/float32-fused-3", "maximum_filter", _f32((20, 21, 64), 45), exact, ref_mod=_sndi, size=3)
_filter("minmax/float32-stream-9", "minimum_filter", _f32((20, 21, 70), 46), exact, ref_mod=_sndi, size=9, mode="constant", cval=0.25)
_filter("minmax/float32-two-launches", "maximum_filter", _f32((20, 21, 64), 45), exact, ref_mod=_sndi,
        knobs=[("mi_debug_set_minmax_f32_fused", (0,), (1,))], size=3)
_filter("minmax/float64-stream-9", "maximum_filter", _f64((12, 13, 37), 47), exact, ref_mod=_sndi, size=9, mode="nearest")
_filter("minmax/float32-image-5", "minimum_filter", _f32((37, 131), 48), exact, ref_mod=_sndi, size=5)
_filter("minmax/rank4-passes", "maximum_filter", _f32((4, 5, 6, 7), 49), exact, ref_mod=_sndi, size=3)
_CROSS3 = np.abs(np.indices((3, 3, 3)) - 1).sum(0) <= 1
_DISK5 = (np.indices((5, 5)) - 2).__pow__(2).sum(0) <= 5
_filter("minmax/runs-cross-3x3x3", "grey_dilation", _f32((12, 20, 70), 50), exact, ref_mod=_sndi, footprint=_CROSS3)
_filter("minmax/runs-disk-2d", "grey_erosion", _ints((70, 96), 51, np.uint8), exact, ref_mod=_sndi, footprint=_DISK5, mode="mirror")
_filter("minmax/untiled-footprint", "grey_dilation", _f32((12, 20, 70), 50), exact, ref_mod=_sndi,
        knobs=[("mi_debug_set_minmax_tiled", (0,), (1,))], footprint=_CROSS3)
_STRUCT = np.random.default_rng(52).standard_normal((3, 3, 3))
_filter("minmax/nd-structure", "grey_dilation", _f64((9, 10, 33), 53), exact, ref_mod=_sndi, structure=_STRUCT)
_filter("minmax/nd-structure-erosion-2d", "grey_erosion", _f64((21, 67), 54), exact, ref_mod=_sndi, structure=_STRUCT[0], mode="wrap")


def _grey_fuzz_cases(count=100):
    """the first `count` cases of the grey-morphology draw (tests/helpers/grey_ref.py) that take a window with holes or a
    structure, against the draw's own reference: the generic kernels of csrc/minmax.hip at every rank, dtype and output form.
    Every other case of rank <= 3 runs outside the rank <= 3 geometry (minmax_nd_kernel<3>)."""
    from helpers import grey_ref as gr
    picked = [(i, c) for i, c in enumerate(gr.drawn()) if c["wkind"] in ("holes", "structure", "footprint+structure") and not c["illegal"]]
    for k, (i, case) in enumerate(picked[:count]):
        generic3 = len(case["shape"]) <= 3 and k % 2 == 1
        route = None
        if gr.has_structure(case):
            route = "minmax_nd_kernel<8>" if len(case["shape"]) > 3 else "minmax_nd_kernel<3>" if generic3 else "minmax3_kernel"

        def call(gpu, x, case=case):
            ret, out, _ = gr.call(_ndi(), case, to_array=gpu.asarray, x=x)
            assert out is None or ret is out
            return ret
        _add("minmax/grey-fuzz-{:03d}-{}-rank{}-{}{}".format(i, case["func"], len(case["shape"]), case["dtype"], "-generic3" if generic3 else ""),
             lambda case=case: (case["x"].copy(),), call, lambda x, case=case: gr.reference(case), exact, knobs=[("mi_debug_set_minmax_fast3", (0,), (1,))] if generic3 else (), route=route)


_grey_fuzz_cases()
for _fn in ("morphological_gradient", "morphological_laplace", "white_tophat", "black_tophat"):
    _filter("minmax/" + _fn + "-uint8", _fn, _ints((12, 20, 70), 55, np.uint8), exact, ref_mod=_sndi, size=3)
    _filter("minmax/" + _fn + "-float32", _fn, _f32((9, 10, 33), 56), exact, ref_mod=_sndi, size=(3, 5, 3))

# ---- rank filters (SciPy, exact)
_filter("rank/median3x3", "median_filter", _ints((40, 64), 60, np.uint8), exact, ref_mod=_sndi, size=3)
_filter("rank/median3x3-ragged", "median_filter", _ints((37, 67), 61, np.uint8), exact, ref_mod=_sndi, size=3, mode="mirror")
_filter("rank/median3x3-float32-ragged", "median_filter", _f32((21, 131), 62), exact, ref_mod=_sndi, size=3)
_filter("rank/median3x3-uint16-ragged", "median_filter", _ints((21, 67), 59, np.uint16), exact, ref_mod=_sndi, size=3, mode="nearest")
_filter("rank/median3x3-float64", "median_filter", _f64((21, 64), 58), exact, ref_mod=_sndi, size=3, mode="constant", cval=0.5)
_filter("rank/median3x3-planes", "median_filter", _f32((5, 21, 64), 57), exact, ref_mod=_sndi, size=(1, 3, 3))
_filter("rank/median27-shared-sort", "median_filter", _f32((12, 20, 70), 63), exact, ref_mod=_sndi, route="median27_stream_kernel", size=3)
_filter("rank/median27-uint8", "median_filter", _ints((12, 20, 64), 64, np.uint8), exact, ref_mod=_sndi, size=3, mode="constant", cval=7)
_filter("rank/median27-per-voxel", "median_filter", _f32((12, 20, 70), 63), exact, ref_mod=_sndi, knobs=[("mi_debug_set_median27", (0,), (1,))],
        size=3)
_filter("rank/rank27", "rank_filter", _ints((9, 10, 33), 65, np.int16), exact, ref_mod=_sndi, rank=5, size=3)
_filter("rank/network16", "median_filter", _f32((21, 67), 66), exact, ref_mod=_sndi, size=(3, 5))
_filter("rank/network32", "median_filter", _f32((21, 67), 67), exact, ref_mod=_sndi, size=5)
_filter("rank/network32-full", "median_filter", _f32((21, 67), 67), exact, ref_mod=_sndi, knobs=[("mi_debug_set_rank_median", (0,), (1,))], size=5)
_filter("rank/network64", "rank_filter", _f32((9, 12, 33), 68), exact, ref_mod=_sndi, rank=11, size=(3, 3, 5), mode="wrap")
_filter("rank/network128", "median_filter", _f32((9, 12, 33), 69), exact, ref_mod=_sndi, size=5)
_filter("rank/beyond128", "median_filter", _f32((9, 10, 17), 70), exact, ref_mod=_sndi, size=(5, 6, 6), mode="reflect")
_filter("rank/selection", "rank_filter", _ints((9, 12, 33), 71, np.uint8), exact, ref_mod=_sndi, knobs=[("mi_debug_set_rank_sorted", (0,), (1,))],
        rank=-2, size=3)
_filter("rank/rank4", "median_filter", _f32((4, 5, 6, 7), 72), exact, ref_mod=_sndi, size=(1, 3, 3, 3), mode="nearest")
_filter("rank/percentile", "percentile_filter", _f32((21, 67), 73), exact, ref_mod=_sndi, percentile=30, size=3)

# ---- binary morphology (SciPy, exact)
BYTES = [("mi_debug_set_bitmorph", (0, 0, 0), (1, 0, 0))]
BITS = [("mi_debug_set_bitmorph", (2, 0, 0), (1, 0, 0))]
_filter("binary/byte-erosion", "binary_erosion", _bools((20, 30, 40), 80), exact, ref_mod=_sndi, knobs=BYTES, iterations=2)
_filter("binary/byte-generic", "binary_dilation", _bools((20, 30, 40), 81, 0.2), exact, ref_mod=_sndi,
        knobs=BYTES + [("mi_debug_set_binary_tiled", (0,), (1,))], border_value=1)
_filter("binary/byte-ragged", "binary_erosion", _bools((9, 11, 37), 82), exact, ref_mod=_sndi, knobs=BYTES, border_value=1)
_filter("binary/byte-image", "binary_dilation", _bools((37, 67), 83, 0.2), exact, ref_mod=_sndi,
        knobs=[("mi_debug_set_bitmorph_2d", (0,), (1,))], iterations=2)
_filter("binary/int16-input", "binary_erosion", _ints((6, 9, 21), 84, np.int16, 0, 1), exact, ref_mod=_sndi, iterations=3)
_filter("binary/bits-fused-3", "binary_erosion", _bools((64, 64, 64), 85, 0.7), exact, ref_mod=_sndi, route="bitmorph3_kernel", iterations=3)
_filter("binary/bits-small", "binary_dilation", _bools((9, 11, 80), 86, 0.1), exact, ref_mod=_sndi, knobs=BITS, route="bitmorph3_kernel",
        iterations=2)
_filter("binary/bits-ragged", "binary_erosion", _bools((9, 11, 70), 87, 0.7), exact, ref_mod=_sndi, knobs=BITS, iterations=2, border_value=1)
_filter("binary/bits-ragged-off", "binary_erosion", _bools((9, 11, 70), 87, 0.7), exact, ref_mod=_sndi,
        knobs=BITS + [("mi_debug_set_bitmorph_ragged", (0,), (1,))], iterations=2, border_value=1)
_filter("binary/bits-image", "binary_erosion", _bools((70, 96), 88, 0.8), exact, ref_mod=_sndi, knobs=BITS, iterations=2)
_filter("binary/bits-table", "binary_dilation", _bools((9, 11, 80), 86, 0.1), exact, ref_mod=_sndi,
        knobs=BITS + [("mi_debug_set_bitmorph_table", (1,), (0,))])
_filter("binary/opening", "binary_opening", _bools((20, 30, 64), 89, 0.7), exact, ref_mod=_sndi)
_filter("binary/closing-image", "binary_closing", _bools((37, 67), 90, 0.4), exact, ref_mod=_sndi, iterations=2)
_filter("binary/hit-or-miss", "binary_hit_or_miss", _bools((9, 11, 37), 91), exact, ref_mod=_sndi)
_filter("binary/erosion-until-stable", "binary_erosion", _bools((12, 20, 96), 92, 0.9), exact, ref_mod=_sndi, knobs=BITS, iterations=-1)


def _seed_mask(shape, seed):
    def make():
        rng = np.random.default_rng(seed)
        mask = _sndi().binary_dilation(rng.random(shape) < 0.08, iterations=2)
        return mask & (rng.random(shape) < 0.02), mask
    return make


def _shell(shape, seed):
    def make():
        g = np.indices(shape).astype(np.float64)
        r = sum((g[d] - (shape[d] - 1) / 2.0) ** 2 / (0.45 * shape[d]) ** 2 for d in range(len(shape)))
        sh = (r < 1.0) & (r > 0.55) & (np.random.default_rng(seed).random(shape) > 0.003)
        return (sh,)
    return make


for _tag, _kn in (("bitfill", BITS), ("no-bitfill", BITS + [("mi_debug_set_bitfill", (0,), (1,))]), ("bytes", BYTES)):
    _add("binary/propagation-" + _tag, _seed_mask((12, 20, 96), 93), lambda gpu, s, m: _ndi().binary_propagation(s, mask=m),
         lambda s, m: _sndi().binary_propagation(s, mask=m), exact, knobs=_kn)
    _add("binary/fill-holes-" + _tag, _shell((24, 28, 64), 94), lambda gpu, x: _ndi().binary_fill_holes(x),
         lambda x: _sndi().binary_fill_holes(x), exact, knobs=_kn)
_add("binary/propagation-image", _seed_mask((37, 67), 95), lambda gpu, s, m: _ndi().binary_propagation(s, mask=m),
     lambda s, m: _sndi().binary_propagation(s, mask=m), exact)
_add("binary/fill-holes-image", _shell((37, 67), 96), lambda gpu, x: _ndi().binary_fill_holes(x), lambda x: _sndi().binary_fill_holes(x), exact)
_add("binary/dilation-masked-until-stable-rank4", _seed_mask((4, 5, 6, 9), 97),
     lambda gpu, s, m: _ndi().binary_dilation(s, iterations=-1, mask=m), lambda s, m: _sndi().binary_dilation(s, iterations=-1, mask=m), exact)

# ---- interpolation (SciPy in float64; the bounds of tests/test_gpu_vs_oracle.py: 2e-6 orders 0 / 1, 2e-5 cubic float32, 1e-11 float64)
_A = np.deg2rad(11.0)
M_GENERAL = np.array([[1.0, 0.05, 0.0], [-0.05, 1.0, 0.02], [0.03, 0.0, 0.98]])
M_ZDEC = np.array([[0.9, 0, 0], [0, 1.03 * np.cos(_A), -np.sin(_A)], [0, np.sin(_A), 0.97 * np.cos(_A)]])       # axis 0 decoupled: z-stream
M_ROWB = np.array([[1.03 * np.cos(_A), -np.sin(_A), 0], [np.sin(_A), 0.97 * np.cos(_A), 0], [0, 0, 1.0]])       # x to itself: row-blend
OFF3 = np.array([0.5, -1.25, 2.0])


def _affine(name, inputs, M, off, compare, knobs=(), route=None, f64=True, **kw):
    def ref(x):
        return _sndi().affine_transform(x.astype(np.float64) if f64 and x.dtype.kind == "f" else x, M, off, **kw)
    _add(name, inputs, lambda gpu, x: _ndi().affine_transform(x, M, off, **kw), ref, compare, knobs, route)


# 20 x 30 x 40 is below the 2^18 output voxels from which the LDS-staged kernels are taken: whatever the matrix, these run the
# per-voxel kernels (the staged ones are the cases on BIG_OUT below)
for _mode in ("constant", "nearest"):
    _affine("interp/order1-small-general-" + _mode, _f32((20, 30, 40), 100), M_GENERAL, OFF3, scaled(2e-6), order=1, mode=_mode, cval=0.25)
    _affine("interp/order1-small-zdecoupled-matrix-" + _mode, _f32((20, 30, 40), 101), M_ZDEC, OFF3, scaled(2e-6), order=1, mode=_mode, cval=0.25)
    _affine("interp/order1-small-xfixed-matrix-" + _mode, _f32((20, 30, 40), 102), M_ROWB, OFF3, scaled(2e-6), order=1, mode=_mode, cval=0.25)
# the LDS-staged order-1 kernels (box, z-stream, row-blend) and the order-3 ones (box, z-factor, z-stream) are taken from 2^18
# output voxels on, rows a multiple of 4 samples: the smallest such output that is no multiple of a tile, from a small input
BIG_OUT = (50, 72, 76)
OFF_BIG = np.array([0.5, -1.25, 2.0])
_affine("interp/order1-lds-box-big", _f32((44, 60, 68), 100), M_GENERAL, OFF_BIG, scaled(2e-6), route="affine3d_lds_kernel", order=1, mode="constant",
        cval=0.25, output_shape=BIG_OUT)
_affine("interp/order1-zstream-big", _f32((44, 60, 68), 101), M_ZDEC, OFF_BIG, scaled(2e-6), route="axis 0 decoupled: streams along it", order=1, mode="constant", cval=0.25,
        output_shape=BIG_OUT)
_affine("interp/order1-rowblend-big", _f32((44, 60, 68), 102), M_ROWB, OFF_BIG, scaled(2e-6), route="rowblend", order=1, mode="constant", cval=0.25,
        output_shape=BIG_OUT)
_affine("interp/order1-round2-kernels", _f32((20, 30, 40), 100), M_GENERAL, OFF3, scaled(2e-6), knobs=[("mi_debug_set_interp_c1", (0,), (1,))],
        order=1, mode="constant", cval=0.25)
_affine("interp/order1-gather", _f32((20, 30, 40), 101), M_ZDEC, OFF3, scaled(2e-6),
        knobs=[("mi_debug_set_affine_zstream", (0,), (1,)), ("mi_debug_set_affine_rowblend", (0,), (1,)), ("mi_debug_set_interp_c1", (5,), (1,))],
        order=1, mode="constant", cval=0.25)
_affine("interp/order0-output-shape", _f32((20, 30, 40), 103), M_GENERAL, OFF3, scaled(2e-6), order=0, mode="grid-wrap", output_shape=(9, 37, 67))
_affine("interp/order1-image", _f32((50, 67), 104), np.array([[1.03 * np.cos(_A), -np.sin(_A)], [np.sin(_A), 0.97 * np.cos(_A)]]),
        np.array([3.5, -7.25]), scaled(2e-6), order=1, mode="reflect", output_shape=(33, 70))
_affine("interp/order1-generic-double", _f32((9, 12, 14), 105), M_GENERAL, OFF3, scaled(2e-6), knobs=[("mi_debug_set_interp_generic", (1,), (0,))],
        order=1, mode="mirror")
_affine("interp/order1-rank4", _f64((4, 5, 6, 7), 106), np.diag([1.0, 0.9, 1.1, 0.95]) + 0.02, np.array([0.1, -0.2, 0.3, 0.0]), scaled(1e-11),
        order=1, mode="nearest")


def _coords(shape, seed, scale=1.0):
    def make():
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(shape).astype(np.float32)
        idx = np.indices(shape).reshape(len(shape), -1).astype(np.float64)
        c = (M_GENERAL[:len(shape), :len(shape)] @ idx + OFF3[:len(shape), None]).reshape((len(shape),) + shape) * scale
        return x, c
    return make


for _tag, _kn in (("small", ()), ("small-zstream-off", [("mi_debug_set_map_zstream", (0,), (1,))])):
    _add("interp/map-coordinates-order1-" + _tag, _coords((20, 30, 40), 107),
         lambda gpu, x, c: _ndi().map_coordinates(x, c, order=1, mode="constant", cval=-1.0),
         lambda x, c: _sndi().map_coordinates(x.astype(np.float64), c, order=1, mode="constant", cval=-1.0), scaled(2e-6), knobs=_kn)
_add("interp/map-coordinates-order1-zstream-big", lambda: tuple(a.astype(np.float32) if k else a for k, a in enumerate(_coords(BIG_OUT, 107)())),
     lambda gpu, x, c: _ndi().map_coordinates(x, c, order=1, mode="constant", cval=-1.0),
     lambda x, c: _sndi().map_coordinates(x.astype(np.float64), c.astype(np.float64), order=1, mode="constant", cval=-1.0), scaled(2e-6),
     route="zstream")
for _order in (2, 3, 4, 5):
    _add("interp/map-coordinates-order{}-float64".format(_order), lambda: (np.random.default_rng(108).standard_normal((9, 10, 11)),
                                                                              np.random.default_rng(109).uniform(-1, 10, size=(3, 50))),
         lambda gpu, x, c, o=_order: _ndi().map_coordinates(x, c, order=o, mode="mirror"),
         lambda x, c, o=_order: _sndi().map_coordinates(x, c, order=o, mode="mirror"), scaled(1e-11))

CUBIC_OFF = [("mi_debug_set_cubic_zstream", (0,), (1,)), ("mi_debug_set_cubic_box", (0,), (1,)), ("mi_debug_set_cubic_rowblend", (0,), (1,))]
_affine("interp/cubic-small-general", _f32((20, 30, 40), 110), M_GENERAL, OFF3, scaled(2e-5), order=3, mode="constant", cval=0.5)
_affine("interp/cubic-small-zdecoupled-matrix", _f32((20, 30, 40), 111), M_ZDEC, OFF3, scaled(2e-5), order=3, mode="mirror")
_affine("interp/cubic-small-zdecoupled-matrix-zfactor-off", _f32((20, 30, 40), 111), M_ZDEC, OFF3, scaled(2e-5), knobs=[("mi_debug_set_cubic_zfactor", (0,), (1,))], order=3,
        mode="mirror")
_affine("interp/cubic-small-xfixed-matrix", _f32((20, 30, 40), 112), M_ROWB, OFF3, scaled(2e-5), order=3, mode="nearest")
_affine("interp/cubic-gather", _f32((20, 30, 40), 110), M_GENERAL, OFF3, scaled(2e-5), knobs=CUBIC_OFF, order=3, mode="constant", cval=0.5)
_affine("interp/cubic-separable-diagonal", _f32((20, 30, 40), 113), np.array([0.9, 1.1, 0.8]), OFF3, scaled(2e-5), order=3, mode="reflect",
        output_shape=(22, 27, 50))
_affine("interp/cubic-separable-r3-passes", _f32((20, 30, 40), 113), np.array([0.9, 1.1, 0.8]), OFF3, scaled(2e-5),
        knobs=[("mi_debug_set_resample_fast", (0,), (1,))], order=3, mode="reflect", output_shape=(22, 27, 50))
_affine("interp/cubic-strip", _f32((20, 30, 40), 113), np.array([0.9, 1.1, 0.8]), OFF3, scaled(2e-5),
        knobs=[("mi_debug_set_cubic_separable", (0,), (1,))], order=3, mode="reflect")
_affine("interp/cubic-box-big", _f32((44, 60, 68), 110), M_GENERAL, OFF_BIG, scaled(2e-5), route="cubic3_box_kernel", order=3, mode="constant",
        cval=0.5, output_shape=BIG_OUT)
_affine("interp/cubic-zfactor-big", _f32((44, 60, 68), 111), M_ZDEC, OFF_BIG, scaled(2e-5), route="cubic3_zfactor_kernel", order=3, mode="mirror",
        output_shape=BIG_OUT)
_affine("interp/cubic-zstream-big", _f32((44, 60, 68), 111), M_ZDEC, OFF_BIG, scaled(2e-5), knobs=[("mi_debug_set_cubic_zfactor", (0,), (1,))],
        route="cubic3_zstream_kernel", order=3, mode="mirror", output_shape=BIG_OUT)
_affine("interp/cubic-rowblend-big", _f32((44, 60, 68), 112), M_ROWB, OFF_BIG, scaled(2e-5), route="rowblend", order=3, mode="nearest",
        output_shape=BIG_OUT)
_affine("interp/cubic-float64", _f64((9, 12, 14), 114), M_GENERAL, OFF3, scaled(1e-11), order=3, mode="mirror")
_affine("interp/order2-float32", _f32((9, 12, 14), 115), M_GENERAL, OFF3, scaled(2e-5), order=2, mode="nearest")

# rows of 140 coefficients (>= 2 tiles of 64) in 180 lines: mi_debug_set_spline_rows(2) takes the row kernels below 16384 lines
ROWS = ("mi_debug_set_spline_rows", (2,), (1,))
for _tag, _kn in (("rows-lds", [ROWS]), ("tiled", [ROWS, ("mi_debug_set_spline_rows_lds", (0,), (1,))]), ("fast", [("mi_debug_set_spline_fast", (2,), (1,))]),
                  ("thread-per-line", [("mi_debug_set_spline_rows", (0,), (1,)), ("mi_debug_set_spline_fast", (0,), (1,))]),
                  ("blocked", [("mi_debug_set_spline_chunk", (64,), (0,)), ("mi_debug_set_spline_fast", (0,), (1,))])):
    _add("interp/spline-filter-float32-" + _tag, _f32((9, 20, 300), 116),
         lambda gpu, x: _ndi().spline_filter(x, 3, output=np.float32, mode="mirror", allow_float32=True),
         lambda x: _sndi().spline_filter(x.astype(np.float64), 3, mode="mirror"),
         close(0, 2e-6 * float(np.abs(_f32((9, 20, 300), 116)()[0]).max())), knobs=_kn)      # 2e-6 max|x|, tests/test_gpu_vs_oracle.py
    _add("interp/spline-filter-float64-" + _tag, _f64((5, 9, 300), 117), lambda gpu, x: _ndi().spline_filter(x, 3, mode="mirror"),
         lambda x: _sndi().spline_filter(x, 3, mode="mirror"), close(1e-11, 1e-11), knobs=_kn)
_add("interp/spline-filter1d-order5", _f64((21, 67), 118), lambda gpu, x: _ndi().spline_filter1d(x, 5, axis=0, mode="reflect"),
     lambda x: _sndi().spline_filter1d(x, 5, axis=0, mode="reflect"), close(1e-11, 1e-11))
_add("interp/zoom-cubic", _f32((13, 18, 22), 119), lambda gpu, x: _ndi().zoom(x, (1.5, 0.8, 1.3)),
     lambda x: _sndi().zoom(x.astype(np.float64), (1.5, 0.8, 1.3)), scaled(2e-5))
_add("interp/zoom-order1-image", _f32((37, 52), 120), lambda gpu, x: _ndi().zoom(x, 1.7, order=1, mode="nearest"),
     lambda x: _sndi().zoom(x.astype(np.float64), 1.7, order=1, mode="nearest"), scaled(2e-6))
_add("interp/shift-cubic", _f32((13, 18, 22), 121), lambda gpu, x: _ndi().shift(x, (1.5, -2.25, 0.4), mode="grid-wrap"),
     lambda x: _sndi().shift(x.astype(np.float64), (1.5, -2.25, 0.4), mode="grid-wrap"), scaled(2e-5))
_add("interp/rotate-volume", _f32((13, 30, 34), 122), lambda gpu, x: _ndi().rotate(x, 17.0, reshape=False),
     lambda x: _sndi().rotate(x.astype(np.float64), 17.0, reshape=False), scaled(2e-5))
_add("interp/rotate-image-reshape", _f32((37, 52), 123), lambda gpu, x: _ndi().rotate(x, 30.0, order=1),
     lambda x: _sndi().rotate(x.astype(np.float64), 30.0, order=1), scaled(2e-6))
# integer images: an output every value of which is an integer in float64 (shifts by whole voxels, order 0 and 1), so that the
# rounding into the integer output has no tie to argue about
_add("interp/uint8-zoom-2", _ints((9, 12, 14), 124, np.uint8), lambda gpu, x: _ndi().zoom(x, 2.0, order=0),
     lambda x: _sndi().zoom(x, 2.0, order=0), exact)
_add("interp/int16-shift-whole", _ints((9, 12, 14), 125, np.int16), lambda gpu, x: _ndi().shift(x, (1, -2, 3), order=1, mode="constant", cval=-7),
     lambda x: _sndi().shift(x, (1, -2, 3), order=1, mode="constant", cval=-7), exact)

# ---- label and the labelled measurements (SciPy, exact)
GENERIC_LABEL = [("mi_debug_set_label_generic", (1,), (0,))]
_S26 = np.ones((3, 3, 3), bool)
for _tag, _kn, _rt in (("tiles", (), "label_tile_kernel"), ("generic", GENERIC_LABEL, "label_connect_kernel")):
    _add("label/volume-" + _tag, _bools((12, 20, 70), 130, 0.35), lambda gpu, x: _ndi().label(x), lambda x: _sndi().label(x), exact_values,
         knobs=_kn, route=_rt)
    _add("label/volume-26-" + _tag, _bools((9, 37, 64), 131, 0.12), lambda gpu, x: _ndi().label(x, _S26), lambda x: _sndi().label(x, _S26),
         exact_values, knobs=_kn, route=_rt)
    _add("label/image-" + _tag, _bools((70, 96), 132, 0.5), lambda gpu, x: _ndi().label(x), lambda x: _sndi().label(x), exact_values, knobs=_kn,
         route=_rt)
_add("label/rank4", _bools((4, 5, 6, 7), 133, 0.4), lambda gpu, x: _ndi().label(x), lambda x: _sndi().label(x), exact_values,
     route="label_connect_kernel")
_add("label/int16-input", _ints((9, 10, 33), 134, np.int16, 0, 2), lambda gpu, x: _ndi().label(x), lambda x: _sndi().label(x), exact_values)


def _labelled(shape, seed, nlab, dtype=np.int16):
    """every value once (SciPy's choice among tied extrema is its sort's), integers (float64 sums are exact in any order)"""
    def make():
        rng = np.random.default_rng(seed)
        n = int(np.prod(shape))
        return (rng.permutation(n) - n // 2).reshape(shape).astype(dtype), rng.integers(0, nlab + 1, size=shape).astype(np.int32)
    return make


def _mirrored(shape, seed, nlab):
    """integers whose mean over every label is 0 (each value comes with its negative under the same label): the deviations
    from the mean and their squares are integers, so that the two-pass variance is the same float64 in any order of summation"""
    def make():
        rng = np.random.default_rng(seed)
        half = rng.integers(1, 300, size=shape).astype(np.float64)
        lab = rng.integers(0, nlab + 1, size=shape).astype(np.int32)
        lab.reshape(-1)[:nlab] = np.arange(1, nlab + 1)                # every label present
        return np.concatenate([half, -half]), np.concatenate([lab, lab])
    return make


def _noted(gpu, expect, value):
    """`value`, once the note of the launches behind it (last_kernel()) holds every text of `expect`"""
    if gpu is not None:
        note = gpu.last_kernel()
        for part in expect:
            assert part in note, (part, note)
    return value


def _measures(index, sums=(), com=()):
    """every labelled measurement of one index; on the device the sums, extrema and position passes must note `sums` (the
    atomics' route, the index route) and center_of_mass, which leaves LDS at a third of the slots in 3-D, `com`"""
    def call(gpu, x, lab, mod=None):
        m = _ndi() if mod is None else mod
        out = [_noted(gpu, ("M_SUMS",) + sums, m.sum_labels(x, lab, index)), m.mean(x, lab, index),
               _noted(gpu, ("M_EXT",) + sums, m.minimum(x, lab, index)), m.maximum(x, lab, index)]
        mn, mx, pmn, pmx = _noted(gpu, ("M_EXT",) + sums + ("M_POS",), m.extrema(x, lab, index))
        out += [mn, mx, np.asarray(pmn), np.asarray(pmx)]
        out += [np.asarray(m.minimum_position(x, lab, index)), np.asarray(m.maximum_position(x, lab, index))]
        out.append(np.asarray(_noted(gpu, ("M_COM",) + com, m.center_of_mass(x, lab, index)), np.float64))
        h = m.histogram(x, -500, 500, 16, lab, index)
        out.append(h)
        return out
    return call


def _measure_cmp(got, want):
    """integer data: float64 sums are exact; SciPy answers positions and extrema in its own integer types"""
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.astype(np.float64), want.astype(np.float64), equal_nan=True)


LDS, GLOBAL = "LDS atomics", "global atomics"
for _name, _index, _how in (("lut-6", list(range(1, 7)), "lut"), ("lut-unordered", [5, 2, 9, 1], "lut"), ("search-wide", [3, 1, 2 ** 20 + 5, 6], "search"),
                            ("scalar", 3, ""), ("none", None, "")):
    _add("measure/lds-atomics-" + _name, _labelled((9, 20, 33), 140, 6),
         lambda gpu, x, lab, i=_index, h=_how: _measures(i, (LDS, h), (LDS, h))(gpu, x, lab),
         lambda x, lab, i=_index: _measures(i)(None, x, lab, _sndi()), _measure_cmp)
# kLdsSlots = 1024 (csrc/measure.hip): one index value more and the sums, squared deviations and extrema go through global
# atomics; center_of_mass in 3-D leaves LDS above 682 slots already
_I1000, _I1025 = list(range(1, 1001)), list(range(1, 1026))
_add("measure/lds-atomics-1000-com-global", _labelled((12, 20, 70), 141, 1000),
     lambda gpu, x, lab: _measures(_I1000, (LDS, "lut"), (GLOBAL,))(gpu, x, lab), lambda x, lab: _measures(_I1000)(None, x, lab, _sndi()),
     _measure_cmp)
_add("measure/global-atomics-1025", _labelled((12, 20, 70), 141, 1025),
     lambda gpu, x, lab: _measures(_I1025, (GLOBAL, "lut"), (GLOBAL,))(gpu, x, lab), lambda x, lab: _measures(_I1025)(None, x, lab, _sndi()),
     _measure_cmp)


def _variances(index, route):
    half = len(index) // 2

    def call(gpu, x, lab, mod=None):
        m = _ndi() if mod is None else mod
        return [_noted(gpu, ("M_SSD", route), m.variance(x, lab, index[:half])),
                _noted(gpu, ("M_SSD", route), m.standard_deviation(x, lab, index[half:]))]
    return call


_add("measure/variance-lds-atomics", _mirrored((9, 20, 33), 142, 6), lambda gpu, x, lab: _variances(list(range(1, 7)), LDS)(gpu, x, lab),
     lambda x, lab: _variances(list(range(1, 7)), "")(None, x, lab, _sndi()), close(1e-12, 0))
# 2050 index values: 1025 slots for the variance and 1025 for the standard deviation
_I2050 = list(range(1, 2051))
_add("measure/variance-global-atomics", _mirrored((12, 20, 70), 144, 2050), lambda gpu, x, lab: _variances(_I2050, GLOBAL)(gpu, x, lab),
     lambda x, lab: _variances(_I2050, "")(None, x, lab, _sndi()), close(1e-12, 0))
_add("measure/histogram-plain", _f64((21, 67), 143), lambda gpu, x: _ndi().histogram(x, -2, 2, 32), lambda x: _sndi().histogram(x, -2, 2, 32),
     exact_values)


# ---- skimage
def _setting_knob(setter, off):
    return lambda *on: [(setter, on, off)]


def _skimage_cases():
    from helpers import corner_ref, edges_ref, exposure_ref, morphsnakes_ref, reconstruct_ref, ridge_ref, tv_ref, tvl1_ref

    # reconstruction: the planner's blocks, small blocks, the generic kernel
    rec = _setting_knob("mi_debug_set_reconstruct", (0, 0, 0))
    for tag, on in (("planner", (0, 0, 0)), ("small", (4, 5, 0)), ("generic", (0, 0, 1))):
        for shape, method, dtype in (((20, 37, 64), "dilation", "uint8"), ((5, 1040), "erosion", "float32"), ((9, 50, 130), "dilation", "int16")):
            def inputs(shape=shape, method=method, dtype=dtype):
                rng = reconstruct_ref.rng_for(shape, method, "box", dtype, "hdome")
                return reconstruct_ref.hdome_input(shape, dtype, method, rng)

            def call(gpu, seed, mask, method=method):
                from cupyimg_amd.skimage import morphology
                return morphology.reconstruction(seed, mask, method=method)
            _add("skimage/reconstruction-{}-{}-{}".format("x".join(map(str, shape)), method, tag), inputs, call,
                 lambda seed, mask, method=method: reconstruct_ref.reconstruct(seed, mask, method=method), exact, knobs=rec(*on),
                 ref_key=("reconstruction", shape, method))

    # total variation: fixed iteration counts, bit for bit
    tvk = _setting_knob("mi_debug_set_tv_chambolle", (0, 0, 0, 0))
    for tag, on in (("planner", (0, 0, 0, 0)), ("small", (3, 2, 1, 0)), ("generic", (0, 0, 0, 1))):
        for shape, dtype in (((12, 20, 70), "float32"), ((70, 96), "float64"), ((2, 5, 1040), "float32")):
            def call(gpu, x):
                from cupyimg_amd.skimage import restoration
                return restoration.denoise_tv_chambolle(x, weight=0.2, eps=0, n_iter_max=7)
            _add("skimage/tv-chambolle-{}-{}-{}".format("x".join(map(str, shape)), dtype, tag),
                 lambda shape=shape, dtype=dtype: (tv_ref.volume(shape, np.dtype(dtype), 1),), call,
                 lambda x: tv_ref.tv_chambolle(x, weight=0.2, eps=0.0, n_iter_max=7)[0], exact, knobs=tvk(*on), ref_key=("tv", shape, dtype))

    # ridge filters: the whole functions within 1e-6 max|reference| (tests/test_gpu_ridges.py, part 4); hessian_matrix against
    # the transcription on SciPy's Gaussian within the same bound
    rk = _setting_knob("mi_debug_set_ridges", (0, 0, 0))
    for tag, on in (("planner", (0, 0, 0)), ("small", (3, 2, 0)), ("generic", (0, 0, 1))):
        for fn, shape in (("meijering", (9, 67)), ("sato", (7, 9, 67)), ("frangi", (19, 23, 70))):
            def call(gpu, x, fn=fn):
                from cupyimg_amd.skimage import filters
                return getattr(filters, fn)(x, sigmas=(1, 2))
            _add("skimage/{}-{}-{}".format(fn, "x".join(map(str, shape)), tag), lambda shape=shape: (ridge_ref.volume(shape, np.float64, 1),), call,
                 lambda x, fn=fn: getattr(ridge_ref, fn)(x, sigmas=(1, 2)), maxnorm(1e-6), knobs=rk(*on), ref_key=("ridges", fn, shape))

        def hcall(gpu, x):
            from cupyimg_amd.skimage import feature
            return feature.hessian_matrix(x, sigma=1.0, mode="reflect", order="rc")

        def hwant0(x):
            # numpy.gradient twice on the device's own smoothed array, bit for bit (tests/test_gpu_ridges.py, part 1)
            import cupyimg_amd
            g = _ndi().gaussian_filter(cupyimg_amd.asarray(x), sigma=1.0, mode="reflect", cval=0).get()
            return ridge_ref.hessian_from_smoothed(g, "rc")
        for shape in ((19, 23, 70), (9, 67)):
            _add("skimage/hessian-matrix-{}-{}".format("x".join(map(str, shape)), tag), lambda shape=shape: (ridge_ref.volume(shape, np.float32, 1),),
                 hcall, hwant0, exact, knobs=rk(*on))

    # morphological snakes
    sk = _setting_knob("mi_debug_set_morphsnakes", (0, 0))
    for tag, on in (("planner", (0, 0)), ("small", (1, 0)), ("generic", (0, 1))):
        for shape, dtype, seed, smoothing in (((20, 37, 70), "float32", 1, 1), ((70, 96), "float32", 2, 2)):
            def call(gpu, x, smoothing=smoothing):
                from cupyimg_amd.skimage import segmentation
                return segmentation.morphological_chan_vese(x, 7, "checkerboard", smoothing=smoothing)
            _add("skimage/chan-vese-{}-{}".format("x".join(map(str, shape)), tag),
                 lambda shape=shape, dtype=dtype, seed=seed: (morphsnakes_ref.exact_image(shape, dtype, seed),), call,
                 lambda x, smoothing=smoothing: morphsnakes_ref.chan_vese(x, 7, "checkerboard", smoothing=smoothing), exact, knobs=sk(*on),
                 ref_key=("chan-vese", shape))
        for shape, dtype in (((12, 20, 70), "float64"), ((70, 96), "float32")):
            def gcall(gpu, x):
                from cupyimg_amd.skimage import segmentation
                return segmentation.morphological_geodesic_active_contour(x, 3, "disk", smoothing=1, threshold=0.5, balloon=-1)
            _add("skimage/gac-{}-{}".format("x".join(map(str, shape)), tag), lambda shape=shape, dtype=dtype: (morphsnakes_ref.volume(shape, dtype, 1),),
                 gcall, lambda x: morphsnakes_ref.geodesic_active_contour(x, 3, "disk", smoothing=1, threshold=0.5, balloon=-1), exact,
                 knobs=sk(*on), ref_key=("gac", shape))

    def auto_call(gpu, x):
        from cupyimg_amd.skimage import segmentation
        return segmentation.morphological_geodesic_active_contour(x, 2, "disk", smoothing=1, threshold="auto", balloon=1)
    _add("skimage/gac-auto-threshold", lambda: (morphsnakes_ref.volume((12, 20, 70), "float64", 1),), auto_call,
         lambda x: morphsnakes_ref.geodesic_active_contour(x, 2, "disk", smoothing=1, threshold="auto", balloon=1), exact)

    # optical flow: the fixed-point iterations at one level, bit for bit
    fk = _setting_knob("mi_debug_set_tvl1", (0, 0))
    for tag, on in (("planner", (0, 0)), ("small", (1, 0)), ("generic", (0, 1))):
        for shape, dtype in (((12, 20, 70), "float32"), ((70, 96), "float64")):
            def inputs(shape=shape, dtype=dtype):
                warped, ref, flow, proj = tvl1_ref.stage_inputs(shape, np.dtype(dtype).type)
                return warped, ref, flow, proj

            def call(gpu, warped, ref, flow, proj):
                from cupyimg_amd.skimage import registration
                grad, NI, rho_0 = registration._prepare(warped, ref, flow)
                f, p, _ = registration._iterate(rho_0, grad, NI, flow, proj, 7)
                return [grad, NI, rho_0, f, p]

            def want(warped, ref, flow, proj):
                grad, NI, rho_0 = tvl1_ref.prepare(warped, ref, flow)
                f, p = tvl1_ref.iterate(rho_0, grad, NI, flow, proj, 7)[:2]
                return [np.ascontiguousarray(grad), NI, rho_0, f, p]
            _add("skimage/tvl1-{}-{}".format("x".join(map(str, shape)), tag), inputs, call, want, exact, knobs=fk(*on), ref_key=("tvl1", shape))

    # the whole solver on one level, against the transcription run on this library's own building blocks (tests/test_gpu_tvl1.py)
    args = dict(attachment=15, tightness=0.3, num_warp=3, num_iter=2, tol=1e-4, prefilter=True)

    def level_inputs():
        ref, mov, _ = tvl1_ref.stop_case("runs_out", np.float32)
        return ref, mov, (0.3 * np.random.default_rng(5).standard_normal((ref.ndim,) + ref.shape)).astype(np.float32)

    def level_call(gpu, ref, mov, flow0):
        from cupyimg_amd.skimage import registration
        return registration._tvl1(ref, mov, flow0, **args)

    def level_want(ref, mov, flow0):
        import cupyimg_amd
        from test_gpu_tvl1 import _device_blocks
        return tvl1_ref.tvl1(ref, mov, flow0, blocks=_device_blocks(cupyimg_amd), **args)
    _add("skimage/tvl1-one-level", level_inputs, level_call, level_want, exact)

    # exposure
    ck =_setting_knob("mi_debug_set_clahe", (0, 0))
    for tag, on in (("fast", (0, 0)), ("generic", (1, 0)), ("shared-hist", (0, 1))):
        for shape, kernel, clip, nbins, dtype in (((9, 37, 64), (4, 9, 8), 0.02, 128, "float32"), ((17, 19), (4, 5), 0.01, 256, "uint16"),
                                                  ((34, 40, 70), (17, 16, 32), 0.01, 256, "uint16")):
            def call(gpu, x, kernel=kernel, clip=clip, nbins=nbins):
                from cupyimg_amd.skimage import exposure
                return exposure.equalize_adapthist(x, kernel_size=kernel, clip_limit=clip, nbins=nbins)
            _add("skimage/clahe-{}-{}".format("x".join(map(str, shape)), tag), lambda shape=shape, dtype=dtype: (exposure_ref.volume(shape, np.dtype(dtype), 1),),
                 call, lambda x, kernel=kernel, clip=clip, nbins=nbins: exposure_ref.equalize_adapthist(x, kernel, clip, nbins), exact, knobs=ck(*on),
                 ref_key=("clahe", shape))

    # edges: masked operators, hysteresis, canny
    ek = _setting_knob("mi_debug_set_edges", (0, 0))
    cases = edges_ref.canny_cases()
    for tag, on in (("planner", (0, 0)), ("small", (1, 0)), ("generic", (0, 1))):
        for fn, shape, dtype in (("sobel", (12, 20, 70), "float32"), ("scharr", (70, 96), "float64"), ("prewitt", (5, 1040), "uint8")):
            def inputs(shape=shape, dtype=dtype):
                from test_gpu_edges import _image, _mask
                return np.array(_image(shape, dtype)), np.array(_mask(shape))

            def call(gpu, x, m, fn=fn):
                from cupyimg_amd.skimage import filters
                return getattr(filters, fn)(x, m, mode="reflect")
            _add("skimage/{}-masked-{}-{}".format(fn, "x".join(map(str, shape)), tag), inputs, call,
                 lambda x, m, fn=fn: edges_ref.edge(fn, x, m, axis=None, mode="reflect", cval=0.0), same_bits, knobs=ek(*on),
                 ref_key=("edges", fn))
        for index in (0, len(cases) // 2, len(cases) - 1):
            cname, image, kw = cases[index]

            def cinputs(image=image, kw=kw):
                return (np.array(image),) + ((np.array(kw["mask"]),) if kw.get("mask") is not None else ())

            def ccall(gpu, x, m=None, kw=kw):
                from cupyimg_amd.skimage import feature
                return feature.canny(x, **dict(kw, mask=m))

            def cwant(x, m=None, kw=kw):
                return edges_ref.canny(x, **dict(kw, mask=m))
            _add("skimage/canny-{}-{}".format(cname, tag), cinputs, ccall, cwant, exact, knobs=ek(*on), ref_key=("canny", cname))

    def hyst_inputs(shape):
        image = _sndi().gaussian_filter(np.random.RandomState(21).uniform(size=shape), 1.0)
        return (image,)
    for shape in ((64, 70), (12, 20, 33)):
        def hcall2(gpu, x):
            from cupyimg_amd.skimage import filters
            lo, hi = (float(v) for v in np.quantile(x.get(), [0.45, 0.8]))
            return filters.apply_hysteresis_threshold(x, lo, hi)

        def hwant(x):
            lo, hi = (float(v) for v in np.quantile(x, [0.45, 0.8]))
            return edges_ref.apply_hysteresis_threshold(x, lo, hi)
        _add("skimage/hysteresis-" + "x".join(map(str, shape)), lambda shape=shape: hyst_inputs(shape), hcall2, hwant, exact)

    # structure tensor and the corner responses
    sk2 = _setting_knob("mi_debug_set_corners", (0, 0))
    for tag, on in (("planner", (0, 0)), ("small", (1, 0)), ("generic", (0, 1))):
        for shape, dtype in (((12, 20, 70), "float32"), ((5, 1040), "float64"), ((37, 131), "float32")):
            def inputs(shape=shape, dtype=dtype):
                from test_corners_yardstick import image_of
                return (np.array(image_of(shape, dtype)),)

            def call(gpu, x, shape=shape):
                from cupyimg_amd.skimage import feature
                xf = gpu.ascontiguousarray(feature._as_float_device(x))
                d = feature._sobel_block(xf, False, False, "reflect", 0.0)
                p = feature._sobel_block(xf, True, False, "reflect", 0.0)
                return [[d[e].get().reshape(shape) for e in range(d.shape[0])], [p[e].get().reshape(shape) for e in range(p.shape[0])]]

            def want(x):
                derivs = corner_ref.derivatives(corner_ref.prepare(x), "reflect", 0.0)
                return [list(derivs), list(corner_ref.products(derivs, "rc"))]
            _add("skimage/structure-products-{}-{}".format("x".join(map(str, shape)), tag), inputs, call, want, same_bits, knobs=sk2(*on), ref_key=("structure-products", shape))

        # an odd-width image through the padded row block: the tensor within the float filters' bound of a float64 SciPy
        # Gaussian of the transcription's products (tests/test_gpu_corners.py), the detectors bit for bit on the device's tensor
        def dinputs():
            from test_corners_yardstick import image_of
            return (np.array(image_of((37, 131), "float64")),)

        def tcall(gpu, x):
            from cupyimg_amd.skimage import feature
            return list(feature.structure_tensor(x, 1.5, mode="reflect", order="rc"))

        def twant(x):
            from test_gpu_corners import _gauss_bound
            out = []
            for p in corner_ref.structure_products(x, "reflect", 0, "rc"):
                ref, B, c = _gauss_bound(p.astype(np.float64), 1.5, "reflect", 0)
                out.append(np.stack([ref, B, np.full(ref.shape, float(c))]))
            return out

        def tcmp(got, want):
            from helpers import value_ranges as V
            ref, B, c = want
            ratio, at = V.ratio_of(got, ref, B, float(c.flat[0]), V.U64)
            assert ratio <= 1.0, (ratio, at)
        _add("skimage/structure-tensor-odd-width-" + tag, dinputs, tcall, twant, tcmp, knobs=sk2(*on), ref_key="structure-tensor-odd-width")

        def dcall(gpu, x):
            from cupyimg_amd.skimage import feature
            t = feature.structure_tensor(x, 1.5, order="rc")
            w, q = feature.corner_foerstner(x, sigma=1.5)
            return [list(t), feature.corner_harris(x, sigma=1.5), feature.corner_shi_tomasi(x, sigma=1.5), w, q,
                    feature.corner_kitchen_rosenfeld(x, mode="reflect")]

        def dwant(x, got):
            t = got[:3]
            w, q = corner_ref.corner_foerstner(*t)
            return [list(t), corner_ref.corner_harris(*t), corner_ref.corner_shi_tomasi(*t), w, q, corner_ref.corner_kitchen_rosenfeld(x, "reflect", 0)]
        _add("skimage/corner-detectors-odd-width-" + tag, dinputs, dcall, dwant, same_bits, knobs=sk2(*on), uses_got=True)

    # structural similarity and the simple metrics
    def ssim_inputs():
        rng = np.random.default_rng(150)
        x = (rng.random((20, 24, 28)) * 255).astype(np.uint8)
        return x, np.clip(x + rng.normal(0, 20, x.shape), 0, 255).astype(np.uint8)

    def ssim_call(gpu, x, y):
        from cupyimg_amd.skimage import metrics
        return [metrics.structural_similarity(x, y), metrics.structural_similarity(x, y, full=True)[1]]

    def ssim_want(x, y):
        from test_gpu_skimage import _ssim_host
        want, wmap = _ssim_host(x, y)
        return [want, wmap]
    # the bounds of tests/test_gpu_skimage.py: the mean within 1e-10, the map within rtol 1e-9 / atol 1e-11
    _add("skimage/ssim-combine-mean", ssim_inputs, ssim_call, ssim_want, [close(0, 1e-10), close(1e-9, 1e-11)])

    def grad_inputs():
        rng = np.random.RandomState(5)
        return rng.rand(30, 30) * 255, rng.rand(30, 30) * 255

    def grad_call(gpu, x, y):
        from cupyimg_amd.skimage import metrics
        got, ggrad, gmap = metrics.structural_similarity(x, y, data_range=255, gradient=True, full=True)
        return [got, ggrad, gmap]

    def grad_want(x, y):
        from test_gpu_skimage import _ssim_host
        want, wmap, wgrad = _ssim_host(x, y, data_range=255, gradient=True)
        return [want, wgrad, wmap]
    # test_ssim_gradient_and_multichannel: the mean below 1e-12, the gradient rtol 1e-8 / atol 1e-14, the map rtol 1e-9 / atol 1e-12
    _add("skimage/ssim-gradient", grad_inputs, grad_call, grad_want, [below(1e-12), close(1e-8, 1e-14), close(1e-9, 1e-12)])

    def rank4_inputs():
        rng = np.random.default_rng(151)
        x = rng.random((8, 9, 10, 11))
        return x, x + 0.1 * rng.standard_normal(x.shape)

    def rank4_call(gpu, x, y):
        from cupyimg_amd.skimage import metrics
        got, gmap = metrics.structural_similarity(x, y, data_range=1.0, full=True)
        return [got, gmap]

    def rank4_want(x, y):
        from test_gpu_skimage import _ssim_host
        return list(_ssim_host(x, y, data_range=1.0))
    _add("skimage/ssim-rank4", rank4_inputs, rank4_call, rank4_want, [close(0, 1e-10), close(1e-9, 1e-11)])

    def metric_call(gpu, a, b):
        from cupyimg_amd.skimage import metrics
        return [metrics.mean_squared_error(a, b), metrics.peak_signal_noise_ratio(a, b), metrics.normalized_root_mse(a, b),
                metrics.normalized_root_mse(a, b, normalization="min-max"), metrics.normalized_root_mse(a, b, normalization="mean")]

    def metric_want(a, b):
        af, bf = a.astype(np.float64), b.astype(np.float64)
        mse = np.mean((af - bf) ** 2)
        return [mse, 10 * np.log10(255 ** 2 / mse), np.sqrt(mse) / np.sqrt(np.mean(af * af)), np.sqrt(mse) / (af.max() - af.min()),
                np.sqrt(mse) / af.mean()]
    _add("skimage/simple-metrics", lambda: tuple(np.random.default_rng(152).integers(0, 256, size=(2, 37, 67)).astype(np.uint8)), metric_call,
         metric_want, [below(1e-10), below(1e-10), below(1e-12), below(1e-12), below(1e-12)])      # test_simple_metrics

    # transform
    for dtype, tol in (("float64", 1e-12), ("float32", 1e-6)):
        def rcall(gpu, x):
            from cupyimg_amd.skimage import transform
            return [transform.resize(x, (19, 26), anti_aliasing=True), transform.resize(x, (40, 61), anti_aliasing=False),
                    transform.pyramid_reduce(x), transform.pyramid_expand(x)]

        def rwant(x):
            x = x.astype(np.float64)
            return [tvl1_ref.resize(x, (19, 26), anti_aliasing=True), tvl1_ref.resize(x, (40, 61), anti_aliasing=False),
                    tvl1_ref.pyramid_reduce(x), tvl1_ref.pyramid_expand(x)]
        _add("skimage/resize-pyramid-" + dtype, lambda dtype=dtype: (tvl1_ref.smooth_noise((37, 52), 21, 1.0).astype(dtype),), rcall, rwant,
             maxnorm(tol))

    # warp: a 3 x 3 homography and the same map as a coordinate array, orders 1 and 3, through map_coordinates, min_max and the
    # clip that keeps cval (0, outside the image's range); SciPy and the bounds of tests/test_gpu_vs_oracle.py (1e-12 and 1e-10)
    H = np.array([[1.0, 0.1, 1.0], [-0.05, 0.95, 2.0], [0.0, 0.0, 1.0]])

    def warp_inputs():
        fimg = np.random.default_rng(30).random((30, 37))
        yy, xx = np.indices(fimg.shape, dtype=np.float64)
        src = np.stack([xx.ravel(), yy.ravel(), np.ones(xx.size)]).T @ H.T
        return fimg, np.stack([src[:, 1].reshape(fimg.shape), src[:, 0].reshape(fimg.shape)])

    def warp_call(gpu, x, coords):
        from cupyimg_amd.skimage import transform
        return [transform.warp(x, H, order=1), transform.warp(x, H, order=3), transform.warp(x, coords, order=1), transform.warp(x, coords, order=3)]

    def warp_want(x, coords):
        out = []
        for order in (1, 3):
            ref = _sndi().map_coordinates(x, coords, order=order, mode="constant", cval=0.0)
            exp = np.clip(ref, x.min(), x.max())
            exp[ref == 0.0] = 0.0
            out.append(exp)
        return out * 2
    _add("skimage/warp-homography-and-coordinates", warp_inputs, warp_call, warp_want, [close(0, 1e-12), close(0, 1e-10)] * 2)

    # the grey and binary morphology facade
    def facade_call(gpu, x):
        from cupyimg_amd.skimage import morphology as skm
        return [skm.erosion(x), skm.dilation(x), skm.opening(x), skm.closing(x), skm.white_tophat(x), skm.black_tophat(x)]

    def facade_want(x):
        nd = _sndi()
        s = nd.generate_binary_structure(2, 1)
        o = nd.grey_dilation(nd.grey_erosion(x, footprint=s), footprint=s)
        c = nd.grey_erosion(nd.grey_dilation(x, footprint=s), footprint=s)
        return [nd.grey_erosion(x, footprint=s), nd.grey_dilation(x, footprint=s), o, c, (x - o).astype(x.dtype), (c - x).astype(x.dtype)]
    _add("skimage/morphology-grey", _ints((37, 67), 153, np.uint8), facade_call, facade_want, exact)

    def bfacade_call(gpu, x):
        from cupyimg_amd.skimage import morphology as skm
        s = np.ones((3, 3), np.uint8)
        return [skm.binary_opening(x, s), skm.binary_closing(x, s)]

    def bfacade_want(x):
        nd = _sndi()
        s = np.ones((3, 3), np.uint8)
        return [nd.binary_dilation(nd.binary_erosion(x, structure=s, border_value=True), structure=s),
                nd.binary_erosion(nd.binary_dilation(x, structure=s), structure=s, border_value=True)]
    _add("skimage/morphology-binary", _bools((40, 33), 154, 0.55), bfacade_call, bfacade_want, exact)

    def eh_call(gpu, x):
        from cupyimg_amd.skimage import exposure
        hist, centers = exposure.histogram(x, nbins=64)
        return [exposure.equalize_hist(x, nbins=64), hist, centers]

    def eh_want(x):
        hist, centers = exposure_ref.histogram(x, 64)
        return [exposure_ref.equalize_hist(x, 64), hist, centers]
    _add("skimage/equalize-hist-histogram", lambda: (exposure_ref.volume((9, 37, 64), np.dtype("float32"), 1),), eh_call, eh_want, exact)


_skimage_cases()


# ---- the array layer (NumPy, exact)
def _array_cases():
    def S():
        from cupyimg_amd.scipy.ndimage import _support
        return _support

    _add("array/astype-float32-to-int16", lambda: ((np.random.default_rng(170).integers(-32768 * 4, 32767 * 4, size=(9, 67)) * 0.25).astype(np.float32),),
         lambda gpu, x: x.astype(np.int16), lambda x: x.astype(np.int16), exact)
    _add("array/astype-uint8-to-float64", _ints((5, 7, 33), 171, np.uint8), lambda gpu, x: x.astype(np.float64), lambda x: x.astype(np.float64), exact)
    _add("array/astype-strided-view", _ints((12, 14, 35), 172, np.int32), lambda gpu, x: x[1:11:2, ::3, 33:2:-2].astype(np.float32),
         lambda x: x[1:11:2, ::3, 33:2:-2].astype(np.float32), exact)
    _add("array/copy-strided-view", _f64((12, 14, 35), 173), lambda gpu, x: [x[::2, 1:, 3:30:3].copy(), gpu.ascontiguousarray(x.transpose(2, 0, 1))],
         lambda x: [x[::2, 1:, 3:30:3].copy(), np.ascontiguousarray(x.transpose(2, 0, 1))], exact)
    for mode in ("constant", "reflect", "edge", "symmetric", "wrap"):
        def pcall(gpu, x, mode=mode):
            from cupyimg_amd import _pad
            return _pad.pad(x, ((2, 3), (0, 4), (5, 1)), mode=mode)
        _add("array/pad-" + mode, _f32((7, 9, 33), 174), pcall, lambda x, mode=mode: np.pad(x, ((2, 3), (0, 4), (5, 1)), mode=mode), exact)

    def bpad(gpu, x):
        from cupyimg_amd import _pad
        return _pad.pad(x, 3, mode="constant", constant_values=1)
    _add("array/pad-bool", _bools((9, 37), 175), bpad, lambda x: np.pad(x, 3, mode="constant", constant_values=1), exact)
    for op, fn in (("add", np.add), ("subtract", np.subtract), ("multiply", np.multiply)):
        _add("array/elementwise-" + op, lambda: tuple(np.random.default_rng(176).standard_normal((2, 9, 67))),
             lambda gpu, a, b, op=op: S().elementwise(op, a, b, gpu.empty(a.shape, np.float64)), lambda a, b, fn=fn: fn(a, b), exact)
    _add("array/elementwise-int16-wrap", lambda: tuple(np.random.default_rng(177).integers(-30000, 30000, size=(2, 5, 131)).astype(np.int16)),
         lambda gpu, a, b: S().elementwise("add", a, b, gpu.empty(a.shape, np.int16)), lambda a, b: a + b, exact)
    _add("array/elementwise-sqrt", lambda: (np.random.default_rng(178).random((9, 67)),),
         lambda gpu, a: S().elementwise("sqrt", a, None, gpu.empty(a.shape, np.float64)), lambda a: np.sqrt(a), exact)
    _add("array/clip", _f32((9, 67), 179), lambda gpu, a: [S().clip(a, -0.5, 0.75), S().clip(a, -0.5, 0.75, keep=float(np.float32(a.get().ravel()[5])))],
         lambda a: [np.clip(a, np.float32(-0.5), np.float32(0.75)), np.where(a == a.ravel()[5], a, np.clip(a, np.float32(-0.5), np.float32(0.75)))], exact)
    for dtype in ("float32", "int16", "uint8", "float64"):
        def inputs(dtype=dtype):
            rng = np.random.default_rng(180)
            return ((rng.standard_normal((300, 1031)) * 100).astype(dtype),)
        _add("array/min-max-" + dtype, inputs, lambda gpu, a: list(S().min_max(a)), lambda a: [float(a.min()), float(a.max())], exact_values)

    def sum_call(gpu, a, b):
        from cupyimg_amd.skimage.metrics import _sum
        return [_sum(0, a), _sum(1, a, b), _sum(2, a)]
    # integers below 2**53 in total: every order of summation gives the same float64
    _add("array/sum", lambda: tuple(np.random.default_rng(181).integers(-1000, 1000, size=(2, 37, 4099)).astype(np.float64)), sum_call,
         lambda a, b: [a.sum(), ((a - b) ** 2).sum(), (a * a).sum()], exact_values)


_array_cases()

# ---- the kernel each case ends on, as last_kernel() names it (the kernels that do not name themselves are absent): a knob or a
# shape that stops selecting the route a case is named for fails the case
_ENDS_ON = {
    "sep/lean5-uniform": "mi::sep3d_lean_kernel<5,10,4,2,2,false>",
    "sep/lean3-gaussian-constant": "mi::sep3d_lean_kernel<5,10,4,2,2,true>",
    "sep/long17-gaussian": "mi::sep3d_long3_kernel<17,true>",
    "sep/long9-ragged": "mi::sep3d_long3_kernel<9,true,ragged>",
    "sep/long11-uniform": "mi::sep3d_long3_kernel<11,true>",
    "sep/image2d": "mi::stream_pass_kernel<9,9,4,0>",
    "sep/lean5-ragged": "mi::sep3d_lean_kernel<5,10,4,2,2,false,ragged>",
    "sep/lean7-ragged-constant": "mi::sep3d_lean_kernel<7,8,4,3,2,true,ragged>",
    "sep/float64-uniform-image": "mi::stream_pass_f64_kernel<1,3,2,0>",
    "correlate/stencil3s": "mi::stencil3s_kernel<3,double,2,ragged>",
    "correlate/stencil3": "mi::stencil3_kernel<3,16,double,dense,correlate>",
    "signal/convolve-full-float64": "mi::affine3d_fast",
    "minmax/uint8-fused-7": "mi::mm3u8_split_kernel<7,min,13,3,3,32,false>",
    "minmax/uint8-ragged-5": "mi::mm3u8_ragged_kernel<5,min>",
    "minmax/uint8-extended-rows-5": "mi::mm3u8_split_kernel<5,min,12,4,3,32,false>",
    "minmax/uint8-ragged-block-end-3": "mi::mm3u8_split_kernel<3,max,12,4,3,32,false>",
    "minmax/uint16-ragged-3": "mi::mm3s16_ragged_kernel<3,min,uint16>",
    "minmax/float32-fused-3": "mi::mm3f32_long_kernel<3,max>",
    "minmax/float32-two-launches": "mi::stream_pass_kernel<1,3,2,2>",
    "rank/median3x3-ragged": "mi::rank3_sorted_kernel<float,16,>",
    "rank/median3x3-float32-ragged": "mi::rank3_sorted_kernel<float,16,>",
    "rank/median3x3-uint16-ragged": "mi::rank3_sorted_kernel<float,16,>",
    "rank/median27-shared-sort": "mi::median27_stream_kernel<13>",
    "rank/median27-uint8": "mi::median27_stream_kernel<13>",
    "rank/median27-per-voxel": "mi::rank3_sorted_kernel<32,27,13>",
    "rank/rank27": "mi::rank3_sorted_kernel<float,32,>",
    "rank/network16": "mi::rank3_sorted_kernel<float,16,>",
    "rank/network32": "mi::rank3_sorted_kernel<32,25,12>",
    "rank/network32-full": "mi::rank3_sorted_kernel<float,32,>",
    "rank/network64": "mi::rank3_sorted_kernel<float,64,>",
    "rank/network128": "mi::rank3_sorted_kernel<float,128,>",
    "rank/beyond128": "mi::rank_nd_kernel",
    "rank/selection": "mi::rank3_kernel",
    "rank/rank4": "mi::rank_nd_kernel",
    "rank/percentile": "mi::rank3_sorted_kernel<float,16,>",
    "binary/byte-generic": "mi::binary3_kernel<bool>",
    "binary/byte-ragged": "mi::binary3_kernel<bool>",
    "binary/byte-image": "mi::binary3_kernel<bool>",
    "binary/int16-input": "mi::binary3_kernel<bool>",
    "binary/bits-fused-3": "mi::bitmorph3_kernel<nomask,1,256,cross>",
    "binary/bits-small": "mi::bitmorph3_kernel<nomask,1,256,cross>",
    "binary/bits-ragged": "mi::bitmorph3_kernel<nomask,1,256,cross,ragged>",
    "binary/bits-ragged-off": "mi::binary3_kernel<bool>",
    "binary/bits-image": "mi::bitmorph3_kernel<nomask,1,256,table>",
    "binary/bits-table": "mi::bitmorph3_kernel<nomask,1,256,table>",
    "binary/closing-image": "mi::binary3_kernel<bool>",
    "binary/hit-or-miss": "mi::binary3_kernel<bool>",
    "binary/erosion-until-stable": "mi::bitmorph3_kernel<nomask,1,256,cross>",
    "binary/propagation-bitfill": "mi::bitfill3_kernel<aligned>",
    "binary/fill-holes-bitfill": "mi::bitfill3_kernel<aligned>",
    "binary/propagation-no-bitfill": "mi::bitmorph3_kernel<mask,1,256,cross>",
    "binary/fill-holes-no-bitfill": "mi::bitmorph3_kernel<mask,1,256,cross>",
    "binary/propagation-image": "mi::binary3_kernel<bool>",
    "binary/fill-holes-image": "mi::binary3_kernel<bool>",
    "binary/dilation-masked-until-stable-rank4": "mi::binary_erosion_kernel<bool,8>",
    "interp/order1-small-general-constant": "mi::affine3d_c1_kernel",
    "interp/order1-small-zdecoupled-matrix-constant": "mi::affine3d_c1_kernel",
    "interp/order1-small-xfixed-matrix-constant": "mi::affine3d_c1_kernel",
    "interp/order1-small-general-nearest": "mi::affine3d_fast",
    "interp/order1-small-zdecoupled-matrix-nearest": "mi::affine3d_fast",
    "interp/order1-small-xfixed-matrix-nearest": "mi::affine3d_fast",
    "interp/order1-lds-box-big": "mi::affine3d_lds_kernel<64,8>",
    "interp/order1-zstream-big": "mi::affine3d_zrect_kernel<32,0>",
    "interp/order1-rowblend-big": "mi::affine3d_rowblend_kernel",
    "interp/order1-round2-kernels": "mi::affine3d_fast",
    "interp/order1-gather": "mi::affine3d_c1_kernel",
    "interp/order0-output-shape": "mi::affine3d_fast",
    "interp/order1-image": "mi::affine3d_fast",
    "interp/map-coordinates-order1-zstream-big": "mi::map_coords3d_zstream_kernel<true,8,1>",
    "interp/cubic-small-general": "mi::cubic3_f32_kernel",
    "interp/cubic-small-zdecoupled-matrix": "mi::cubic3_f32_kernel",
    "interp/cubic-small-zdecoupled-matrix-zfactor-off": "mi::cubic3_f32_kernel",
    "interp/cubic-small-xfixed-matrix": "mi::cubic3_f32_kernel",
    "interp/cubic-gather": "mi::cubic3_f32_kernel",
    "interp/cubic-strip": "mi::cubic3_diag_f32_kernel",
    "interp/cubic-box-big": "mi::cubic3_box_kernel",
    "interp/cubic-zfactor-big": "mi::cubic3_zfactor_kernel<0>",
    "interp/cubic-zstream-big": "mi::cubic3_zstream_kernel<0>",
    "interp/cubic-rowblend-big": "mi::cubic3_rowblend_kernel",
    "interp/zoom-order1-image": "mi::affine3d_fast",
    "interp/rotate-volume": "mi::cubic3_f32_kernel",
    "interp/rotate-image-reshape": "mi::affine3d_fast",
    "label/volume-tiles": "mi::label_tile_kernel",
    "label/volume-26-tiles": "mi::label_tile_kernel",
    "label/image-tiles": "mi::label_tile_kernel",
    "label/volume-generic": "mi::label_connect_kernel<binary>",
    "label/volume-26-generic": "mi::label_connect_kernel<binary>",
    "label/image-generic": "mi::label_connect_kernel<binary>",
    "label/rank4": "mi::label_connect_kernel<binary>",
    "label/int16-input": "mi::label_tile_kernel",
    "skimage/reconstruction-20x37x64-dilation-planner": "mi::greyrec3_kernel<uint8,dilation>",
    "skimage/reconstruction-5x1040-erosion-planner": "mi::greyrec3_kernel<float32,erosion>",
    "skimage/reconstruction-9x50x130-dilation-planner": "mi::greyrec3_kernel<int16,dilation>",
    "skimage/reconstruction-20x37x64-dilation-small": "mi::greyrec3_kernel<uint8,dilation>",
    "skimage/reconstruction-5x1040-erosion-small": "mi::greyrec3_kernel<float32,erosion>",
    "skimage/reconstruction-9x50x130-dilation-small": "mi::greyrec3_kernel<int16,dilation>",
    "skimage/reconstruction-20x37x64-dilation-generic": "mi::greyrec_generic_kernel<dilation>",
    "skimage/reconstruction-5x1040-erosion-generic": "mi::greyrec_generic_kernel<erosion>",
    "skimage/reconstruction-9x50x130-dilation-generic": "mi::greyrec_generic_kernel<dilation>",
    "skimage/tv-chambolle-12x20x70-float32-planner": "mi::tv_fused_kernel<float32,volume>",
    "skimage/tv-chambolle-70x96-float64-planner": "mi::tv_fused_kernel<float64,image>",
    "skimage/tv-chambolle-2x5x1040-float32-planner": "mi::tv_fused_kernel<float32,volume>",
    "skimage/tv-chambolle-12x20x70-float32-small": "mi::tv_fused_kernel<float32,volume>",
    "skimage/tv-chambolle-70x96-float64-small": "mi::tv_fused_kernel<float64,image>",
    "skimage/tv-chambolle-2x5x1040-float32-small": "mi::tv_fused_kernel<float32,volume>",
    "skimage/tv-chambolle-12x20x70-float32-generic": "mi::tv_generic_kernel<float32>",
    "skimage/tv-chambolle-70x96-float64-generic": "mi::tv_generic_kernel<float64>",
    "skimage/tv-chambolle-2x5x1040-float32-generic": "mi::tv_generic_kernel<float32>",
    "skimage/meijering-9x67-planner": "mi::ridge_tile_kernel<float64,2,fused>",
    "skimage/sato-7x9x67-planner": "mi::ridge_tile_kernel<float64,3,fused>",
    "skimage/frangi-19x23x70-planner": "mi::ridge_tile_kernel<float64,3,fused>",
    "skimage/hessian-matrix-19x23x70-planner": "mi::ridge_tile_kernel<float32,3,hessian-rc>",
    "skimage/hessian-matrix-9x67-planner": "mi::ridge_tile_kernel<float32,2,hessian-rc>",
    "skimage/meijering-9x67-small": "mi::ridge_tile_kernel<float64,2,fused>",
    "skimage/sato-7x9x67-small": "mi::ridge_tile_kernel<float64,3,fused>",
    "skimage/frangi-19x23x70-small": "mi::ridge_tile_kernel<float64,3,fused>",
    "skimage/hessian-matrix-19x23x70-small": "mi::ridge_tile_kernel<float32,3,hessian-rc>",
    "skimage/hessian-matrix-9x67-small": "mi::ridge_tile_kernel<float32,2,hessian-rc>",
    "skimage/meijering-9x67-generic": "mi::eig_generic_kernel<float64,2>",
    "skimage/sato-7x9x67-generic": "mi::eig_generic_kernel<float64,3>",
    "skimage/frangi-19x23x70-generic": "mi::eig_generic_kernel<float64,3>",
    "skimage/hessian-matrix-19x23x70-generic": "mi::hessian_generic_kernel<float32>",
    "skimage/hessian-matrix-9x67-generic": "mi::hessian_generic_kernel<float32>",
    "skimage/chan-vese-20x37x70-planner": "mi::snake_fused_kernel<acwe,float32,3,smoothing=1>",
    "skimage/chan-vese-70x96-planner": "mi::snake_fused_kernel<acwe,float32,2,smoothing=2>",
    "skimage/gac-12x20x70-planner": "mi::snake_fused_kernel<gac,float64,3,smoothing=1>",
    "skimage/gac-70x96-planner": "mi::snake_fused_kernel<gac,float32,2,smoothing=1>",
    "skimage/chan-vese-20x37x70-small": "mi::snake_fused_kernel<acwe,float32,3,smoothing=1>",
    "skimage/chan-vese-70x96-small": "mi::snake_fused_kernel<acwe,float32,2,smoothing=2>",
    "skimage/gac-12x20x70-small": "mi::snake_fused_kernel<gac,float64,3,smoothing=1>",
    "skimage/gac-70x96-small": "mi::snake_fused_kernel<gac,float32,2,smoothing=1>",
    "skimage/chan-vese-20x37x70-generic": "mi::snake_generic_kernel<acwe,float32,3>",
    "skimage/chan-vese-70x96-generic": "mi::snake_generic_kernel<acwe,float32,2>",
    "skimage/gac-12x20x70-generic": "mi::snake_generic_kernel<gac,float64,3>",
    "skimage/gac-70x96-generic": "mi::snake_generic_kernel<gac,float32,2>",
    "skimage/gac-auto-threshold": "mi::snake_fused_kernel<gac,float64,3,smoothing=1>",
    "skimage/tvl1-12x20x70-planner": "mi::tvl1_reg_fused_kernel<float32,volume>",
    "skimage/tvl1-70x96-planner": "mi::tvl1_reg_fused_kernel<float64,image>",
    "skimage/tvl1-12x20x70-small": "mi::tvl1_reg_fused_kernel<float32,volume>",
    "skimage/tvl1-70x96-small": "mi::tvl1_reg_fused_kernel<float64,image>",
    "skimage/tvl1-12x20x70-generic": "mi::tvl1_step_kernels<float32>",
    "skimage/tvl1-70x96-generic": "mi::tvl1_step_kernels<float64>",
    "skimage/tvl1-one-level": "mi::tvl1_reg_fused_kernel<float32,volume>",
    "skimage/clahe-9x37x64-fast": "mi::clahe_apply_kernel<float32,3>",
    "skimage/clahe-17x19-fast": "mi::clahe_apply_kernel<uint16,2>",
    "skimage/clahe-34x40x70-fast": "mi::clahe_apply_kernel<uint16,3>",
    "skimage/clahe-9x37x64-generic": "mi::clahe_generic_kernel<float32,3>",
    "skimage/clahe-17x19-generic": "mi::clahe_generic_kernel<uint16,2>",
    "skimage/clahe-34x40x70-generic": "mi::clahe_generic_kernel<uint16,3>",
    "skimage/clahe-9x37x64-shared-hist": "mi::clahe_apply_kernel<float32,3>",
    "skimage/clahe-17x19-shared-hist": "mi::clahe_apply_kernel<uint16,2>",
    "skimage/clahe-34x40x70-shared-hist": "mi::clahe_apply_kernel<uint16,3>",
    "skimage/sobel-masked-12x20x70-planner": "mi::edge_fused_kernel<float32,3>",
    "skimage/scharr-masked-70x96-planner": "mi::edge_fused_kernel<float64,2>",
    "skimage/prewitt-masked-5x1040-planner": "mi::edge_fused_kernel<float64,2>",
    "skimage/canny-ring-float64-planner": "mi::canny_nms_kernel",
    "skimage/canny-noise_37x131-float32-planner": "mi::binary3_kernel<bool>",
    "skimage/canny-noise_37x131-quantiles-uint8-planner": "mi::binary3_kernel<bool>",
    "skimage/sobel-masked-12x20x70-small": "mi::edge_fused_kernel<float32,3>",
    "skimage/scharr-masked-70x96-small": "mi::edge_fused_kernel<float64,2>",
    "skimage/prewitt-masked-5x1040-small": "mi::edge_fused_kernel<float64,2>",
    "skimage/canny-ring-float64-small": "mi::canny_nms_kernel",
    "skimage/canny-noise_37x131-float32-small": "mi::binary3_kernel<bool>",
    "skimage/canny-noise_37x131-quantiles-uint8-small": "mi::binary3_kernel<bool>",
    "skimage/sobel-masked-12x20x70-generic": "mi::edge_generic<float32>",
    "skimage/scharr-masked-70x96-generic": "mi::edge_generic<float64>",
    "skimage/prewitt-masked-5x1040-generic": "mi::edge_generic<float64>",
    "skimage/canny-ring-float64-generic": "mi::canny_generic_kernel",
    "skimage/canny-noise_37x131-float32-generic": "mi::binary3_kernel<bool>",
    "skimage/canny-noise_37x131-quantiles-uint8-generic": "mi::binary3_kernel<bool>",
    "skimage/hysteresis-64x70": "mi::binary3_kernel<bool>",
    "skimage/hysteresis-12x20x33": "mi::binary3_kernel<bool>",
    "skimage/structure-products-12x20x70-planner": "mi::st_fused_kernel<float32,3,products>",
    "skimage/structure-products-5x1040-planner": "mi::st_fused_kernel<float64,2,products>",
    "skimage/structure-products-37x131-planner": "mi::st_fused_kernel<float32,2,products>",
    "skimage/structure-tensor-odd-width-planner": "mi::st_fused_kernel<float64,2,products>",
    "skimage/corner-detectors-odd-width-planner": "mi::corner_response_kernel<float64,kitchen_rosenfeld>",
    "skimage/structure-products-12x20x70-small": "mi::st_fused_kernel<float32,3,products>",
    "skimage/structure-products-5x1040-small": "mi::st_fused_kernel<float64,2,products>",
    "skimage/structure-products-37x131-small": "mi::st_fused_kernel<float32,2,products>",
    "skimage/structure-tensor-odd-width-small": "mi::st_fused_kernel<float64,2,products>",
    "skimage/corner-detectors-odd-width-small": "mi::corner_response_kernel<float64,kitchen_rosenfeld>",
    "skimage/structure-products-12x20x70-generic": "mi::st_generic<float32>",
    "skimage/structure-products-5x1040-generic": "mi::st_generic<float64>",
    "skimage/structure-products-37x131-generic": "mi::st_generic<float32>",
    "skimage/structure-tensor-odd-width-generic": "mi::st_generic<float64>",
    "skimage/corner-detectors-odd-width-generic": "mi::corner_response_kernel<float64,kitchen_rosenfeld>",
    "skimage/ssim-combine-mean": "mi::stream_pass_f64_kernel<1,7,2,0>",
    "skimage/ssim-gradient": "mi::stream_pass_f64_kernel<7,7,2,0>",
    "skimage/resize-pyramid-float64": "mi::stream_pass_f64_kernel<7,7,2,0>",
    "skimage/resize-pyramid-float32": "mi::stream_pass_kernel<7,7,2,0>",
    "skimage/morphology-binary": "mi::binary3_kernel<bool>",
    "skimage/equalize-hist-histogram": "mi::interp_map_kernel<float32,LDS>",
    "array/pad-constant": "mi::affine3d_fast",
    "array/pad-reflect": "mi::affine3d_fast",
    "array/pad-edge": "mi::affine3d_fast",
    "array/pad-symmetric": "mi::affine3d_fast",
    "array/pad-wrap": "mi::affine3d_fast",
}
for _case in CASES:
    if _case.name in _ENDS_ON:
        _case.route = tuple(p for p in ((_case.route,) if isinstance(_case.route, str) else _case.route or ()) if p) + (_ENDS_ON[_case.name],)
assert not set(_ENDS_ON) - {c.name for c in CASES}
