"""Grey morphology on the device against the plain NumPy reference of tests/helpers/grey_ref.py (which
tests/test_grey_yardstick.py holds against SciPy bit for bit): the seeded draw on both geometries of mi_minmax_nd, and
directed cases for what the draw's small shapes cannot reach (a leading axis beyond 65535, windows of more than 2048 cells,
tap tables of more than 128 entries).  Every comparison is exact: dtype, shape and every element; the route of each case is
read from last_kernel().

The three generic kernels of csrc/minmax.hip note themselves as `minmax3_kernel` (rank <= 3 geometry), `minmax_nd_kernel<3>`
(rank <= 3 arrays outside that geometry, or with mi_debug_set_minmax_fast3(0)) and `minmax_nd_kernel<8>` (rank >= 4)."""
import ctypes

import numpy as np
import pytest

from helpers import grey_ref as gr

pytestmark = pytest.mark.gpu

FAST3, GENERIC3, GENERIC8 = "minmax3_kernel", "minmax_nd_kernel<3>", "minmax_nd_kernel<8>"
_WANT = {}


def _want(i, case):
    """the reference's result of drawn case `i`, computed once"""
    if i not in _WANT:
        _WANT[i] = gr.reference(case)
        if isinstance(_WANT[i], np.ndarray):
            _WANT[i].setflags(write=False)
    return _WANT[i]


def _fast3(on):
    from cupyimg_amd import _lib
    assert _lib.load().mi_debug_set_minmax_fast3(ctypes.c_int(on)) == 0


def _run(gpu, case):
    """(outcome of the call, the note of the last kernel the call launched that notes itself, "" for none)"""
    from cupyimg_amd.scipy import ndimage as ndi
    # last_kernel() keeps the last note: a tiny launch of a kernel no grey call ends on marks "none"
    ndi.binary_erosion(gpu.asarray(np.ones((2, 2, 2, 2), np.int16)))
    got = gr.call(ndi, case, to_array=gpu.asarray)
    note = gpu.last_kernel()
    return got, "" if "binary_erosion_kernel<int16" in note else note


def _check(gpu, case, want, route):
    """the failures (texts) of one run of `case` that has to end on the kernel named `route`"""
    got, note = _run(gpu, case)
    ok, why = gr.judge(case, want, got)
    bad = [] if ok else [(case["desc"], note, why)]
    generic = "minmax3_kernel" in note or "minmax_nd_kernel" in note
    must = gr.has_structure(case) and not isinstance(want, ValueError)       # no other route takes a structure
    if (generic or must) and route not in note:
        bad.append((case["desc"], "ended on '%s', not on %s" % (note, route)))
    if must and "structure=1" not in note:
        bad.append((case["desc"], "the note does not name the structure: '%s'" % note))
    return bad


@pytest.mark.parametrize("family", gr.FAMILIES)
def test_drawn_cases_equal_the_reference_on_both_geometries(gpu, family):
    bad, runs, generic_runs = [], 0, 0
    try:
        for i, case in enumerate(gr.drawn()):
            if gr.family(case) != family:
                continue
            want = _want(i, case)
            if len(case["shape"]) > 3:
                bad += _check(gpu, case, want, GENERIC8)
                runs += 1
                continue
            for on, route in ((1, FAST3), (0, GENERIC3)):
                _fast3(on)
                bad += _check(gpu, case, want, route)
                runs += 1
            generic_runs += gr.has_structure(case) and not case["illegal"]
    finally:
        _fast3(1)
    print("family %s: %d runs, %d rank <= 3 cases with a structure on both geometries, %d failures" % (family, runs, generic_runs, len(bad)))
    assert runs >= 100 and generic_runs >= 8, (runs, generic_runs)
    assert not bad, (len(bad), bad[:6])


# ---------------------------------------------------------------------------------------------------------------------
# directed cases
# ---------------------------------------------------------------------------------------------------------------------
def _directed(gpu, case, route):
    want = gr.reference(case)
    assert isinstance(want, np.ndarray), want
    bad = _check(gpu, case, want, route)
    assert not bad, bad
    return want


@pytest.mark.parametrize("func", ["grey_erosion", "grey_dilation"])
def test_leading_axis_beyond_65535_takes_the_generic_rank3_kernel(gpu, func):
    rng = np.random.default_rng(101)
    x = rng.integers(0, 256, size=(65540, 2, 3)).astype(np.uint8)
    fp = np.ones((3, 2, 2), bool)
    fp[2, 1, 1] = False
    st = rng.integers(-24, 24, size=fp.shape) / 8.0 + 0.1
    _directed(gpu, gr.make_case(func, x, footprint=fp, structure=st), GENERIC3)


@pytest.mark.parametrize("func", ["grey_erosion", "grey_dilation"])
def test_window_of_more_than_2048_cells_takes_the_generic_rank3_kernel(gpu, func):
    rng = np.random.default_rng(102)
    x = rng.normal(0.0, 40.0, size=(50, 50)).astype(np.float32)
    fp = rng.random((46, 46)) > 0.3
    fp[23, 23] = False
    assert fp.size == 2116 and not fp.all()
    st = rng.integers(-24, 24, size=fp.shape) / 8.0 + 0.1
    _directed(gpu, gr.make_case(func, x, footprint=fp, structure=st, mode="mirror"), GENERIC3)


@pytest.mark.parametrize("func", ["grey_erosion", "grey_dilation"])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("ext,shape,origin", [((12, 12), (17, 70), (-3, 5)), ((5, 6, 5), (6, 7, 66), (1, -3, -2))])
def test_more_than_128_taps_with_values_use_the_device_tap_table(gpu, func, dtype, ext, shape, origin):
    rng = np.random.default_rng(103)
    x = rng.normal(0.0, 40.0, size=shape).astype(dtype)
    st = rng.integers(-24, 24, size=ext) / 8.0 + 0.1
    assert st.size in (144, 150)
    case = gr.make_case(func, x, structure=st, mode="constant", cval=1.5, origin=list(origin))
    _directed(gpu, case, FAST3)
    assert "ntaps=%d" % st.size in gpu.last_kernel() and "device-buffer" in gpu.last_kernel(), gpu.last_kernel()


@pytest.mark.parametrize("func", ["grey_erosion", "grey_dilation"])
@pytest.mark.parametrize("shape,ext,origin", [((3, 4, 5, 70), (2, 1, 3, 4), (-1, 0, 1, -2)), ((2, 3, 2, 4, 9), (1, 2, 2, 3, 2), (0, -1, 0, 1, -1))])
def test_rank_4_and_5_with_a_structure_and_an_origin(gpu, func, shape, ext, origin):
    rng = np.random.default_rng(104)
    for dtype in ("uint16", "float64"):
        x = rng.integers(0, 1000, size=shape).astype(dtype)
        st = rng.integers(-24, 24, size=ext) / 8.0 + 0.1
        _directed(gpu, gr.make_case(func, x, structure=st, mode="nearest", origin=list(origin)), GENERIC8)


def test_uint8_erosion_by_fives_wraps_like_the_reference(gpu):
    """tap 0 goes negative in double, the later taps wrap in uint8, the store wraps"""
    x = (np.arange(9 * 70).reshape(9, 70) % 5).astype(np.uint8)
    case = gr.make_case("grey_erosion", x, structure=np.full((3, 3), 5.0))
    want = _directed(gpu, case, FAST3)
    assert want.dtype == np.uint8 and want.min() >= 251          # every result has wrapped


@pytest.mark.parametrize("out_dtype", ["float32", "float64"])
def test_first_tap_in_double_later_taps_in_float32(gpu, out_dtype):
    """structure values no float32 holds: the result tells tap 0 in double from tap 0 in float32"""
    rng = np.random.default_rng(105)
    x = rng.random((9, 70)).astype(np.float32)
    st = np.array([[1.0 / 3.0, 0.1], [0.1, 1.0 / 3.0]])
    for func in ("grey_erosion", "grey_dilation"):
        case = gr.make_case(func, x, out_kind="dtype", out_dtype=out_dtype, structure=st)
        want = _directed(gpu, case, FAST3)
        other = gr.reference(case, first_tap_in_dtype=True)
        assert (want != other).sum() >= 20, (want != other).sum()      # the case discriminates


@pytest.mark.parametrize("func", ["morphological_laplace", "morphological_gradient"])
def test_composites_on_an_even_footprint_with_an_origin_return_the_output_array(gpu, func):
    from cupyimg_amd import _lib
    rng = np.random.default_rng(106)
    x = rng.integers(0, 256, size=(9, 70)).astype(np.uint8)
    fp = np.array([[1, 0, 1, 1], [1, 1, 0, 1]], bool)
    case = gr.make_case(func, x, out_kind="array", out_layout="c", footprint=fp, origin=[-1, 1])
    want = gr.reference(case)
    got, note = _run(gpu, case)
    assert got[0] is got[1]                                       # the result is the array given as output
    assert gr.judge(case, want, got) == (True, ""), gr.judge(case, want, got)
    assert "stencil3_kernel" in note or FAST3 in note, note
    tiled = _lib.load().mi_debug_set_minmax_tiled
    try:
        assert tiled(ctypes.c_int(0)) == 0
        bad = _check(gpu, case, want, FAST3)
        assert not bad, bad
        assert "structure=0" in gpu.last_kernel(), gpu.last_kernel()
    finally:
        tiled(ctypes.c_int(1))
