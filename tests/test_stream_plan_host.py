"""The chunk planner of the streaming launches (csrc/stream3d.hpp plan_stream_chunks), through its debug export.  No device
is needed: the planner is host arithmetic and the library loads without a GPU."""
import ctypes
import itertools

NLINES = (1, 2, 7, 8, 63, 64, 181, 217, 512, 4095, 4096, 4097, 100000)
N_AXIS = tuple(range(1, 301)) + (511, 512, 513, 1024, 2047, 2048, 2049, 4096)
RAMPS = (0, 2, 4, 8, 12, 32)
LIMITS = ((16, 1024), (8, 2048), (8, 1024))      # (shortest chunk, most chunks tried): the three pairs the launches pass


def yardstick(nlines, n_axis, ramp, min_chunk, max_chunks):
    """The loop every streaming launch carried a copy of before the planner was shared, transcribed line by line.  The
    arithmetic is integer and IEEE double, as in C++, so the comparison is exact."""
    nch = 1
    best = 1e300
    c = 1
    while c <= n_axis and c <= max_chunks:
        chunk = (n_axis + c - 1) // c
        if c > 1 and chunk < min_chunk:
            break
        real = (n_axis + chunk - 1) // chunk
        rounds = max(1.0, float(nlines) * real / 4096.0)
        cost = rounds * ((chunk + ramp) + 4.0)
        if cost < best * 0.999:
            best = cost
            nch = real
        c += 1
    chunk = (n_axis + nch - 1) // nch
    return chunk, (n_axis + chunk - 1) // chunk


def test_planner_matches_the_loop_it_replaced():
    from cupyimg_amd import _lib
    plan = _lib.load().mi_debug_plan_stream_chunks
    plan.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)] * 2
    plan.restype = ctypes.c_int
    chunk, nchunks = ctypes.c_int(), ctypes.c_int()
    pc, pn = ctypes.byref(chunk), ctypes.byref(nchunks)
    wrong = []
    for (min_chunk, max_chunks), ramp, nlines, n_axis in itertools.product(LIMITS, RAMPS, NLINES, N_AXIS):
        assert plan(nlines, n_axis, ramp, min_chunk, max_chunks, pc, pn) == 0
        got = (chunk.value, nchunks.value)
        covers = got[0] * got[1] >= n_axis > got[0] * (got[1] - 1)
        if got != yardstick(nlines, n_axis, ramp, min_chunk, max_chunks) or not covers:
            wrong.append(((nlines, n_axis, ramp, min_chunk, max_chunks), got))
    assert not wrong, wrong[:10]


def test_planner_refuses_empty_problems():
    from cupyimg_amd import _lib
    plan = _lib.load().mi_debug_plan_stream_chunks
    plan.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)] * 2
    plan.restype = ctypes.c_int
    chunk, nchunks = ctypes.c_int(), ctypes.c_int()
    for args in ((0, 8, 2, 8, 1024), (8, 0, 2, 8, 1024), (8, 8, -1, 8, 1024), (8, 8, 2, 0, 1024), (8, 8, 2, 8, 0)):
        assert plan(*args, ctypes.byref(chunk), ctypes.byref(nchunks)) == _lib.MI_ERR_INVALID_ARG
    assert plan(8, 8, 2, 8, 1024, None, ctypes.byref(nchunks)) == _lib.MI_ERR_INVALID_ARG
