"""What the uint8 and 16-bit streaming entry points accept and refuse, called directly through ctypes.

A wrong refusal never shows as a wrong result (the Python layer catches Unsupported and takes another device route), so
the gates get a table of their own: for every case the return code and the text of mi_last_error(), and for accepted
cases the output, bit for bit against the oracle.  Every descriptor points into a real device allocation, so a gate
that wrongly accepts still runs on valid memory.  Shapes are the smallest that reach each rule (a few KiB)."""
import ctypes

import numpy as np
import pytest

from oracle import ndimage as orc

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUP = 0, -1, -2
ACCEPT = "accept"
NA = "n/a"              # the case has no meaning for this entry point (it has no size / origin / footprint)


def R(msg):
    """Refused as unsupported; the text is "<entry>: <msg>"."""
    return (UNSUP, msg)


def BAD(msg):
    """Invalid argument; the text has no prefix (_lib.check maps these two to ValueError by substring)."""
    return (INVALID, msg)


# ----------------------------------------------------------------------------------------------------------------------
# calling the entry points.  `op` holds what a case changes in the operator's own arguments:
#   cval, even (an even size / row count), origin (along the first filtered axis), empty (an all -1 footprint), mode
# ----------------------------------------------------------------------------------------------------------------------
def ints(*v):
    return (ctypes.c_int * len(v))(*v)


CROSS = (0, 1, 0)                                   # half widths of the rows of a 3 x 3 cross
SIX = (-1, 0, -1, 0, 1, 0, -1, 0, -1)               # 3 x 3 x 3, 6-connected, [dz][dy]


def call(lib, entry, xin, xout, op):
    a, b = ctypes.byref(xin._desc()), ctypes.byref(xout._desc())
    cval, mode = op.get("cval", 0), op.get("mode", 0)
    even, origin, empty = op.get("even", False), op.get("origin", 0), op.get("empty", False)
    if entry in ("minmax3d_u8", "minmax3d_16"):
        return getattr(lib, "mi_" + entry)(a, b, ints(3, 3, 2) if even else ints(3, 3, 3), ints(0, origin, 0), ints(mode, mode, mode), cval, 0, None)
    if entry == "minmax3d_u8_planes":
        planes = (ctypes.c_int64 * 2)(0, xin.shape[0] if xin.ndim == 3 else 1)
        return lib.mi_minmax3d_u8_planes(a, b, ints(2, 2, 2) if even else ints(3, 3, 3), ints(0, origin, 0), ints(mode, mode, mode), cval, 0, planes, 1, None)
    if entry in ("minmax_runs_u8", "minmax_runs_16"):
        hw = (-1, -1, -1) if empty else CROSS
        return getattr(lib, "mi_" + entry)(a, b, 2 if even else 3, ints(*hw), ints(mode, mode), cval, 0, None)
    if entry == "minmax_runs3d_u8":
        return lib.mi_minmax_runs3d_u8(a, b, ints(*((-1,) * 9 if empty else SIX)), ints(mode, mode, mode), cval, 0, None)
    if entry in ("uniform2d_u8", "uniform2d_16"):
        return getattr(lib, "mi_" + entry)(a, b, ints(2, 3) if even else ints(3, 3), origin, ints(mode, mode), cval, None)
    if entry in ("uniform_z_u8", "uniform_z_16"):
        return getattr(lib, "mi_" + entry)(a, b, 4 if even else 3, origin, mode, cval, None)
    assert entry == "median3x3"
    return lib.mi_median3x3(a, b, ints(mode, mode), float(cval), None)


def reference(entry, x, op):
    """What the accepted call computes, from the oracle (mode reflect, cval unused)."""
    origin = op.get("origin", 0)
    lead = (1,) * (x.ndim - 2)                      # images are one-plane volumes: the windows lie in the last two axes
    v = x.view(np.uint8) if x.dtype == np.bool_ else x
    if entry in ("minmax3d_u8", "minmax3d_16", "minmax3d_u8_planes"):
        return orc.minimum_filter(v, size=(3, 3, 3)[3 - x.ndim:])
    if entry in ("minmax_runs_u8", "minmax_runs_16"):
        fp = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool).reshape(lead + (3, 3))
        return orc.minimum_filter(v, footprint=fp)
    if entry == "minmax_runs3d_u8":
        fp = np.zeros((3, 3, 3), bool)
        fp[1, 1, :] = fp[1, :, 1] = fp[:, 1, 1] = True
        return orc.minimum_filter(v, footprint=fp)
    if entry in ("uniform2d_u8", "uniform2d_16"):
        return orc.uniform_filter(v, size=lead + (3, 3), origin=(0,) * len(lead) + (origin, 0))
    if entry in ("uniform_z_u8", "uniform_z_16"):
        return orc.uniform_filter(v, size=(3, 1, 1), origin=(origin, 0, 0))
    assert entry == "median3x3"
    p = np.pad(v, [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)], mode="symmetric")
    ny, nx = x.shape[-2:]
    win = np.stack([p[..., dy:dy + ny, dx:dx + nx] for dy in range(3) for dx in range(3)])
    return np.sort(win, axis=0)[4]


# ----------------------------------------------------------------------------------------------------------------------
# the arrays of a case: (input, output, host copy of the input)
# ----------------------------------------------------------------------------------------------------------------------
def plain(shape, dtype=None):
    def make(gpu, dt):
        dt = np.dtype(dtype or dt)
        rng = np.random.default_rng(7)
        x = rng.integers(0, 2, size=shape).astype(dt) if dt == np.bool_ else \
            rng.integers(np.iinfo(dt).min, int(np.iinfo(dt).max) + 1, size=shape).astype(dt)
        return gpu.asarray(x), gpu.empty(shape, dt), x
    return make


def aliased(shape):
    def make(gpu, dt):
        a = gpu.empty(shape, dt)
        return a, a, None
    return make


def strided(shape):
    """The input takes every other element of an allocation twice as wide."""
    def make(gpu, dt):
        wide = gpu.empty(shape[:-1] + (2 * shape[-1],), dt)
        item = np.dtype(dt).itemsize
        strides = tuple(2 * s for s in gpu.empty(shape, dt).strides[:-1]) + (2 * item,)
        view = gpu.ndarray(shape, dt, _mem=wide._mem, _ptr=wide.ptr, _strides=strides)
        return view, gpu.empty(shape, dt), None
    return make


def misaligned(shape):
    """The input starts 4 bytes into an allocation that is 16 bytes longer than the array."""
    def make(gpu, dt):
        item = np.dtype(dt).itemsize
        room = gpu.empty((int(np.prod(shape)) + 16 // item,), dt)
        view = gpu.ndarray(shape, dt, _mem=room._mem, _ptr=room.ptr + 4)
        return view, gpu.empty(shape, dt), None
    return make


def mismatched(shape_in, shape_out):
    def make(gpu, dt):
        return gpu.empty(shape_in, dt), gpu.empty(shape_out, dt), None
    return make


# ----------------------------------------------------------------------------------------------------------------------
# uint8: (case, arrays, op, {entry: outcome}); "*" is the outcome of every entry not named
# ----------------------------------------------------------------------------------------------------------------------
U8 = ("minmax3d_u8", "minmax3d_u8_planes", "minmax_runs_u8", "minmax_runs3d_u8", "uniform2d_u8", "uniform_z_u8")
X32, X64 = R("x extent must be a multiple of 16, >= 32"), R("x extent must be a multiple of 16, >= 64")
RANK3, RANK23, RANK3B = R("needs 3-D uint8 in/out"), R("needs 2-D / 3-D uint8 in/out"), R("needs 3-D uint8 / bool in/out")
RANK_U8 = {"*": RANK3, "minmax_runs_u8": RANK23, "uniform2d_u8": RANK23, "minmax_runs3d_u8": RANK3B}
V64 = (2, 2, 64)

U8_CASES = [
    ("nx16", plain((2, 2, 16)), {}, {"*": X32, "minmax3d_u8_planes": X64}),
    ("nx32", plain((2, 2, 32)), {}, {"*": ACCEPT, "minmax3d_u8_planes": X64}),
    ("nx40", plain((2, 2, 40)), {}, {"*": X32, "minmax3d_u8_planes": X64}),      # minmax3d_u8: the ragged route refuses first (small volume)
    ("nx48", plain((2, 2, 48)), {}, {"*": ACCEPT, "minmax3d_u8_planes": X64}),
    ("nx64", plain(V64), {}, {"*": ACCEPT}),
    ("nx1040", plain((2, 2, 1040)), {}, {"*": X32, "minmax3d_u8_planes": X64, "uniform_z_u8": ACCEPT}),     # (nx & 1023) == 16; uniform_z has no x window
    ("rank1", plain((64,)), {}, RANK_U8),
    ("rank2", plain((4, 64)), {}, dict(RANK_U8, minmax_runs_u8=ACCEPT, uniform2d_u8=ACCEPT)),
    ("rank4", plain((1, 2, 2, 64)), {}, RANK_U8),
    ("uint16", plain(V64, np.uint16), {}, RANK_U8),
    ("bool", plain(V64, np.bool_), {}, dict(RANK_U8, minmax_runs3d_u8=ACCEPT)),
    ("in-place", aliased(V64), {}, {"*": R("in-place"), "minmax3d_u8_planes": R("needs distinct C-contiguous arrays")}),
    ("strided", strided(V64), {}, {"*": R("needs C-contiguous arrays"), "minmax3d_u8_planes": R("needs distinct C-contiguous arrays")}),
    ("misaligned", misaligned(V64), {}, {"*": R("needs 16-byte aligned data")}),
    ("cval-1", plain(V64), {"cval": -1}, {"*": R("cval outside uint8")}),
    ("cval256", plain(V64), {"cval": 256}, {"*": R("cval outside uint8")}),
    ("even", plain(V64), {"even": True}, {
        "minmax3d_u8": R("sizes must be odd with origin 0"), "minmax3d_u8_planes": R("cubic sizes 3 / 5 / 7 only"),
        "minmax_runs_u8": R("1, 3, 5, 7 or 9 footprint rows"), "minmax_runs3d_u8": NA,
        "uniform2d_u8": R("sizes must be odd and <= 9"), "uniform_z_u8": R("odd size 3 .. 9")}),
    ("origin1", plain(V64), {"origin": 1}, {
        "minmax3d_u8": R("sizes must be odd with origin 0"), "minmax3d_u8_planes": R("origin must be 0"),
        "minmax_runs_u8": NA, "minmax_runs3d_u8": NA, "uniform2d_u8": ACCEPT, "uniform_z_u8": ACCEPT}),
    ("origin2", plain(V64), {"origin": 2}, {
        "minmax3d_u8": R("sizes must be odd with origin 0"), "minmax3d_u8_planes": R("origin must be 0"),
        "minmax_runs_u8": NA, "minmax_runs3d_u8": NA, "uniform2d_u8": BAD("invalid origin"), "uniform_z_u8": BAD("invalid origin")}),
    ("shape", mismatched(V64, (2, 2, 32)), {}, {"*": BAD("output shape is not correct")}),
    ("empty", plain(V64), {"empty": True}, {"*": NA, "minmax_runs_u8": R("empty footprint"), "minmax_runs3d_u8": R("empty footprint")}),
]

# ----------------------------------------------------------------------------------------------------------------------
# uint16 / int16; the prefix of mi_median3x3 is "median3x3"
# ----------------------------------------------------------------------------------------------------------------------
S16 = ("minmax3d_16", "minmax_runs_16", "uniform2d_16", "uniform_z_16", "median3x3")
X16 = R("x extent must be a multiple of 8, >= 16")
RANK16 = R("needs 2-D / 3-D uint16 or int16 in/out")
W16 = (2, 2, 32)
CVAL16 = {"*": R("cval outside the dtype"), "median3x3": R("cval is not a value of the dtype")}      # the median looks at cval in constant mode only


def s16_cases(dt):
    lo, hi = (-32769, 32768) if dt == np.int16 else (-1, 65536)
    return [
        ("nx8", plain((2, 2, 8)), {}, {"*": X16}),
        ("nx16", plain((2, 2, 16)), {}, {"*": ACCEPT}),
        ("nx20", plain((2, 2, 20)), {}, {"*": X16}),                             # minmax3d_16: the ragged route refuses first (small volume)
        ("nx24", plain((2, 2, 24)), {}, {"*": ACCEPT}),
        ("nx520", plain((2, 2, 520)), {}, {"*": R("x extent unsuitable for the streaming x window")}),      # a last tile of 8 pixels: one lane
        ("rank1", plain((32,)), {}, {"*": RANK16}),
        ("rank2", plain((4, 32)), {}, {"*": ACCEPT, "uniform_z_16": R("needs a volume")}),
        ("rank4", plain((1, 2, 2, 32)), {}, {"*": RANK16}),
        ("int32", plain(W16, np.int32), {}, {"*": RANK16, "median3x3": R("needs 2-D / 3-D float32, float64, uint8, uint16 or int16 in/out")}),
        ("in-place", aliased(W16), {}, {"*": R("in-place")}),
        ("strided", strided(W16), {}, {"*": R("needs C-contiguous arrays")}),
        ("misaligned", misaligned(W16), {}, {"*": R("needs 16-byte aligned data")}),
        ("cval-lo", plain(W16), {"cval": lo, "mode": 1}, CVAL16),
        ("cval-hi", plain(W16), {"cval": hi, "mode": 1}, CVAL16),
        ("even", plain(W16), {"even": True}, {
            "minmax3d_16": R("sizes must be odd, <= 9, with origin 0"), "minmax_runs_16": R("1, 3, 5, 7 or 9 footprint rows"),
            "uniform2d_16": R("sizes must be odd and <= 9"), "uniform_z_16": R("odd size 3 .. 9"), "median3x3": NA}),
        ("origin1", plain(W16), {"origin": 1}, {
            "minmax3d_16": R("sizes must be odd, <= 9, with origin 0"), "minmax_runs_16": NA, "uniform2d_16": ACCEPT, "uniform_z_16": ACCEPT,
            "median3x3": NA}),
        ("origin2", plain(W16), {"origin": 2}, {
            "minmax3d_16": R("sizes must be odd, <= 9, with origin 0"), "minmax_runs_16": NA, "uniform2d_16": BAD("invalid origin"),
            "uniform_z_16": BAD("invalid origin"), "median3x3": NA}),
        ("shape", mismatched(W16, (2, 2, 16)), {}, {"*": BAD("output shape is not correct")}),
        ("empty", plain(W16), {"empty": True}, {"*": NA, "minmax_runs_16": R("empty footprint")}),
    ]


def run_family(gpu, entries, cases, dt):
    from cupyimg_amd import _lib
    lib = _lib.load()
    wrong = []
    for name, arrays, op, expect in cases:
        xin, xout, host = arrays(gpu, dt)
        for entry in entries:
            want = expect.get(entry, expect.get("*"))
            assert want is not None, (name, entry)
            if want == NA:
                continue
            rc = call(lib, entry, xin, xout, op)
            text = _lib.last_error() if rc != OK else ""
            print("{:20s} {:12s} rc={:2d} {}".format(entry, name, rc, text))
            if want == ACCEPT:
                if rc != OK:
                    wrong.append((entry, name, "refused", rc, text))
                elif not np.array_equal(xout.get().view(np.uint8), reference(entry, host, op).view(np.uint8)):
                    wrong.append((entry, name, "result differs from the oracle"))
                continue
            code, msg = want
            full = msg if code == INVALID else "{}: {}".format(entry, msg)
            if (rc, text) != (code, full):
                wrong.append((entry, name, "got", rc, text, "expected", code, full))
    assert not wrong, wrong


def test_uint8_gates(gpu):
    run_family(gpu, U8, U8_CASES, np.uint8)


@pytest.mark.parametrize("dt", [np.uint16, np.int16], ids=["uint16", "int16"])
def test_16bit_gates(gpu, dt):
    run_family(gpu, S16, s16_cases(dt), dt)
