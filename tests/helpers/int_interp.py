"""Integer images through the interpolation family (affine_transform, map_coordinates, shift, zoom, rotate), judged against
SciPy's integer path: the generators, SciPy's rounding rule, the unrounded (float64) result, the band around .5 ties
and the table of cases.

Test infrastructure (host only: NumPy and SciPy): used by tests/test_int_interp_yardstick.py, which proves every piece
on SciPy alone and holds the CPU oracle to it, and by tests/test_gpu_int_interp.py, never by the package.

The contract.  With an integer output SciPy interpolates in double, rounds half away from zero and saturates
(`round_like_scipy`).  A device result has to EQUAL SciPy's, output for output.  The only outputs excused are those
whose unrounded value u lies so close to a .5 tie that two correct double evaluations may round apart:

    | |u| mod 1 - 0.5 | <= band,      band = interp_c(ndim, order) . 2^-53 . B + coordinate term

(`tie_band`; B = |coefficients| interpolated with the same weights, as in tests/test_gpu_value_ranges.py with u = 2^-24).
The band is derived from the arithmetic, never fitted to a device; on 16-bit data it is about 1e-8, so it excuses less
than one output per case (`CAP` is a condition on the inputs: a case whose excused share exceeds it is no test).  Even
an excused output may differ by one at the most.  For order 0 no arithmetic is rounded, only the choice of the sample:
the excused outputs are those with a coordinate within the coordinate rounding of a half-integer.
Cases built on exact ties (order 1 at dyadic positions: every value is a multiple of 1/64, exact in double) are compared
with no band at all.
"""
import functools
import warnings

import numpy as np
import scipy.ndimage as sndi
import scipy.special as ssp

from helpers import value_ranges as vr

NPAD = 12                 # SciPy's pad for `nearest` / `grid-constant` before the prefilter
CAP = 1e-3                # largest share of outputs of one case that the band may excuse
SMALL, LARGE = (9, 12, 14), (24, 40, 61)
MODES = ("constant", "grid-constant", "nearest", "mirror", "reflect", "wrap", "grid-wrap")


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def _as3(shape):
    """The 3-D shape the generators of value_ranges.py are asked for: leading ones added, leading axes merged."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 3:
        return (1,) * (3 - len(shape)) + shape
    return (int(np.prod(shape[:-2])),) + shape[-2:]


def int_extremes(shape, dtype, seed=0):
    """vr.int_extremes at any rank and for any integer dtype up to 32 bits (uint8, int8, int32 besides the 16-bit ones)."""
    return vr.int_extremes(_as3(shape), dtype, seed).reshape(shape)


def ct_as(shape, dtype, seed=0):
    """CT Hounsfield units (vr.ct_hu, int16) stored in a wider type: as they are in int64, moved up by 32768 (so that
    the -32768 padding becomes 0) in uint32 / uint64.  For the dtype plumbing only: far below 2^53, so every value is
    exact in double."""
    hu = vr.ct_hu(_as3(shape), seed).reshape(shape).astype(np.int64)
    dtype = np.dtype(dtype)
    return (hu + 32768 if dtype.kind == "u" else hu).astype(dtype)


def mask(shape, seed=0):
    """A bool mask: tissue and bone of the CT phantom."""
    return vr.ct_hu(_as3(shape), seed).reshape(shape) > 0


_KINDS = {
    "ct_i16": lambda s: vr.ct_hu(_as3(s), seed=31).reshape(s),
    "mr_u16": lambda s: vr.mr_u12(_as3(s), seed=32).reshape(s),
    "ext_i16": lambda s: int_extremes(s, np.int16, seed=33),
    "ext_u16": lambda s: int_extremes(s, np.uint16, seed=34),
    "ext_u8": lambda s: int_extremes(s, np.uint8, seed=35),
    "ext_i8": lambda s: int_extremes(s, np.int8, seed=36),
    "ext_i32": lambda s: int_extremes(s, np.int32, seed=37),
    "ext_i32s": lambda s: int_extremes(s, np.int32, seed=37) >> 8,          # the same image on 24 bits
    "ct_i64": lambda s: ct_as(s, np.int64, seed=38),
    "ct_u32": lambda s: ct_as(s, np.uint32, seed=39),
    "ct_u64": lambda s: ct_as(s, np.uint64, seed=40),
    "ct_f32": lambda s: vr.ct_hu(_as3(s), seed=41, dtype=np.float32).reshape(s),
    "mask": lambda s: mask(s, seed=42),
}
DTYPE_KINDS = ("ct_i16", "mr_u16", "ext_i16", "ext_u16", "ext_u8", "ext_i8", "ext_i32", "ct_i64", "ct_u32", "ct_u64")
# an in-range integral fill value per image (97, not 100: blended with the 0 of the CT padding at the general matrix's
# weight 0.135 along z, 100 gives 13.5 -- rows of ties that are an accident of the inputs)
CVAL = {"ct_i16": -1000.0, "ct_i64": -1000.0, "ct_f32": -1000.0, "ext_i16": -100.0, "ext_i8": -100.0, "ext_i32": -100.0, "ext_i32s": -100.0,
        "mr_u16": 97.0, "ext_u16": 97.0, "ext_u8": 97.0, "ct_u32": 97.0, "ct_u64": 97.0, "mask": 0.0}


@functools.lru_cache(maxsize=None)
def data(kind, shape):
    x = np.ascontiguousarray(_KINDS[kind](tuple(shape)))
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# SciPy's rounding
# ---------------------------------------------------------------------------------------------------------------------
def round_like_scipy(t, dtype):
    """CASE_INTERP_OUT_INT / _UINT of SciPy's ni_interpolation.c: signed `t > 0 ? t + 0.5 : t - 0.5`, unsigned
    `t > 0 ? t + 0.5 : 0`, clipped to the range of the type, truncated; bool `t != 0`; a float type is a plain cast."""
    dtype = np.dtype(dtype)
    t = np.asarray(t, np.float64)
    if dtype.kind == "b":
        return t != 0
    if dtype.kind == "f":
        return t.astype(dtype)
    info = np.iinfo(dtype)
    r = np.where(t > 0, t + 0.5, t - 0.5 if dtype.kind == "i" else 0.0)
    lo, hi = float(info.min), float(info.max)
    if dtype.itemsize == 8:
        hi = np.nextafter(hi, 0.0)          # 2^63 / 2^64 are not values of the type (beyond 2^53: out of scope anyway)
    return np.trunc(np.clip(r, lo, hi)).astype(dtype)


def representable(cval, dtype):
    """Whether casting cval to dtype (NumPy's assignment, as np.pad does it) leaves it unchanged."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return bool(np.asarray(cval, np.float64).astype(dtype).astype(np.float64) == float(cval))
        except (OverflowError, ValueError):
            return False


# ---------------------------------------------------------------------------------------------------------------------
# the unrounded result
# ---------------------------------------------------------------------------------------------------------------------
def _quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # zoom's grid_mode advice, the 1-D matrix notice
        return fn(*args, **kw)


def _settings(kw):
    return int(kw.get("order", 3)), kw.get("mode", "constant"), float(kw.get("cval", 0.0)), bool(kw.get("prefilter", True))


def pad_cast(x, order, mode, cval, prefilter):
    """True in the one cell where SciPy's result is NOT the rounded result of its float64 path: order >= 2 in
    `grid-constant` pads the image by 12 samples of cval BEFORE the prefilter, in the image's own dtype, so the ring
    holds cval cast to that dtype (-1000.3 -> -1000 in int16, float32(-1000.3) in float32); the taps beyond the ring
    read the true cval."""
    return order >= 2 and prefilter and mode == "grid-constant" and not representable(cval, x.dtype)


def unrounded(fn, x, *args, **kw):
    """What SciPy's `fn(x, *args, **kw)` computes before it rounds into the output: the same call on x.astype(float64)
    with output=float64.  In the pad-cast cell: pad x as SciPy does (np.pad on x's dtype), prefilter in double, and call
    with prefilter=False, the true cval and the positions moved by the 12 samples."""
    name = fn if isinstance(fn, str) else fn.__name__
    f = getattr(sndi, name)
    kw = dict(kw, output=np.float64)
    order, mode, cval, prefilter = _settings(kw)
    x = np.asarray(x)
    if not pad_cast(x, order, mode, cval, prefilter):
        return _quiet(f, x.astype(np.float64), *args, **kw)
    p = np.pad(x, NPAD, mode="constant", constant_values=cval)
    coef = sndi.spline_filter(p.astype(np.float64), order, output=np.float64, mode=mode)
    kw["prefilter"] = False
    if name == "affine_transform":
        kw["offset"] = np.broadcast_to(np.asarray(kw.get("offset", 0.0), np.float64), (x.ndim,)) + float(NPAD)
        kw.setdefault("output_shape", x.shape)
        return _quiet(f, coef, *args, **kw)
    if name == "map_coordinates":
        return _quiet(f, coef, np.asarray(args[0], np.float64) + float(NPAD), *args[1:], **kw)
    if name == "shift":
        return _quiet(f, coef, *args, **kw)[(slice(NPAD, -NPAD),) * x.ndim]
    raise NotImplementedError("the pad-cast cell is restated for affine_transform, map_coordinates and shift")


# ---------------------------------------------------------------------------------------------------------------------
# geometry: where every output samples the input
# ---------------------------------------------------------------------------------------------------------------------
def general(shape):
    """The general matrix of tests/test_gpu_value_ranges.py (`_m30`: 30 degrees in the plane of the first two axes
    times a scaling per axis), centred on the volume and moved by (0.5, -1.25, 2.0), at any rank."""
    n = len(shape)
    M = np.eye(n)
    if n >= 2:
        a = np.deg2rad(30.0)
        M[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    # rank 1: an irrational scale -- with 0.97 every weight is a multiple of 1/200, and on integers those tie by the dozen
    M = M @ np.diag([1.0, 0.97, 1.03, 0.94][:n] if n > 1 else [np.sqrt(0.94)])
    ctr = (np.asarray(shape, np.float64) - 1) / 2.0
    return M, ctr - M @ ctr + np.asarray([0.5, -1.25, 2.0, 0.75][:n])


def _affine_positions(M, off, out_shape):
    """(positions, their rounding): c = M o + off, and per axis (2 ndim + 2) . 2^-53 . (|M| o + |off| + 2): SciPy and
    the device each round ndim products and ndim sums of partial results no larger than that."""
    n = len(out_shape)
    idx = np.indices(out_shape, dtype=np.float64).reshape(n, -1)
    off = np.asarray(off, np.float64)
    c = (M @ idx + off[:, None]).reshape((n,) + tuple(out_shape))
    s = (np.abs(M) @ idx + np.abs(off)[:, None]).reshape(c.shape)
    return c, (2 * n + 2) * vr.U64 * (s + 2.0)


def positions(name, x, out_shape, *args, **kw):
    """Input coordinates (ndim, *out_shape) of every output of the call and the rounding they carry."""
    n = x.ndim
    if name == "map_coordinates":
        c = np.asarray(args[0], np.float64)           # handed over as data: the same on both sides
        return c, np.zeros_like(c)
    if name == "affine_transform":
        M = np.asarray(args[0], np.float64)
        M = np.diag(M) if M.ndim == 1 else M
        off = np.broadcast_to(np.asarray(kw.get("offset", 0.0), np.float64), (n,))
        return _affine_positions(M, off, out_shape)
    if name == "shift":
        return _affine_positions(np.eye(n), -np.broadcast_to(np.asarray(args[0], np.float64), (n,)), out_shape)
    if name == "zoom":
        if kw.get("grid_mode", False):
            sc = np.array([i / o for i, o in zip(x.shape, out_shape)])
            return _affine_positions(np.diag(sc), 0.5 * sc - 0.5, out_shape)
        sc = np.array([(i - 1) / (o - 1) if o > 1 else 1.0 for i, o in zip(x.shape, out_shape)])
        return _affine_positions(np.diag(sc), np.zeros(n), out_shape)
    if name == "rotate":
        axes = sorted(a % n for a in kw.get("axes", (1, 0)))
        c, s = float(ssp.cosdg(args[0])), float(ssp.sindg(args[0]))
        rot = np.array([[c, s], [-s, c]])
        in_c = (np.asarray(x.shape, np.float64)[axes] - 1) / 2
        off2 = in_c - rot @ ((np.asarray(out_shape, np.float64)[axes] - 1) / 2)
        M, off = np.eye(n), np.zeros(n)
        M[np.ix_(axes, axes)] = rot
        off[axes] = off2
        return _affine_positions(M, off, out_shape)
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------------------------
# the band
# ---------------------------------------------------------------------------------------------------------------------
def _coefficients(x, order, mode, cval, prefilter):
    """(float64 coefficients as SciPy builds them, npad)"""
    if order < 2 or not prefilter:
        return np.asarray(x, np.float64), 0
    npad = NPAD if mode in ("nearest", "grid-constant") else 0
    if mode == "nearest":
        x = np.pad(x, NPAD, mode="edge")
    elif mode == "grid-constant":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x = np.pad(x, NPAD, mode="constant", constant_values=cval)
    return sndi.spline_filter(np.asarray(x, np.float64), order, output=np.float64, mode=mode), npad


def _largest_steps(coef, mode, cval):
    """Per axis the largest |coef[i + 1] - coef[i]| (in the constant modes the step to cval at the ends, in the wrapping
    ones the step from the last sample to the first too): an upper bound of the local step vr.coord_term looks up."""
    out = []
    for a in range(coef.ndim):
        L = float(np.abs(np.diff(coef, axis=a)).max()) if coef.shape[a] > 1 else 0.0
        if mode in ("constant", "grid-constant"):
            L = max(L, float(np.abs(np.take(coef, [0, -1], axis=a) - cval).max()))
        elif mode in ("wrap", "grid-wrap"):
            L = max(L, float(np.abs(np.take(coef, 0, axis=a) - np.take(coef, -1, axis=a)).max()))
        out.append(L)
    return out


def tie_band(name, x, coords, *args, **kw):
    """Per-output half-width within which two correct double evaluations may land on either side of a .5 tie:
    vr.interp_c(ndim, order) . 2^-53 . B + the coordinate term with u = 2^-53.  B: |coefficients| (SciPy's 12-sample pad
    included where it applies) interpolated at the same positions with prefilter=False and |cval|.  Coordinate term:
    vr.coord_term in the modes it folds (`constant`, `mirror`); in the others the same sum, 2u (|c_a| + 2) L_a over the axes,
    with the largest step of the whole axis for L_a -- never smaller than the local one."""
    order, mode, cval, prefilter = _settings(kw)
    x = np.asarray(x)
    coef, npad = _coefficients(x, order, mode, cval, prefilter)
    B = sndi.map_coordinates(np.abs(coef), coords + float(npad), output=np.float64, order=order, mode=mode, cval=abs(cval),
                             prefilter=False)
    if npad == 0 and mode in ("constant", "mirror"):
        T = vr.coord_term(coef, coords, order, mode, cval, u=vr.U64)
    else:
        T = np.zeros(coords.shape[1:])
        for a, L in enumerate(_largest_steps(coef, mode, cval)):
            T += 2.0 * vr.U64 * (np.abs(coords[a]) + 2.0) * L
    return vr.interp_c(x.ndim, order) * vr.U64 * B + T


def excused(u, band, half=None):
    """The outputs the band excuses: | |u| mod 1 - 0.5 | <= band; with `half` (order 0) that mask instead."""
    if half is not None:
        return np.asarray(half, bool)
    return np.abs(np.abs(np.asarray(u, np.float64)) % 1.0 - 0.5) <= band


def compare(got, want, u=None, band=None, half=None):
    """Asserts got == want at every output that is not excused, |got - want| <= 1 at the excused ones, and that the
    excused share is within CAP.  u None (with half None): nothing is excused.  Returns the number excused."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if u is None and half is None:
        ex = np.zeros(want.shape, bool)
    else:
        ex = excused(u, band, half)
        assert ex.shape == want.shape, (ex.shape, want.shape)
        assert ex.mean() <= CAP, "the band excuses %.2e of the outputs: the case is no test" % ex.mean()
    if want.dtype.kind == "b":
        bad, far = (got != want) & ~ex, np.zeros(want.shape, bool)
    else:
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))      # exact below 2^53
        bad, far = (d != 0) & ~ex, (d > 1) & ex
    if bad.any() or far.any():
        at = np.unravel_index(int(np.argmax(bad | far)), want.shape)
        raise AssertionError("%d of %d outputs differ outside the band, %d excused ones by more than one; first at %s: got %r, "
                             "want %r, unrounded %r" % (int(bad.sum()), want.size, int(far.sum()), at, got[at], want[at],
                                                        None if u is None else float(np.asarray(u)[at])))
    return int(ex.sum())


def compare_float(got, want, band):
    """A float output: no rounding to an integer, |got - want| <= band (the double bound), plus one rounding of the
    reference for a float32 output."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    w = want.astype(np.float64)
    tol = band + (vr.U32 * np.abs(w) if want.dtype == np.float32 else 0.0)
    r = np.abs(got.astype(np.float64) - w) / (tol + vr.TINY)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    assert r[at] <= 1.0, "%.3g times the bound at %s: got %r, want %r" % (r[at], at, got[at], want[at])
    return float(r[at])


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One call: `fn(data(kind, shape), *args, **kw)`.  `coords`: map_coordinates takes the positions of the general
    matrix as "f64" / "f32" device arrays or as a "host" array.  `output`: None, a dtype, or ("prealloc", dtype).
    `exact`: built on exact ties -- no band.  `tags`: what the yardstick holds the case to (saturates, dyadic, padcast)."""

    def __init__(self, group, fn, kind, shape, args=(), coords=None, output=None, exact=False, tags=(), **kw):
        self.group, self.fn, self.kind, self.shape = group, fn, kind, tuple(shape)
        self.args, self.coords, self.output, self.exact, self.tags, self.kw = tuple(args), coords, output, exact, frozenset(tags), kw

    @property
    def id(self):
        a = ",".join(_short(v) for v in self.args)
        k = ",".join("%s=%s" % (n, _short(v)) for n, v in sorted(self.kw.items()))
        o = "" if self.output is None else "->%s" % _short(self.output)
        return "%s(%s%s)[%s]%s%s" % (self.fn, self.kind + "x".join(map(str, self.shape)), "," + a if a else "", k, o,
                                     "," + self.coords if self.coords else "")

    @property
    def x(self):
        return data(self.kind, self.shape)

    @property
    def order(self):
        return _settings(self.kw)[0]

    @property
    def out_dtype(self):
        if self.output is None:
            return self.x.dtype
        return np.dtype(self.output[1] if isinstance(self.output, tuple) else self.output)

    def host_args(self):
        if self.fn != "map_coordinates":
            return self.args
        M, off = general(self.shape)
        c, _ = _affine_positions(M, off, self.shape)
        return (np.ascontiguousarray(c, np.float32 if self.coords == "f32" else np.float64),)

    def call(self, module, x, out_shape=None):
        """The call on a host module with SciPy's signatures (scipy.ndimage, the CPU oracle)."""
        kw = dict(self.kw)
        if isinstance(self.output, tuple):
            kw["output"] = np.zeros(out_shape, self.output[1])
        elif self.output is not None:
            kw["output"] = self.output
        return _quiet(getattr(module, self.fn), x, *self.host_args(), **kw)

    def scipy(self):
        """SciPy's own result: the reference."""
        want = self.call(sndi, self.x, self.x.shape)
        return want

    def device(self, gpu, ndi, out_shape):
        """The same call on the device; the result on the host."""
        kw = dict(self.kw)
        if isinstance(self.output, tuple):
            kw["output"] = gpu.asarray(np.zeros(out_shape, self.output[1]))
        elif self.output is not None:
            kw["output"] = self.output
        args = self.host_args()
        if self.fn == "map_coordinates" and self.coords != "host":
            args = (gpu.asarray(args[0]),)
        return _quiet(getattr(ndi, self.fn), gpu.asarray(self.x), *args, **kw).get()

    def evidence(self):
        """(u, band, half): the unrounded result, the tie band (None for order 0) and, for order 0, the outputs with a
        coordinate within its rounding of a half-integer."""
        x, args = self.x, self.host_args()
        u = unrounded(self.fn, x, *args, **self.kw)
        coords, cband = positions(self.fn, x, u.shape, *args, **self.kw)
        if self.order == 0:
            return u, None, (np.abs(np.abs(coords) % 1.0 - 0.5) <= cband).any(axis=0)
        if self.order == 1 and np.array_equal(coords * 64.0, np.rint(coords * 64.0)) and np.abs(x).max() < 2 ** 31:
            # every position a multiple of 1/64: weights, products and sums are exact in double on both sides (a zoom by
            # 2 or 0.5 with grid_mode, a rotation by 90 degrees) -- the ties are exact ones and nothing is excused
            return u, None, None
        return u, tie_band(self.fn, x, coords, *args, **self.kw), None

    def check(self, got, want, evidence=None):
        """`got` against SciPy's `want` under the contract of this module.  The evidence is only worked out when an
        output differs (or handed in by a caller that has it)."""
        if self.exact:
            return compare(got, want)
        if self.out_dtype.kind == "f":
            u, band, _ = evidence or self.evidence()
            return compare_float(got, want, band)
        if evidence is None and got.dtype == want.dtype and np.array_equal(got, want):
            return 0
        u, band, half = evidence or self.evidence()
        if band is None and half is None:
            return compare(got, want)
        return compare(got, want, u, band, half)


def _short(v):
    if isinstance(v, np.ndarray):
        return "m%s" % "x".join(map(str, v.shape))
    if isinstance(v, type):
        return v.__name__
    if isinstance(v, tuple):
        return "(" + " ".join(_short(i) for i in v) + ")"
    return str(v)


def _affine(group, kind, shape, **kw):
    M, off = general(shape)
    kw.setdefault("cval", CVAL[kind])
    return Case(group, "affine_transform", kind, shape, (M,), offset=off, **kw)


# An order-1 result on integers at positions with a small common denominator q is a multiple of 1 / q: for even q that is
# not a power of two it ties by the dozen, and the positions (0.3, 1.2 o + 0.1, ...) are not exact in double, so the ties
# are only near ones -- the inputs then miss the cap.  The shift is irrational for that reason.
SHIFT = (float(np.sqrt(0.1)), -float(np.sqrt(2.6)), float(np.sqrt(5.0)))


# SciPy itself refuses these (np.pad of a 16-bit image with a value beyond its range raises OverflowError: "Python
# integer 1000000 out of bounds for int16"), so they are no part of the table; the yardstick checks that it still does.
def refused_by_scipy():
    return [_affine("fill", "ct_i16", SMALL, order=3, mode="grid-constant", cval=c) for c in (1e6, -1e6)]


@functools.lru_cache(maxsize=None)
def table():
    """Every case, as a tuple; the GPU tests and the yardstick walk the same one."""
    T = []
    # every dtype through the general affine transform: every order and mode on the small volume, orders 0, 1, 3, 5 on the
    # one with ragged rows and more than one block per axis
    # int32 at full range: a double keeps 22 bits below such a value and a spline of order >= 3 spends them -- the derived
    # band reaches 4e-4 (order 3), 1.2e-3 (4) and 3.4e-3 .. 1.2e-2 (5) and would excuse up to 1.4 % of a case, past the
    # cap.  Orders 0 .. 2 run at full range; orders 3 .. 5 run on the same image moved down to 24 bits, and the clamp at
    # the int32 limits is reached through fill values beyond them (the `fill` cases below).
    for kind in DTYPE_KINDS:
        for shape, orders in ((SMALL, (0, 1, 2, 3, 4, 5)), (LARGE, (0, 1, 3, 5))):
            for order in orders:
                k = "ext_i32s" if kind == "ext_i32" and order >= 3 else kind
                sat = ("saturates",) if k.startswith("ext_") and k != "ext_i32s" and order >= 3 else ()
                for mode in MODES + (("grid-mirror",) if shape == SMALL and order == 3 else ()):
                    T.append(_affine("dtypes", k, shape, order=order, mode=mode, tags=sat))
    # fill values: fractional ones, and ones beyond the output range
    for kind in ("ct_i16", "ext_u8"):
        for mode in ("constant", "grid-constant"):
            for order in (1, 3):
                for cval in (-1000.3, -1000.7, 100.7, 1e6, -1e6):
                    if kind == "ct_i16" and order == 3 and mode == "grid-constant" and abs(cval) == 1e6:
                        continue                      # refused_by_scipy()
                    tags = (("padcast",) if order == 3 and mode == "grid-constant" and cval in (-1000.3, -1000.7, 100.7) else ()) \
                        + (("saturates",) if abs(cval) == 1e6 else ())
                    T.append(_affine("fill", kind, SMALL, order=order, mode=mode, cval=cval, tags=tags))
    for order in (1, 3):
        for cval in (3e9, -3e9):
            T.append(_affine("fill", "ext_i32s", SMALL, order=order, mode="constant", cval=cval, tags=("saturates",)))
    T.append(_affine("fill", "ct_i16", LARGE, order=3, mode="grid-constant", cval=-1000.3, tags=("padcast",)))
    T.append(_affine("fill", "ct_f32", SMALL, order=3, mode="grid-constant", cval=-1000.3, output=np.float64, tags=("padcast",)))
    # exact ties: order 1 at dyadic positions, no band
    for kind, shape in (("ct_i16", LARGE), ("ext_u16", SMALL)):
        T.append(Case("ties", "shift", kind, shape, ((0.5, 0.25, -0.5),), order=1, exact=True, tags=("ties",)))
        T.append(Case("ties", "zoom", kind, shape, (2.0,), order=1, grid_mode=True, exact=True, tags=("ties",)))
        T.append(Case("ties", "affine_transform", kind, shape, (np.array([0.5, 0.5, 0.5]),), order=1, exact=True,
                      tags=("ties", "dyadic")))
    # the rest of the family
    for kind in ("ct_i16", "mr_u16"):
        cv = CVAL[kind]
        for order in (1, 3):
            for mode in ("constant", "mirror"):
                T.append(Case("family", "shift", kind, SMALL, (SHIFT,), order=order, mode=mode, cval=cv))
                for ck in ("f64", "f32", "host"):
                    T.append(Case("family", "map_coordinates", kind, SMALL, coords=ck, order=order, mode=mode, cval=cv))
            for z in (2.0, 0.5, (1.3, 0.8, 1.0)):
                for grid in (False, True):
                    # another volume where the small one's positions have a small even denominator (see SHIFT): the large
                    # one (odd denominators), or 9 x 10 x 14 -> 12 x 8 x 14 (steps 0.75, 1.25, 1: exact)
                    shape = LARGE if (z, grid) == (0.5, False) else (9, 10, 14) if (z, grid) == ((1.3, 0.8, 1.0), True) else SMALL
                    T.append(Case("family", "zoom", kind, shape, (z,), order=order, cval=cv,
                                  **(dict(mode="grid-constant", grid_mode=True) if grid else dict(mode="nearest"))))
            for angle in (30.0, 90.0, -17.5):
                for axes in ((1, 0), (1, 2), (0, 2)):
                    for reshape in (True, False):
                        shape = LARGE if (angle, axes, reshape) == (30.0, (0, 2), True) else SMALL
                        T.append(Case("family", "rotate", kind, shape, (angle,), axes=axes, reshape=reshape, order=order, cval=cv))
        for order in (2, 3, 4, 5):
            for mode in ("constant", "mirror"):
                T.append(_affine("family", kind, SMALL, order=order, mode=mode, prefilter=False))
    # an output dtype other than the input's
    for order in (1, 3):
        for mode in ("constant", "mirror"):
            s = dict(order=order, mode=mode)
            T.append(_affine("output", "ct_f32", SMALL, output=np.int16, **s))
            T.append(_affine("output", "ct_f32", SMALL, output=np.uint8, tags=("saturates",), **s))
            T.append(_affine("output", "ct_i16", SMALL, output=np.uint8, tags=("saturates",), **s))
            T.append(_affine("output", "ct_i16", SMALL, output=np.float64, **s))
            T.append(_affine("output", "ct_i16", SMALL, output=np.float32, **s))
            T.append(_affine("output", "ct_i16", SMALL, output=("prealloc", np.int16), **s))
    # ranks other than 3 and short axes, int16 in and out
    for shape in ((1, 12, 14), (6, 1, 7), (2, 2, 2), (40,), (21, 26), (5, 6, 7, 8)):
        for order in (1, 3):
            for mode in ("constant", "nearest", "mirror", "grid-wrap"):
                T.append(_affine("ranks", "ct_i16", shape, order=order, mode=mode))
    # bool: order 0 (the general matrix keeps the positions off the half-integers)
    for shape in (SMALL, (21, 26)):
        for mode, cval in (("constant", 0.0), ("constant", 1.0), ("nearest", 0.0)):
            for output in (None, np.uint8):
                T.append(_affine("bool", "mask", shape, order=0, mode=mode, cval=cval, output=output))
    ids = [c.id for c in T]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:5]
    return tuple(T)


def buckets(groups=None):
    """The table cut into test-sized pieces: {id: [cases]}, one per (group, image, shape, order)."""
    out = {}
    for c in table():
        if groups is None or c.group in groups:
            out.setdefault("%s-%s-%s-o%d" % (c.group, c.kind, "x".join(map(str, c.shape)), c.order), []).append(c)
    return out
