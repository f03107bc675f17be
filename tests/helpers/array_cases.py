"""Inputs and expectations for the tests of the array layer (casts, strided copies, fills, reductions); pure NumPy.

Value ladders
    `ladder(dtype)`: the edges at which a cast can go wrong (type limits, the 8 / 16 / 24 / 31 / 32 / 53 / 63 bit
    boundaries and, for floats, signed zeros, halves, subnormals, infinities, NaN), every one of them that the dtype holds.
    `f16_all()` is every float16 bit pattern.

Admission rule, `admitted(values, target)` -- which (source value, target dtype) pairs have a defined result:
    integer -> anything      always (modular between integers, round to nearest even into floats);
    float -> integer         when the truncated value fits the target; also a negative value with |v| < 2**63 into an
                             unsigned target, where the result is trunc(v) mod 2**bits (the rule at the top of
                             csrc/copy.hip); NaN, +-inf and anything else out of range are NOT admitted (NumPy leaves
                             them undefined);
    float -> bool            always (NaN is True, -0.0 is False);
    float -> float           always (NaNs compared by place, the sign of zero compared).
    `expected_cast(values, target)` is the expectation for admitted values: Python-integer arithmetic for float ->
    integer, NumPy's own cast for everything else.  tests/test_array_cases_yardstick.py holds it against NumPy.

float64 -> float16 witnesses, `f16_witnesses()`: float64 values one ulp off the midpoint of two neighbouring halves.  A
    conversion that goes through float32 first lands exactly on the midpoint and then rounds to even: wrong for about half.

Exactly summable arrays, `exact_array(dtype, shape, seed)`: integers below 2**10 in magnitude, or multiples of 2**-8 below
    2**10 (float16: below 4).  Values, squares and squared differences are then multiples of 2**-16 below 2**22 (integers:
    multiples of 1), 38 bits each: any partial sum of up to 2**15 float terms (EXACT_MAX_FLOAT_TERMS; 2**31 integer terms)
    fits in 53 bits, so a device reduction in float64 must EQUAL the reference whatever its order.

Layouts, `layouts(shape)`: (base shape, view) pairs; `view(base_array)` works on NumPy and on device arrays alike and
    gives an array of `shape` (the `None` layout: of `shape` with one more unit axis) that lies inside its base.
"""
import math
import warnings

import numpy as np

# the order of core._DTYPE_CODES
DTYPES = tuple(np.dtype(t) for t in (np.bool_, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64,
                                     np.uint64, np.float32, np.float64, np.float16))
MAX_NDIM = 8

_INT_EDGES = [-32769, -32768, -129, -128, -1, 0, 1, 127, 128, 255, 256, 32767, 32768, 65535, 65536,
              2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32,
              2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63]


def _quiet_cast(values, target):
    """NumPy's cast; only the overflow into a narrower float (a finite value beyond 65504 becomes inf in float16, float64's
    largest values become inf in float32) is silenced, by name"""
    with warnings.catch_warnings():
        if np.dtype(target) in (np.float16, np.float32):
            warnings.filterwarnings("ignore", message="overflow encountered in cast", category=RuntimeWarning)
        return np.asarray(values).astype(target)


def ladder(dtype):
    """1-D array of `dtype` with every edge value the dtype holds"""
    dtype = np.dtype(dtype)
    if dtype.kind == "b":
        return np.array([False, True])
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        cand = _INT_EDGES + [info.min, info.min + 1, info.max - 1, info.max]
        return np.array(sorted({v for v in cand if info.min <= v <= info.max}), dtype=dtype)
    info = np.finfo(dtype)
    one = dtype.type(1)
    vals = []
    for v in _INT_EDGES:                       # the integers this float type holds exactly
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f = dtype.type(v)
        if np.isfinite(f) and int(f) == v:
            vals.append(f)
    below_one = np.nextafter(one, dtype.type(0))
    pos = [dtype.type(0.5), below_one, dtype.type(1.5), dtype.type(2.5), info.smallest_subnormal,
           np.nextafter(info.tiny, dtype.type(0)), info.tiny, info.max, dtype.type(np.inf)]
    vals += [dtype.type(0.0), -dtype.type(0.0), dtype.type(np.nan)]
    vals += pos + [-p for p in pos]
    if dtype == np.float64:
        f32 = np.finfo(np.float32)
        half_ulp_beyond = float(f32.max) + 2.0 ** 103            # ulp(float32 max) = 2**104: the tie between max and 2**128
        sub = 2.0 ** -149                                        # float32's smallest subnormal
        extra = [half_ulp_beyond, np.nextafter(half_ulp_beyond, 0.0), np.nextafter(half_ulp_beyond, np.inf),
                 0.5 * sub, 1.5 * sub, 2.5 * sub, np.nextafter(0.5 * sub, 1.0), np.nextafter(1.5 * sub, 0.0),
                 (2 ** 23 - 0.5) * sub]                          # the last: between the largest subnormal and the smallest normal
        vals += extra + [-e for e in extra]
    return np.array(vals, dtype=dtype)


def f16_all():
    """every float16 bit pattern (NaN payloads included)"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _int_bits(target):
    return 8 * np.dtype(target).itemsize


def admitted(values, target):
    """boolean mask over `values`: which of them have a defined cast to `target` (the rule of the module docstring)"""
    values = np.asarray(values)
    target = np.dtype(target)
    if values.dtype.kind != "f" or target.kind in "fb":
        return np.ones(values.shape, bool)
    v = values.astype(np.float64)                                # exact: every float16 / float32 is a float64
    finite = np.isfinite(v)
    t = np.trunc(np.where(finite, v, 0.0))
    info = np.iinfo(target)
    fits = finite & (t >= float(info.min)) & (t < float(info.max + 1))      # both limits are powers of two (or 0): exact in float64
    if target.kind == "u":
        fits |= finite & (t < 0) & (np.abs(v) < 2.0 ** 63)
    return fits


def expected_cast(values, target):
    """the result demanded for admitted `values` cast to `target`"""
    values = np.asarray(values)
    target = np.dtype(target)
    if values.dtype.kind == "f" and target.kind in "iu":
        bits = _int_bits(target)
        unsigned = np.dtype("u{}".format(target.itemsize))
        wrapped = [int(x) % (1 << bits) for x in values.astype(np.float64).ravel().tolist()]      # int() truncates toward zero
        return np.array(wrapped, dtype=unsigned).view(target).reshape(values.shape)
    return _quiet_cast(values, target)


def rint_admitted(values, target):
    """mask for the round-half-even copy into an integer `target`: rint(v) fits (NumPy is the reference there)"""
    v = np.asarray(values).astype(np.float64)
    finite = np.isfinite(v)
    r = np.rint(np.where(finite, v, 0.0))
    info = np.iinfo(target)
    return finite & (r >= float(info.min)) & (r < float(info.max + 1))


def rint_ties(dtype):
    """ties of `dtype` (float32 / float64), small ones and the largest the type holds (ulp 0.5 just below 2**(p - 1))"""
    p = np.finfo(dtype).nmant + 1
    top = 2.0 ** (p - 2)
    pos = [0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 254.5, 255.5, 32766.5, 32767.5, 65534.5, 65535.5, top + 0.5, top + 1.5,
           2 * top - 0.5, 2 * top - 1.5]
    return np.array(pos + [-x for x in pos], dtype=dtype)


def same_floats(got, want):
    """float arrays agree: NaN in the same places, every other element bit for bit (so the sign of zero counts)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.dtype("u{}".format(got.dtype.itemsize))
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(np.ascontiguousarray(got).view(u)[~gn],
                                                          np.ascontiguousarray(want).view(u)[~wn]))


def same(got, want):
    """`same_floats` for floats, np.array_equal plus dtype / shape for everything else"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind == "f":
        return same_floats(got, want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(got, want))


# ---------------------------------------------------------------- float64 -> float16 witnesses
def f16_witnesses(seed=7, count=4096):
    """dict of float64 arrays: 'up' / 'down' (midpoint of a random positive half and its successor, moved one float64 ulp up /
    down), 'neg_up' / 'neg_down' (their negations), `count` values each; 'subnormal' (the same around midpoints inside
    float16's subnormal range) and 'top' (values around 65520, where float16 overflows)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(1, 0x7bff, size=count).astype(np.uint16)            # positive, finite, successor finite
    lo = bits.view(np.float16).astype(np.float64)
    hi = (bits + np.uint16(1)).view(np.float16).astype(np.float64)
    mid = 0.5 * (lo + hi)                                                    # exact: 12 significant bits
    up, down = np.nextafter(mid, np.inf), np.nextafter(mid, 0.0)
    k = np.arange(0, 1023, dtype=np.float64)
    smid = (k + 0.5) * 2.0 ** -24
    sub = np.concatenate([np.nextafter(smid, np.inf), np.nextafter(smid, 0.0), smid])
    top = np.array([65519.999, np.nextafter(65520.0, 0.0), 65520.0 - 2.0 ** -30, 65520.0, np.nextafter(65520.0, np.inf),
                    65504.0, 65504.0 + 2.0 ** -30, 65519.0])
    return {"up": up, "down": down, "neg_up": -up, "neg_down": -down,
            "subnormal": np.concatenate([sub, -sub]), "top": np.concatenate([top, -top])}


# ---------------------------------------------------------------- exactly summable arrays
EXACT_MAX_FLOAT_TERMS = 2 ** 15


def exact_array(dtype, shape, seed):
    """random array whose values, squares and squared differences (against another such array) sum exactly in float64"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "b":
        return rng.integers(0, 2, size=shape).astype(bool)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(max(info.min, -1023), min(info.max, 1023) + 1, size=shape).astype(dtype)
    kmax = 2 ** 10 if dtype == np.float16 else 2 ** 18                       # |x| < 4 (11 significant bits) or < 2**10
    return (rng.integers(-kmax + 1, kmax, size=shape) * 2.0 ** -8).astype(dtype)


def general_f64(n, seed):
    """float64 values without structure: signs mixed, magnitudes over six decades"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, size=n)


def sum_reference(op, a, b=None):
    """(correctly rounded sum, sum of magnitudes) of operation `op` of mi_sum: 0 values, 1 squared differences, 2 squares;
    the terms are formed in float64 as the kernel forms them, summed without error by math.fsum"""
    a = np.asarray(a).astype(np.float64).ravel()
    if op == 0:
        terms = a
    elif op == 2:
        terms = a * a
    else:
        d = a - np.asarray(b).astype(np.float64).ravel()
        terms = d * d
    return math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())


def sum_bound(n, magnitude):
    """|computed - exact| <= (n - 1) u sum|x_i| for a float64 summation in ANY order (Higham, Accuracy and Stability of
    Numerical Algorithms, eq. 4.4 to first order; the second-order term is below one part in 2**30 for n < 2**23)"""
    return (n - 1) * 2.0 ** -53 * magnitude * (1 + 2.0 ** -30)


# ---------------------------------------------------------------- layouts
class View:
    """index expression (and optional transposition) to apply to a base array"""

    def __init__(self, name, index=(), axes=None):
        self.name, self.index, self.axes = name, tuple(index), axes

    def __call__(self, base):
        v = base[self.index] if self.index else base[...]
        return v.transpose(*self.axes) if self.axes is not None else v

    def __repr__(self):
        return self.name


def layouts(shape):
    """(base shape, View) pairs: contiguous; [::2], [::-1] and [1:-1] on each axis; a transposition; a None axis"""
    shape = tuple(shape)
    nd = len(shape)
    full = slice(None)
    out = [(shape, View("contiguous"))]
    for ax in range(nd):
        def at(s, ax=ax):
            return (full,) * ax + (s,)
        n = shape[ax]
        out.append((shape[:ax] + (2 * n,) + shape[ax + 1:], View("step2@{}".format(ax), at(slice(None, None, 2)))))
        out.append((shape, View("reverse@{}".format(ax), at(slice(None, None, -1)))))
        out.append((shape[:ax] + (n + 2,) + shape[ax + 1:], View("inner@{}".format(ax), at(slice(1, -1)))))
    if nd >= 2:
        out.append((shape[::-1], View("transposed", (), tuple(range(nd - 1, -1, -1)))))
        rolled = tuple(range(1, nd)) + (0,)                                  # base axes order such that .transpose(rolled) gives `shape`
        base = [0] * nd
        for i, a in enumerate(rolled):
            base[a] = shape[i]
        out.append((tuple(base), View("rolled", (), rolled)))
    if nd < MAX_NDIM:
        for pos in sorted({0, nd // 2, nd}):
            out.append((shape, View("newaxis@{}".format(pos), (full,) * pos + (None,))))
    return out


# rank 0 and ranks 1 to 8 (8 = MI_MAX_NDIM); odd lengths and unit axes mixed in
RANK_SHAPES = ((), (7,), (5, 6), (3, 4, 5), (3, 2, 4, 3), (2, 3, 1, 4, 3), (2, 3, 2, 1, 3, 2), (2, 1, 3, 2, 2, 3, 2),
               (2, 3, 1, 2, 2, 1, 3, 2))


def view_extent(view_array, base_array):
    """(lowest, one past highest) byte offset the NumPy view touches, relative to its base, from shape and strides"""
    off = view_array.__array_interface__["data"][0] - base_array.__array_interface__["data"][0]
    lo = hi = off
    for n, st in zip(view_array.shape, view_array.strides):
        if n == 0:
            return off, off
        if st >= 0:
            hi += (n - 1) * st
        else:
            lo += (n - 1) * st
    return lo, hi + view_array.itemsize
