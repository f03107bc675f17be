"""Host references of ndimage.label's reductions, their error bounds, and the random draw of `fuzz_vs_scipy.py --measure`.

Test infrastructure: used by scripts/fuzz_vs_scipy.py (`--measure`), tests/test_measure_yardstick.py and
tests/test_gpu_measure_routes.py, never by the package.

References.  Every region's statistics are accumulated on the host with `ufunc.at` / `bincount` over a per-voxel slot
(`region_slots`: which entry of `index` a voxel belongs to, matched by exact Python-integer equality, so uint64 labels
of 2**63 and up and negative index values compare as SciPy compares them).  Sums are accumulated in long double
(unit roundoff u_ref = 2**-64 on x86; 2**-53 where long double is double), extrema and counts exactly in the input
dtype, positions as the first voxel in C order at the extreme (the last NaN where the maximum is NaN).

Bounds (u = 2**-53, the device accumulates in float64; n_k = voxels of region k; S_k = sum of |v| over it):
  * sum.  The device reduces a wave's run of equal slots by shuffles (depth 6), adds each run's total into an LDS or a
    global accumulator, and flushes each workgroup's LDS accumulator into the global one.  An addend's chain of
    additions is at most 6 + (run heads of its region before it in its workgroup) + (workgroups flushing the region):
    together at most 6 + n_k + 1.  One more rounding converts an int64 / uint64 value of 2**53 or more to double.  So
        |got - ref| <= k u S_k + n_k u_ref S_k,   k = n_k + 8,
    the second term being the reference's own error (sequential long double additions).
  * mean = sum / n_k:  bound(sum) / n_k + u |mean|.
  * variance (two passes: mean m', then sum of (v - m')^2, divided by n_k).  With D_k = sum (v - m)^2 and the mean's
    error e_m = bound(mean): sum (v - m')^2 = D_k + n_k (m' - m)^2 exactly, each (v - m')^2 carries 3 roundings, the
    sum k more, the division one:
        |got - ref| <= ((k + 4) u + (n_k + 3) u_ref) D_k / n_k + (e_m^2 + C_k) (1 + 2 k u),
    where C_k = sum (2 |v - m| c_v + c_v^2) / n_k and c_v = u |v| is the rounding of an int64 / uint64 value to double
    (0 for every other dtype).
    It scales with the spread, not with the values: 1e4 + noise is held to the same bound as zero-mean data.
  * standard deviation: |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= bv / max(sqrt(var), sqrt(bv)), plus
    u |std| for the last rounding.
  * center of mass, per axis c = T / S with T = sum v x, S = sum v:  with e_T = (k + 2) u sum |v x| (the product and
    the conversion of v add one rounding each) and e_S = bound(sum),  |got - ref| <= (e_T + |c| e_S) / (|S| - e_S) + u |c|  (infinite when
    |S| <= e_S: a centre of a region of zero mass is not defined and is not judged).

Exact comparisons.  Extrema, positions, counts and histograms are exact.  When the data are integer-valued and every
partial sum stays below 2**53 (sum |v| and sum |v x| < 2**53), float64 sums are exact whatever the order of the
additions; sum, mean and center_of_mass are then compared bit for bit against the correctly rounded quotient
float64(T) / float64(S): a dropped or double-counted voxel shows as a difference of one whole value.
"""
import numpy as np

U = 2.0 ** -53
U_REF = float(np.finfo(np.longdouble).eps) / 2
EXACT_LIMIT = 2.0 ** 53

FUNCS = ["sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum", "minimum_position",
         "maximum_position", "extrema", "center_of_mass", "histogram"]


# ---------------------------------------------------------------------------------------------------------------------
# regions
# ---------------------------------------------------------------------------------------------------------------------
def index_form(index):
    """'all' (no labels), 'none', 'scalar' or 'seq' -- how SciPy shapes the answer"""
    if index is None:
        return "none"
    return "scalar" if np.ndim(index) == 0 else "seq"


def region_slots(labels, index, size):
    """(slot of every voxel, -1 outside every region; rows: the slot of each index entry; number of slots).
    Slot j is the first index entry of its value; entries of equal value share it."""
    if labels is None:
        return np.zeros(size, np.int64), np.zeros(1, np.int64), 1
    lab = np.asarray(labels).ravel()
    if index is None:
        return np.where(lab > 0, 0, -1).astype(np.int64), np.zeros(1, np.int64), 1
    # Python integers as given: NumPy makes a list that mixes small ones with ones of 2**63 and up float64
    vals = np.asarray(index, dtype=object).ravel().tolist() if not isinstance(index, np.ndarray) else index.ravel().tolist()
    first = {}
    rows = np.empty(len(vals), np.int64)
    for k, v in enumerate(vals):
        rows[k] = first.setdefault(int(v), k)
    u, inv = np.unique(lab, return_inverse=True)
    lut = np.array([first.get(int(v), -1) for v in u.tolist()], np.int64)
    return lut[inv.ravel()] if u.size else np.zeros(0, np.int64), rows, max(len(vals), 1)


class Ref:
    """float64-or-better statistics per slot of one (input, labels, index)"""

    def __init__(self, x, labels, index):
        x = np.asarray(x)
        self.x, self.shape, self.form = x, x.shape, ("all" if labels is None else index_form(index))
        slot, self.rows, K = region_slots(labels, index, x.size)
        self.K = K
        sel = np.flatnonzero(slot >= 0)
        self.sel, self.s = sel, slot[sel]
        v = x.ravel()[sel]
        self.v = v
        self.vl = v.astype(np.longdouble)
        self.n = np.bincount(self.s, minlength=K)

    # -- sums
    def _acc(self, w):
        out = np.zeros(self.K, np.longdouble)
        np.add.at(out, self.s, w)
        return out

    def integer_valued(self):
        v = self.v
        if v.dtype.kind in "biu":
            return True
        f = v[np.isfinite(v)]
        return f.size == v.size and np.array_equal(f, np.floor(f))

    def sums(self):
        S = self._acc(self.vl)
        A = self._acc(np.abs(self.vl))
        k = self.n + 8.0
        exact = self.integer_valued() and bool(np.all(A < EXACT_LIMIT))
        bound = np.zeros(self.K) if exact else (k * U + self.n * U_REF) * A.astype(np.float64)
        return S.astype(np.float64), bound, exact, S, A

    def mean(self):
        s64, bs, exact, S, _ = self.sums()
        with np.errstate(all="ignore"):
            m = s64 / self.n if exact else (S / self.n).astype(np.float64)
            b = np.zeros(self.K) if exact else bs / self.n + U * np.abs(m)
        return m, b, exact

    def variance(self):
        m, bm, _ = self.mean()
        ml = (self._acc(self.vl) / self.n)
        with np.errstate(all="ignore"):
            d = self.vl - ml[self.s]
            D = self._acc(d * d)
            var = (D / self.n).astype(np.float64)
            k = self.n + 8.0
            # an int64 / uint64 value of 2**53 or more is rounded to double before it is centred: |dv| <= u |v|
            cv = (np.abs(self.vl) * U).astype(np.float64) if self.v.dtype.itemsize == 8 and self.v.dtype.kind in "iu" \
                else np.zeros(self.v.size)
            conv = (self._acc(2 * np.abs(d).astype(np.float64) * cv + cv * cv) / self.n).astype(np.float64)
            b = ((k + 4) * U + (self.n + 3) * U_REF) * var + bm ** 2 * (1 + 2 * k * U) + conv * (1 + 2 * k * U)
        return var, b

    def std(self):
        var, bv = self.variance()
        with np.errstate(all="ignore"):
            sd = np.sqrt(var)
            b = bv / np.maximum(np.sqrt(var), np.sqrt(bv)) + U * sd
        return sd, b

    def com(self):
        s64, bs, exact_s, S, A = self.sums()
        coords = np.unravel_index(self.sel, self.shape) if self.shape else ()
        ref, bnd = [], []
        k = self.n + 8.0
        for c in coords:
            t = self.vl * c.astype(np.longdouble)
            T, TA = self._acc(t), self._acc(np.abs(t))
            exact = exact_s and bool(np.all(TA < EXACT_LIMIT))
            with np.errstate(all="ignore"):
                r = T.astype(np.float64) / s64 if exact else (T / S).astype(np.float64)
                eT = (k + 2) * U * TA.astype(np.float64) + self.n * U_REF * TA.astype(np.float64)
                den = np.abs(S.astype(np.float64)) - bs
                b = np.zeros(self.K) if exact else np.where(den > 0, (eT + np.abs(r) * bs) / den, np.inf) + U * np.abs(r)
            ref.append(r)
            bnd.append(b)
        if not coords:
            return np.zeros((self.K, 0)), np.zeros((self.K, 0))
        return np.stack(ref, 1), np.stack(bnd, 1)

    # -- exact statistics
    def extrema(self, nan_min_propagates=False):
        """(min, max, min position, max position, present); positions are linear C-order indices"""
        K, v, s = self.K, self.v, self.s
        present = self.n > 0
        dt = v.dtype
        if dt.kind == "f":
            w = v.astype(np.float64)
            mn = np.full(K, np.nan)
            np.fmin.at(mn, s, w)                         # NaN skipped unless nothing else
            mx = np.full(K, -np.inf)
            np.maximum.at(mx, s, w)                      # NaN wins
            hasnan = np.zeros(K, bool)
            hasnan[s[np.isnan(w)]] = True
            mx[hasnan] = np.nan
            mx[~present] = np.nan
        else:
            w = v.astype(np.uint64 if dt == np.uint64 else np.int64)
            info = np.iinfo(w.dtype)
            mn = np.full(K, info.max, w.dtype)
            mx = np.full(K, info.min, w.dtype)
            np.minimum.at(mn, s, w)
            np.maximum.at(mx, s, w)
        # positions: the first voxel at the extreme (== : -0.0 and +0.0 are one value); the last NaN when the maximum
        # is NaN; the first NaN when a region holds nothing but NaN (its minimum)
        pmn = np.zeros(K, np.int64)
        pmx = np.zeros(K, np.int64)
        if v.size:
            if dt.kind == "f":
                kmin = np.where(np.isnan(mn[s]), np.isnan(w), w == mn[s])
                kmax = np.where(np.isnan(mx[s]), np.isnan(w), w == mx[s])
            else:
                kmin, kmax = w == mn[s], w == mx[s]
            _first(pmn, s[kmin], self.sel[kmin])
            _first(pmx, s[kmax], self.sel[kmax])
            if dt.kind == "f":
                last_nan = np.isnan(mx[s]) & np.isnan(w)
                tmp = np.full(K, -1, np.int64)
                np.maximum.at(tmp, s[last_nan], self.sel[last_nan])
                pmx = np.where(tmp >= 0, tmp, pmx)
        if dt.kind == "f" and nan_min_propagates:
            mn[hasnan] = np.nan                          # SciPy's vals.min() with no index or a scalar one
        zero = np.zeros(K, mn.dtype)
        mn = np.where(present, mn, zero)
        mx = np.where(present, mx, zero)
        return mn, mx, np.where(present, pmn, 0), np.where(present, pmx, 0), present

    def histogram(self, edges):
        bins = len(edges) - 1
        w = self.v.astype(np.float64)
        b = np.searchsorted(edges, w, side="right") - 1
        b[w == edges[-1]] = bins - 1
        ok = (w >= edges[0]) & (w <= edges[-1])
        h = np.bincount(self.s[ok] * bins + b[ok], minlength=self.K * bins).reshape(self.K, bins)
        return h, self.n > 0


def _first(out, slots, pos):
    """out[slot] = smallest pos of that slot (slots with no entry keep their value)"""
    if slots.size:
        tmp = np.full(out.size, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(tmp, slots, pos)
        hit = tmp != np.iinfo(np.int64).max
        out[hit] = tmp[hit]


def ratio(got, ref, bound):
    """max |got - ref| / bound over the entries; non-finite references must match exactly (NaN with NaN, inf with the
    same inf); entries with an infinite bound are not judged"""
    ref = np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape).ravel()
    got, ref = np.asarray(got, np.float64).ravel(), ref.ravel()
    if got.shape != ref.shape:
        return float("inf")
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin], equal_nan=True):
        return float("inf")
    g, r, b = got[fin], ref[fin], bound[fin]
    err = np.abs(g - r)
    if np.any(~np.isfinite(err) & np.isfinite(b)):
        return float("inf")
    judged = np.isfinite(b)
    err, b = err[judged], b[judged]
    if err.size == 0:
        return 0.0
    if np.any((b == 0) & (err != 0)):
        return float("inf")
    with np.errstate(all="ignore"):
        q = np.where(b > 0, err / np.where(b > 0, b, 1), 0.0)
    return float(q.max())


# ---------------------------------------------------------------------------------------------------------------------
# the --measure draw: reductions
# ---------------------------------------------------------------------------------------------------------------------
IN_DTYPES = ["bool", "uint8", "int16", "uint16", "int32", "int64", "uint64", "float16", "float32", "float64"]
LAB_DTYPES = ["bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"]
LUT_SLACK = 1 << 16          # measurements._LUT_SLACK: a lookup table when imax - imin < 4 K + LUT_SLACK


def _values(rng, shape, dtype):
    """input on the value ranges of tests/helpers/value_ranges.py, cast to `dtype`; floats carry +-0, +-inf, NaN"""
    from helpers import value_ranges as vr
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    flat = (max(n // 64, 1), 64) if n >= 64 else (1, max(n, 1))     # the generators draw 2-D / 3-D volumes
    seed = int(rng.integers(1 << 30))
    take = lambda a: np.asarray(a).ravel()[:n].reshape(shape) if np.asarray(a).size >= n else \
        np.resize(np.asarray(a).ravel(), n).reshape(shape)
    gen = str(rng.choice(["mr", "ct", "1e4", "extremes", "small"]))
    if dtype == np.bool_:
        return rng.random(shape) < rng.random(), gen
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        if gen == "extremes" and dtype.itemsize == 2:
            a = vr.int_extremes(flat, dtype, seed)
        elif gen == "extremes":
            a = rng.integers(int(info.min), int(info.max), size=flat, dtype=dtype, endpoint=True)
            a.ravel()[rng.random(a.size) < 0.05] = info.max
            a.ravel()[rng.random(a.size) < 0.05] = info.min
        elif gen == "ct" and info.min < 0:
            a = vr.ct_hu(flat, seed).astype(dtype)
        elif gen == "small":
            a = rng.integers(max(int(info.min), -3), min(int(info.max), 3), size=flat, endpoint=True)
        else:
            a = vr.mr_u12(flat, seed)
            a = (a >> 4) if info.max < 4095 else a
        return take(np.asarray(a).astype(dtype)), gen
    if gen == "ct":
        a = vr.ct_hu(flat, seed, dtype=np.float32)
    elif gen == "1e4":
        a = vr.offset_1e4(flat, seed)
    elif gen == "extremes":
        a = rng.standard_normal(flat) * 10.0 ** rng.integers(-3, 4, size=flat)
    elif gen == "small":
        a = rng.integers(-3, 4, size=flat).astype(np.float64)
    else:
        a = vr.mr_u12(flat, seed, dtype=np.float32)
    a = take(a).astype(dtype)
    if dtype == np.float64 and gen in ("mr", "ct") and rng.random() < 0.5:
        a = a + rng.standard_normal(shape) * 0.25           # real-valued float64 data
    if rng.random() < 0.35:
        specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -0.0], dtype)
        w = rng.choice(specials.size, size=n, p=[0.3, 0.3, 0.1, 0.1, 0.1, 0.1])
        m = rng.random(n) < float(rng.choice([0.001, 0.02, 0.2]))
        a.ravel()[m] = specials[w[m]]
    elif rng.random() < 0.3:
        a.ravel()[rng.random(n) < 0.3] = -0.0
    return a, gen


def _runs(rng, n, values):
    """a label stream of runs of equal values: lengths 1, 2, 63, 64, 65, 255 .. 257 or random"""
    out = np.empty(n, np.int64)
    i = 0
    choices = np.array([1, 1, 2, 3, 63, 64, 65, 127, 128, 255, 256, 257])
    while i < n:
        L = int(rng.choice(choices)) if rng.random() < 0.7 else int(rng.integers(1, 400))
        out[i:i + L] = values[int(rng.integers(values.size))]
        i += L
    return out


def draw_reduction(rng):
    """one random reduction case: dict(func, x, labels, index, index_kind, kw, note)"""
    func = str(rng.choice(FUNCS))
    nd = int(rng.choice([1, 2, 2, 3, 3, 3]))
    big = rng.random() < 0.25
    if nd == 1:
        shape = (int(rng.choice([1, 63, 64, 65, 255, 256, 257, 4096, rng.integers(1, 3000)])) if not big
                 else int(rng.integers(60000, 150000)),)
    elif nd == 2:
        shape = (int(rng.integers(1, 70 if not big else 400)), int(rng.choice([1, 63, 64, 65, 256, rng.integers(2, 300)])))
    else:
        shape = tuple(int(rng.integers(1, 20 if not big else 48)) for _ in range(2)) + \
            (int(rng.choice([1, 7, 8, 9, 31, 32, 33, 64, 65, rng.integers(2, 80)])),)
    n = int(np.prod(shape))
    x, gen = _values(rng, shape, str(rng.choice(IN_DTYPES)))
    kind = str(rng.choice(["none_labels", "none", "scalar", "list", "host", "device", "list", "host", "device"]))
    if kind == "none_labels":
        return dict(func=func, x=x, labels=None, index=None, index_kind="none", kw=_hist_kw(rng, x, func), gen=gen)
    ldt = np.dtype(str(rng.choice(LAB_DTYPES)))
    # slot counts: few, around the LDS limit (1024) and around center_of_mass's 2048 / ndim
    K = int(rng.choice([1, 2, 5, 17, 1023, 1024, 1025, 2048 // nd - 1, 2048 // nd, 2048 // nd + 1, 2048 // nd + 2]))
    if ldt == np.bool_:
        vals = np.array([0, 1])
    else:
        info = np.iinfo(ldt)
        K = min(K, int(info.max) - max(int(info.min), -50) - 4)
        lo = int(rng.integers(max(int(info.min), -50), min(int(info.max) - K - 3, 200) + 1))
        vals = lo + np.arange(K + 3, dtype=np.int64)
        if ldt.itemsize >= 4 and rng.random() < 0.4:
            # a range on the other side of the lookup-table / search threshold: one value far away
            wide = 4 * K + LUT_SLACK + int(rng.integers(-2, 3))
            far = int(vals[-1]) + wide if int(vals[-1]) + wide <= int(info.max) else None
            if far is not None:
                vals = np.append(vals, far)
        if ldt == np.uint64 and rng.random() < 0.5:
            span = int(vals[-1]) - lo
            base = (1 << 63) - int(rng.integers(0, 3)) if rng.random() < 0.5 else 2 ** 64 - 1 - span
            vals = [int(v) - lo + base for v in vals]             # labels of 2**63 and up: negative as int64
    vals = [int(v) for v in vals]
    varr = np.array(vals, dtype=np.uint64 if max(vals) >= 1 << 63 else np.int64)
    labv = varr[_runs(rng, n, np.arange(len(vals)))].astype(ldt).reshape(shape)
    if kind == "none":
        index = None
    else:
        pick = [int(vals[i]) for i in rng.integers(0, len(vals), size=K)]
        if K > 1 and rng.random() < 0.5:
            pick[int(rng.integers(K))] = pick[0]                  # a duplicate
        extra = [0]
        if not (ldt == np.uint64 and max(pick) >= 1 << 63):
            extra += [-1, -int(rng.integers(2, 300))]             # negative: no unsigned label carries it
        if ldt != np.bool_:
            extra.append(int(max(pick)) + 1 if max(pick) + 1 < int(np.iinfo(ldt).max) else int(min(pick)) - 1)
        pick += [e for e in extra if rng.random() < 0.5]
        pick = [int(p) for p in rng.permutation(np.array(pick, dtype=object))]
        if min(pick) < 0 and max(pick) >= 1 << 63:
            pick = [p for p in pick if p >= 0]                     # NumPy would make such a list float64
        if kind == "scalar":
            index = pick[0] if rng.random() < 0.5 else np.asarray(pick[0]).astype(np.uint64 if pick[0] >= 1 << 63 else np.int64)[()]
        elif kind == "list":
            index = pick
        else:
            index = np.array(pick, dtype=np.uint64 if max(pick) >= 1 << 63 else np.int64)
            if kind == "host" and rng.random() < 0.3 and ldt != np.bool_ and min(pick) >= np.iinfo(ldt).min and \
                    max(pick) <= np.iinfo(ldt).max:
                index = index.astype(ldt)                          # an index of the labels' dtype
            if kind == "device" and index.dtype != np.int64:
                kind = "host"                                      # device index arrays are int64
    return dict(func=func, x=x, labels=labv, index=index, index_kind=kind, kw=_hist_kw(rng, x, func), gen=gen)


def _hist_kw(rng, x, func):
    if func != "histogram":
        return {}
    f = x[np.isfinite(x)] if x.dtype.kind == "f" else x
    lo = float(f.min()) if f.size else 0.0
    hi = float(f.max()) if f.size else 1.0
    mn = float(rng.choice([lo, np.floor(lo), lo - 1, 0.0, -1024.0]))
    mx = float(rng.choice([hi, np.ceil(hi), hi + 1, 3071.0, mn]))
    if rng.random() < 0.1:
        mn, mx = mx + 1, mn                                        # min > max: SciPy raises
    return dict(min=mn, max=mx, bins=int(rng.choice([1, 2, 7, 10, 64, 255, 256, 1000])))


def call(mod, case, asarray=None):
    """run the case's function on `mod` (scipy.ndimage, or the package with `asarray` moving arrays to the device)"""
    x, lab, idx = case["x"], case["labels"], case["index"]
    if asarray is not None:
        x = asarray(x)
        lab = None if lab is None else asarray(lab)
        if case["index_kind"] == "device":
            idx = asarray(np.asarray(idx, np.int64))
    f = getattr(mod, case["func"])
    kw = case["kw"]
    if case["func"] == "histogram":
        return f(x, kw["min"], kw["max"], kw["bins"], lab, idx)
    return f(x, lab, idx)


def _host(r):
    return r.get() if hasattr(r, "get") else r


def _struct(r, exempt_dtype=False):
    """the result's type, shape and dtype (positions and centres: tuples of Python or NumPy numbers)"""
    if r is None:
        return None
    if isinstance(r, list):
        return ("list", len(r), [_struct(e, exempt_dtype) for e in r])
    if isinstance(r, tuple):
        if all(isinstance(e, (int, float, np.number)) for e in r):
            return ("numbers", len(r))          # a position or a centre: Python or NumPy numbers
        return ("tuple", len(r), [_struct(e, exempt_dtype) for e in r])
    if hasattr(r, "get") or isinstance(r, (np.ndarray, np.generic)):
        return ("array", tuple(r.shape), None if exempt_dtype else np.dtype(r.dtype).name)
    return ("number",)


def _pos(p, shape):
    return tuple(int(c) for c in np.unravel_index(int(p), shape)) if len(shape) else ()


def _exact(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return bool(np.array_equal(a.astype(np.float64), b.astype(np.float64), equal_nan=True))
    return bool(np.array_equal(a, b))


def scipy_exact(case):
    """False where SciPy 1.15 itself is unreliable and only the host reference judges the values: uint64 labels of 2**53
    or more with a sequence index (np.searchsorted matches them through float64, so neighbouring labels merge)"""
    lab = case["labels"]
    return not (lab is not None and lab.dtype == np.uint64 and lab.size and int(lab.max()) >= 1 << 53 and
                index_form(case["index"]) == "seq")


def judge(case, got, want=None, want_exc=None, got_exc=None, check_struct=True):
    """(ok, worst bound ratio, reason) for the result `got` of `case` (device results or SciPy's own); `want` /
    `want_exc`: SciPy's result or exception on the host copy"""
    func, x, lab, idx = case["func"], case["x"], case["labels"], case["index"]
    form = "all" if lab is None else index_form(idx)
    # SciPy 1.15 defects, judged against the host reference alone: IndexError for a NaN position with no index or a
    # scalar one (positions[vals == vals.min()][0]), and for a sequence index over labels holding their dtype's
    # largest value (labels.max() + 1 wraps in the labels' dtype)
    scipy_defect = isinstance(want_exc, IndexError) and func in ("minimum", "maximum", "minimum_position",
                                                                 "maximum_position", "extrema")
    if want_exc is not None and not scipy_defect:
        if got_exc is None:
            return False, float("inf"), "SciPy raised %s, the device did not" % type(want_exc).__name__
        if type(got_exc) is not type(want_exc):
            return False, float("inf"), "raised %s, SciPy %s" % (type(got_exc).__name__, type(want_exc).__name__)
        return True, 0.0, "both raised %s" % type(want_exc).__name__
    if got_exc is not None:
        return False, float("inf"), "raised %s: %s" % (type(got_exc).__name__, str(got_exc)[:120])
    if want is not None and not scipy_exact(case):
        want = want if check_struct else None
        check_values_with_scipy = False
    else:
        check_values_with_scipy = True
    if check_struct and want is not None:
        exempt = func == "sum_labels" and form != "seq"         # SciPy: input.sum() in the input's dtype
        if _struct(got, exempt) != _struct(want, exempt):
            return False, float("inf"), "result structure %s, SciPy %s" % (_struct(got, exempt), _struct(want, exempt))
    ref = Ref(x, lab, idx)
    rows = ref.rows
    one = form != "seq"

    def vals(r):
        return np.asarray(_host(r)).reshape(-1)

    if func in ("sum_labels", "mean", "variance", "standard_deviation"):
        r, b = {"sum_labels": lambda: ref.sums()[:2], "mean": lambda: ref.mean()[:2], "variance": ref.variance,
                "standard_deviation": ref.std}[func]()
        q = ratio(vals(got), r[rows], b[rows])
        return q <= 1.0, q, "bound ratio %.3g" % q
    if func == "center_of_mass":
        r, b = ref.com()
        g = np.asarray([got] if one else got, np.float64).reshape(len(rows), len(x.shape))
        q = ratio(g, r[rows], b[rows])
        return q <= 1.0, q, "bound ratio %.3g" % q
    if func == "histogram":
        kw = case["kw"]
        if lab is not None and idx is not None and lab.dtype == np.uint64:
            # SciPy's labeled_comprehension compares labels with index.astype(labels.dtype): -1 names 2**64 - 1
            ref = Ref(x, lab, [int(v) % (1 << 64) for v in np.asarray(idx, dtype=object).ravel().tolist()])
            rows = ref.rows
        edges = np.linspace(kw["min"], kw["max"], kw["bins"] + 1)
        h, present = ref.histogram(edges)
        rs = [h[k] if (present[k] or not (lab is not None and idx is not None)) else None for k in rows]
        gs = [got] if one else got
        for g, r in zip(gs, rs):
            if (g is None) != (r is None) or (r is not None and not _exact(_host(g), r)):
                return False, float("inf"), "histogram counts differ"
        if want is not None and check_values_with_scipy:
            ws = [want] if one else want
            for g, w in zip(gs, ws):
                if (g is None) != (w is None) or (w is not None and not _exact(_host(g), w)):
                    return False, float("inf"), "histogram differs from SciPy"
        return True, 0.0, "exact"
    mn, mx, pmn, pmx, _ = ref.extrema(nan_min_propagates=one)
    parts = {"minimum": [("v", mn)], "maximum": [("v", mx)], "minimum_position": [("p", pmn)],
             "maximum_position": [("p", pmx)], "extrema": [("v", mn), ("v", mx), ("p", pmn), ("p", pmx)]}[func]
    gparts = list(got) if func == "extrema" else [got]
    wparts = (list(want) if func == "extrema" else [want]) if want is not None and not scipy_defect and \
        check_values_with_scipy else None
    for j, ((what, r), g) in enumerate(zip(parts, gparts)):
        if what == "v":
            if not _exact(vals(g), r[rows]):
                return False, float("inf"), "extreme differs from the host reference"
            if wparts is not None and not _exact(vals(g), vals(wparts[j])):
                return False, float("inf"), "extreme differs from SciPy"
        else:
            rp = [_pos(p, x.shape) for p in r[rows]]
            gp = [g] if one else g
            if [tuple(int(c) for c in t) for t in gp] != rp:
                return False, float("inf"), "position differs from the first occurrence: %s vs %s" % (gp[:4], rp[:4])
            if wparts is not None and one:                         # SciPy's choice among ties is defined here
                if tuple(int(c) for c in g) != tuple(int(c) for c in wparts[j]):
                    return False, float("inf"), "position differs from SciPy"
    return True, 0.0, "exact"
