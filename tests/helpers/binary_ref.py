"""An independent reference of scipy.ndimage's binary morphology in plain NumPy, and the random draw of cases that the
yardstick (tests/test_binary_yardstick.py), the differential fuzzer (scripts/fuzz_vs_scipy.py --binary) and the route
tests (tests/test_gpu_binary_routes.py) share.

The reference (no SciPy inside):
  * truth is `x != 0` evaluated in the array's own dtype: NaN, +-inf and subnormals are foreground, -0.0 is background,
    an int16 256 / int32 65536 / int64 2**32 is foreground (nothing narrows to a byte first);
  * structure index k on an axis of extent s with origin o taps the voxel at offset k - s // 2 - o;
  * an erosion is true where every set tap sees a true voxel, a dilation mirrors the structure, negates the origin
    (one more subtracted on even extents) and is true where any tap sees a true voxel;
  * taps outside the array see `border_value`; voxels whose mask is zero keep the truth of the input;
  * iterations >= 1 repeat the step, iterations < 1 repeat it until nothing changes.
One step is built from a padded copy and one shifted AND / OR per set tap: the shapes are small, clarity beats speed.

Results are bool arrays; how a result reaches `output=` (array, dtype, aliasing the input) is the caller's side and is
judged by `judge` below against what SciPy does: only an ARRAY given as `output` changes the dtype (a dtype is ignored:
the result is bool), erosion / dilation / opening / closing / propagation return that array, hit_or_miss and fill_holes
return None.

float16: SciPy's C code has no float16 and raises; float16 -> float32 is exact and keeps every zero / nonzero
distinction, so the yardstick compares the reference on the float16 array with SciPy on its float32 copy.
"""
import numpy as np

FUNCS = ("erosion", "dilation", "opening", "closing", "hit_or_miss", "propagation", "fill_holes")
IN_DTYPES = ("bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "float16", "float32", "float64")
OUT_DTYPES = ("bool", "uint8", "int8", "int16", "int32", "int64", "float16", "float32", "float64")
LAST_AXIS = tuple(range(1, 41)) + (63, 64, 65, 96, 181, 260)
ITERATIONS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13)

# name -> (value, dtypes it is planted in): the values at which "nonzero is foreground" can go wrong
EDGE_VALUES = {
    "nan": (np.nan, ("float16", "float32", "float64")),
    "+inf": (np.inf, ("float16", "float32", "float64")),
    "-inf": (-np.inf, ("float16", "float32", "float64")),
    "f32 subnormal": (1e-45, ("float32",)),
    "f16 subnormal": (6e-8, ("float16",)),
    "f64 subnormal": (5e-324, ("float64",)),
    "int16 256": (256, ("int16", "uint16")),
    "int32 65536": (65536, ("int32", "uint32")),
    "int64 2**32": (2 ** 32, ("int64",)),
    "int64 65536": (65536, ("int64",)),
    "int32 256": (256, ("int32", "uint32", "int64")),
    "int8 -128": (-128, ("int8",)),
}


def edge_values_for(dtype):
    """[(name, value)] of the edge values that exist in `dtype`"""
    return [(k, v) for k, (v, dts) in EDGE_VALUES.items() if np.dtype(dtype).name in dts]


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def truth(x):
    """foreground of an array: nonzero in its own dtype"""
    x = np.asarray(x)
    return x != 0


def generate_binary_structure(rank, connectivity):
    if connectivity < 1:
        connectivity = 1
    if rank < 1:
        return np.array(True, dtype=bool)
    return np.abs(np.indices([3] * rank) - 1).sum(axis=0) <= connectivity


def _origins(origin, ndim):
    if np.ndim(origin) == 0:
        return [int(origin)] * ndim
    origin = [int(o) for o in origin]
    if len(origin) != ndim:
        raise RuntimeError("origin must have length equal to input rank")
    return origin


def tap_offsets(structure, origin):
    """offsets (tuples) at which the erosion by `structure` with `origin` reads its neighbours"""
    st = truth(structure)
    origin = _origins(origin, st.ndim)
    for s, o in zip(st.shape, origin):
        if s // 2 + o < 0 or s // 2 + o >= s:
            raise ValueError("invalid origin")
    return [tuple(int(k) - s // 2 - o for k, s, o in zip(idx, st.shape, origin)) for idx in np.argwhere(st)]


def mirrored(structure, origin):
    """the erosion-form structure and origin of the dilation by `structure` with `origin`"""
    st = truth(structure)
    origin = _origins(origin, st.ndim)
    st = st[(slice(None, None, -1),) * st.ndim]
    return st, [-o - (0 if s & 1 else 1) for o, s in zip(origin, st.shape)]


def dilation_offsets(structure, origin):
    return tap_offsets(*mirrored(structure, origin))


def step(cur, offsets, border_value, mask, dilate, negate=None):
    """one iteration on the bool array `cur`.  `negate` (mutation checks only): index of a tap whose offset is negated."""
    offsets = [tuple(-v for v in o) if i == negate else o for i, o in enumerate(offsets)]
    nd = cur.ndim
    pad = [max([abs(o[d]) for o in offsets] + [0]) for d in range(nd)]
    big = np.full([n + 2 * p for n, p in zip(cur.shape, pad)], bool(border_value), dtype=bool)
    big[tuple(slice(p, p + n) for n, p in zip(cur.shape, pad))] = cur
    res = np.zeros(cur.shape, bool) if dilate else np.ones(cur.shape, bool)
    for o in offsets:
        view = big[tuple(slice(p + d, p + d + n) for n, p, d in zip(cur.shape, pad, o))]
        if dilate:
            res |= view
        else:
            res &= view
    if mask is not None:
        res = np.where(mask, res, cur)
    return res


def _run(input, offsets, iterations, mask, border_value, dilate, truth_of=truth, negate=None, count=None):
    input = np.asarray(input)
    cur = truth_of(input)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != input.shape:
            raise RuntimeError("mask and input must have equal sizes")
        mask = truth(mask)
    if iterations >= 1:
        for _ in range(iterations):
            cur = step(cur, offsets, border_value, mask, dilate, negate)
        return cur
    limit = 4 * (sum(input.shape) + input.size) + 8
    for n in range(limit):
        nxt = step(cur, offsets, border_value, mask, dilate, negate)
        if np.array_equal(nxt, cur):
            if count is not None:
                count.append(n)         # iterations that changed something
            return cur
        cur = nxt
    raise RuntimeError("the iteration does not end (the operator is not monotone)")


def _structure(structure, ndim):
    if structure is None:
        return generate_binary_structure(ndim, 1)
    st = truth(structure)
    if st.ndim != ndim:
        raise RuntimeError("structure and input must have same dimensionality")
    if st.size < 1:
        raise RuntimeError("structure must not be empty")
    return st


def erosion(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, **dbg):
    input = np.asarray(input)
    st = _structure(structure, input.ndim)
    return _run(input, tap_offsets(st, origin), iterations, mask, border_value, False, **dbg)


def dilation(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, **dbg):
    input = np.asarray(input)
    st = _structure(structure, input.ndim)
    return _run(input, dilation_offsets(st, origin), iterations, mask, border_value, True, **dbg)


def opening(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, **dbg):
    tmp = erosion(input, structure, iterations, mask, border_value, origin, **dbg)
    dbg.pop("truth_of", None)
    return dilation(tmp, structure, iterations, mask, border_value, origin, **dbg)


def closing(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, **dbg):
    tmp = dilation(input, structure, iterations, mask, border_value, origin, **dbg)
    dbg.pop("truth_of", None)
    return erosion(tmp, structure, iterations, mask, border_value, origin, **dbg)


def hit_or_miss(input, structure1=None, structure2=None, origin1=0, origin2=None, **dbg):
    input = np.asarray(input)
    st1 = _structure(structure1, input.ndim)
    st2 = np.logical_not(st1) if structure2 is None else _structure(structure2, input.ndim)
    if origin2 is None:
        origin2 = origin1
    hit = erosion(input, st1, 1, None, 0, origin1, **dbg)
    # the miss: the erosion of the COMPLEMENT by structure2 (outside the array the complement is true)
    dbg2 = dict(dbg)
    t = dbg2.pop("truth_of", truth)
    miss = _run(np.logical_not(t(input)), tap_offsets(st2, origin2), 1, None, 1, False, **dbg2)
    return hit & miss


def propagation(input, structure=None, mask=None, border_value=0, origin=0, **dbg):
    return dilation(input, structure, -1, mask, border_value, origin, **dbg)


def fill_holes(input, structure=None, origin=0, **dbg):
    t = dbg.pop("truth_of", truth)
    background = np.logical_not(t(np.asarray(input)))
    reached = dilation(np.zeros(background.shape, bool), structure, -1, background, 1, origin, **dbg)
    return np.logical_not(reached)


def iterate_structure(structure, iterations, origin=None):
    st = truth(structure)
    if iterations < 2:
        return st.copy()
    ni = iterations - 1
    shape = [s + ni * (s - 1) for s in st.shape]
    out = np.zeros(shape, bool)
    out[tuple(slice(ni * (s // 2), ni * (s // 2) + s) for s in st.shape)] = st
    out = dilation(out, st, iterations=ni)
    if origin is None:
        return out
    return out, [iterations * o for o in _origins(origin, st.ndim)]


_REF = dict(erosion=erosion, dilation=dilation, opening=opening, closing=closing, hit_or_miss=hit_or_miss,
            propagation=propagation, fill_holes=fill_holes)
API = dict(erosion="binary_erosion", dilation="binary_dilation", opening="binary_opening", closing="binary_closing",
           hit_or_miss="binary_hit_or_miss", propagation="binary_propagation", fill_holes="binary_fill_holes")
RETURNS_NONE = ("hit_or_miss", "fill_holes")        # with an array as `output`
UNTIL_STABLE = ("propagation", "fill_holes")


# ---------------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------------
def _octahedron(r):
    return np.abs(np.indices((2 * r + 1,) * 3) - r).sum(axis=0) <= r


def _draw_shape(rng, nd):
    last = int(rng.choice(LAST_AXIS))
    if nd == 1:
        return (last,)
    hi = {2: 70, 3: 24}.get(nd, 7)
    rest = [1 if rng.random() < 0.1 else int(rng.integers(1, hi + 1)) for _ in range(nd - 1)]
    if nd >= 4:
        # the reference costs size x taps per iteration: ranks 4 and 5 keep the documented axis ranges, biased small
        rest = [min(v, int(rng.integers(1, 8))) for v in rest]
        while int(np.prod(rest)) * last > 30000:
            last = int(rng.choice(LAST_AXIS[:40]))
            rest[int(rng.integers(len(rest)))] = int(rng.integers(1, 4))
    return tuple(rest) + (last,)


def _draw_structure(rng, nd, shape):
    """(structure or None, name)"""
    u = rng.random()
    if u < 0.12:
        return None, "None"
    if u < 0.37:
        c = int(rng.integers(1, nd + 1))
        return generate_binary_structure(nd, c), "conn%d" % c
    if nd == 3 and u < 0.52:
        r = int(rng.choice([2, 2, 3]))
        st = np.ones((2 * r + 1,) * 3, bool) if rng.random() < 0.5 else _octahedron(r)
        name = ("cube" if st.all() else "octa") + str(r)
        if rng.random() < 0.4:          # one tap knocked out: no longer a Minkowski power of a 3 x 3 x 3 structure
            taps = np.argwhere(st)
            st[tuple(taps[int(rng.integers(len(taps)))])] = False
            name += "-1"
        return st, name
    top = 5 if nd <= 3 else 3
    ext = [int(rng.integers(1, top + 1)) for _ in range(nd)]
    if rng.random() < 0.15 and nd <= 3:
        ext[-1] = int(rng.choice([7, 9]))
    if rng.random() < 0.1:              # larger than the array on one axis
        d = int(rng.integers(nd))
        if shape[d] < top:
            ext[d] = min(top, shape[d] + 1 + int(rng.integers(0, 2)))
    st = rng.random(ext) > rng.choice([0.2, 0.5])
    if not st.any():
        st.flat[int(rng.integers(st.size))] = True
    if rng.random() < 0.3:              # without its centre
        st[tuple(s // 2 for s in ext)] = False
        if not st.any():
            st.flat[0] = True
    return st, "rand" + "x".join(map(str, ext))


def _draw_origin(rng, sshape):
    """any origin that is legal for the erosion; the mirrored dilation's -o (-1 on even extents) is then legal too"""
    if rng.random() < 0.45:
        return 0
    return [int(rng.integers(-(s // 2), (s - 1) // 2 + 1)) for s in sshape]


def _make_monotone(st, origin, dilate):
    """set the tap of `st` that reads the voxel itself, so that an until-stable run ends"""
    st = st.copy()
    o = _origins(origin, st.ndim)
    if dilate:
        idx = tuple(s - 1 - (s // 2 - oo - (0 if s & 1 else 1)) for s, oo in zip(st.shape, o))
    else:
        idx = tuple(s // 2 + oo for s, oo in zip(st.shape, o))
    st[idx] = True
    return st


def _draw_mask(rng, shape):
    u = rng.random()
    if u < 0.5:
        return None, "none"
    on = rng.random(shape) < rng.uniform(0.3, 0.95)
    if u < 0.75:
        return on, "bool"
    kind = str(rng.choice(["uint8", "int32", "float32"]))
    if kind == "uint8":
        m = (on * rng.choice([1, 2, 128, 255], size=shape)).astype(np.uint8)
    elif kind == "int32":
        m = (on * rng.choice([1, 256, 65536, -1], size=shape)).astype(np.int32)
    else:
        m = (on * rng.choice([1.0, 0.5, 1e-45], size=shape)).astype(np.float32)
        m[on & (rng.random(shape) < 0.3)] = np.nan
        m[~on & (rng.random(shape) < 0.5)] = -0.0
    return m, kind


def _draw_input(rng, shape, dtype):
    """(x, kind of density, names of the edge values planted)"""
    dt = np.dtype(dtype)
    u = rng.random()
    if u < 0.94:
        # an exact count, so that small arrays hold the drawn share too
        n = int(np.prod(shape))
        k = int(round(rng.uniform(0.15, 0.85) * n))
        lo, hi = -(-n // 10), (9 * n) // 10
        if lo <= hi:
            k = min(max(k, lo), hi)
        fg = np.zeros(n, bool)
        fg[rng.permutation(n)[:k]] = True
        fg = fg.reshape(shape)
        kind = "mixed"
    elif u < 0.96:
        fg, kind = np.zeros(shape, bool), "all-false"
    elif u < 0.98:
        fg, kind = np.ones(shape, bool), "all-true"
    else:
        fg, kind = np.zeros(shape, bool), "single"
        if fg.size:
            fg.flat[int(rng.integers(fg.size))] = True
    if dt.kind == "b":
        return fg.copy(), kind, []
    small = rng.integers(1, 4, size=shape)
    if dt.kind in "if" and dt.name != "int8":
        small = small * rng.choice([1, -1], size=shape)
    x = (fg * small).astype(dt)
    edges = edge_values_for(dt)
    planted = []
    if edges and fg.any():
        spots = np.flatnonzero(fg)
        for name, value in edges:
            if rng.random() < 0.6:
                sel = spots[rng.random(len(spots)) < 0.25]
                if len(sel) == 0:
                    sel = spots[:1]
                x.flat[sel] = np.array(value).astype(dt)
                planted.append(name)
    if dt.kind == "f":
        x[~fg & (rng.random(shape) < 0.5)] = -0.0
    assert np.array_equal(x != 0, fg)
    return x, kind, planted


def view_of(base, layout):
    """the case's array from its contiguous base (host or device array alike)"""
    if layout == "every-other":
        return base[..., ::2]
    if layout == "transposed":
        nd = base.ndim
        return base.transpose(*([nd - 1] + list(range(1, nd - 1)) + [0]))
    return base


def _base_for(x, layout, filler):
    if layout == "every-other":
        big = np.repeat(x, 2, axis=-1)
        big[..., 1::2] = filler
        return big
    if layout == "transposed":
        return np.ascontiguousarray(np.swapaxes(x, 0, -1))
    return np.ascontiguousarray(x)


def draw_case(rng):
    """One random call: dict(func, x_base, x_layout, kw, out_kind, out_dtype, out_layout, desc, ...).  `x_base` / `out_base`
    are contiguous host arrays, view_of() gives the arrays the call sees."""
    func = str(rng.choice(FUNCS))
    nd = int(rng.choice([1, 2, 2, 3, 3, 3, 4, 5]))
    shape = _draw_shape(rng, nd)
    dtype = str(rng.choice(IN_DTYPES))
    x, density_kind, planted = _draw_input(rng, shape, dtype)
    layout = str(rng.choice(["c", "c", "every-other", "transposed"])) if nd >= 2 else "c"
    filler = True if dtype == "bool" else 77
    x_base = _base_for(x, layout, filler)

    st, sname = _draw_structure(rng, nd, shape)
    sshape = (3,) * nd if st is None else st.shape
    kw = {}
    until_stable = func in UNTIL_STABLE
    if func == "hit_or_miss":
        st2, s2name = (None, "None") if rng.random() < 0.4 else _draw_structure(rng, nd, shape)
        kw = dict(structure1=st, structure2=st2, origin1=_draw_origin(rng, sshape),
                  origin2=_draw_origin(rng, sshape if st2 is None else st2.shape))
        if rng.random() < 0.3 and (st2 is None or st2.shape == tuple(sshape)):
            kw["origin2"] = None        # = origin1, which has to be legal for structure2 as well
        sname += "/" + s2name
    else:
        origin = _draw_origin(rng, sshape)
        if func in ("erosion", "dilation", "opening", "closing"):
            it = int(rng.choice(ITERATIONS)) if rng.random() < 0.8 else int(rng.choice([0, -1, -3]))
            if func in ("opening", "closing") and it < 1 and rng.random() < 0.5:
                it = int(rng.choice(ITERATIONS))
            kw["iterations"] = it
            until_stable = it < 1
        if until_stable:
            if st is None:
                origin = 0              # the default cross holds its centre
            elif func in ("opening", "closing"):
                st = _make_monotone(_make_monotone(st, origin, False), origin, True)
            else:
                st = _make_monotone(st, origin, func != "erosion")
        kw.update(structure=st, origin=origin)
        if func != "fill_holes":
            kw["border_value"] = int(rng.integers(0, 2))
            kw["mask"], mname = _draw_mask(rng, shape)
        if func == "fill_holes":
            mname = "none"
    u = rng.random()
    out_dtype = str(rng.choice(OUT_DTYPES))
    out_layout = None
    if u < 0.35:
        out_kind = "none"
    elif u < 0.5:
        out_kind = "dtype"
    else:
        out_kind = "array"
        out_layout = str(rng.choice(["c", "c", "strided", "input"]))
        if out_layout == "input":
            out_dtype = dtype
    case = dict(func=func, x_base=x_base, x_layout=layout, kw=kw, out_kind=out_kind, out_dtype=out_dtype,
                out_layout=out_layout, density_kind=density_kind, edges=planted, until_stable=until_stable,
                shape=shape, dtype=dtype)
    case["desc"] = (func, shape, dtype, layout, density_kind, sname,
                    {k: v for k, v in kw.items() if k in ("iterations", "border_value", "origin", "origin1", "origin2")},
                    "mask " + (mname if func != "hit_or_miss" else "none"),
                    "out " + out_kind + ("" if out_kind == "none" else ":" + out_dtype + (":" + out_layout if out_layout else "")),
                    planted)
    return case


def monotone_offsets(case):
    """the tap-offset lists of the case's until-stable steps (each must hold the zero offset)"""
    kw, nd = case["kw"], len(case["shape"])
    st = _structure(kw.get("structure"), nd)
    origin = kw.get("origin", 0)
    er, di = tap_offsets(st, origin), dilation_offsets(st, origin)
    return {"erosion": [er], "dilation": [di], "propagation": [di], "fill_holes": [di]}.get(case["func"], [er, di])


def reference(case, **dbg):
    """the reference's bool result of a drawn case"""
    x = view_of(case["x_base"], case["x_layout"])
    return _REF[case["func"]](x, **case["kw"], **dbg)


def _f32(a, on):
    return a.astype(np.float32) if on and isinstance(a, np.ndarray) and a.dtype == np.float16 else a


def call(mod, case, to_array=None, f16_as_f32=False):
    """Run the case through `mod` (scipy.ndimage or the device module; `to_array` puts a host array on the device).
    Returns (what the function returned, the array given as output or None, (the allocation that array lies in, the
    bytes between its samples before the call) or None), arrays as the module's own.  f16_as_f32: float16 arrays are handed over as float32 (SciPy has no float16)."""
    put = to_array or (lambda a: a)
    x = view_of(put(_f32(case["x_base"], f16_as_f32)), case["x_layout"])
    kw = dict(case["kw"])
    if kw.get("mask") is not None:
        kw["mask"] = put(kw["mask"])
    out = base = None
    if case["out_kind"] == "dtype":
        kw["output"] = np.dtype(case["out_dtype"])
        if f16_as_f32 and kw["output"] == np.float16:
            kw["output"] = np.dtype(np.float32)
    elif case["out_kind"] == "array":
        if case["out_layout"] == "input":
            out = x
        else:
            shape = tuple(case["shape"])
            if case["out_layout"] == "strided":
                shape = shape[:-1] + (2 * shape[-1],)
            host = _f32(np.full(shape, 77, dtype=np.uint8).view(np.bool_) if case["out_dtype"] == "bool" else
                        np.full(shape, 77, dtype=case["out_dtype"]), f16_as_f32)
            base = (put(host), host[..., 1::2].tobytes())
            out = base[0][..., ::2] if case["out_layout"] == "strided" else base[0]
        kw["output"] = out
    if mod.__name__.startswith("scipy"):
        return _scipy_brute_force(mod, case["func"], x, kw), out, base
    ret = getattr(mod, API[case["func"]])(x, **kw)
    return ret, out, base


def _scipy_brute_force(sndi, func, x, kw):
    """SciPy, always with brute_force=True: its coordinate-list path (iterations != 1 with the centre set) corrupts the heap
    for even-sized structures with an origin (scripts/fuzz_vs_scipy.py).  binary_propagation and binary_fill_holes do not
    take the flag, so their few lines are spelled out here around binary_dilation."""
    if func == "hit_or_miss":
        return sndi.binary_hit_or_miss(x, **kw)         # single iterations only
    if func == "propagation":
        return sndi.binary_dilation(x, kw.get("structure"), -1, kw.get("mask"), kw.get("output"), kw.get("border_value", 0),
                                    kw.get("origin", 0), brute_force=True)
    if func == "fill_holes":
        mask = np.logical_not(x)
        tmp = np.zeros(mask.shape, bool)
        output = kw.get("output")
        if isinstance(output, np.ndarray):
            sndi.binary_dilation(tmp, kw.get("structure"), -1, mask, output, 1, kw.get("origin", 0), brute_force=True)
            np.logical_not(output, output)
            return None
        output = sndi.binary_dilation(tmp, kw.get("structure"), -1, mask, None, 1, kw.get("origin", 0), brute_force=True)
        np.logical_not(output, output)
        return output
    return getattr(sndi, API[func])(x, brute_force=True, **kw)


def to_host(a):
    return a.get() if hasattr(a, "get") and not isinstance(a, np.ndarray) else np.asarray(a)


def judge(case, want, ret, out, base, f16_as_f32=False):
    """(ok, why): the outcome of call() against the reference's bool result `want`"""
    if case["out_kind"] != "array":
        if ret is None:
            return False, "returned None"
        got = to_host(ret)
        if got.dtype != np.bool_:
            return False, "dtype %s, not bool" % got.dtype
    else:
        if case["func"] in RETURNS_NONE:
            if ret is not None:
                return False, "returned %s, not None" % type(ret).__name__
        elif ret is not out:
            return False, "did not return the output array"
        got = to_host(out)
        odt = np.dtype(case["out_dtype"])
        if f16_as_f32 and odt == np.float16:
            odt = np.dtype(np.float32)
        if got.dtype != odt:
            return False, "output dtype changed to %s" % got.dtype
        if base is not None and case["out_layout"] == "strided" and to_host(base[0])[..., 1::2].tobytes() != base[1]:
            return False, "wrote between the samples of a strided output"
    if got.shape != want.shape:
        return False, "shape %s, not %s" % (got.shape, want.shape)
    exp = want.astype(got.dtype)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        return False, "%d of %d voxels differ, first at %s" % (len(bad), exp.size, tuple(int(v) for v in bad[0]))
    return True, ""
