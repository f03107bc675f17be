"""An independent reference of scipy.ndimage's grey morphology in plain NumPy, and the random draw of cases that the
yardstick (tests/test_grey_yardstick.py) and the device fuzz (tests/test_gpu_grey_fuzz.py) share.

The reference (no SciPy inside) restates SciPy's arithmetic, which csrc/minmax.hip commits to bit for bit:
  * a window with holes or with a structure is one n-D pass: the array is padded once (the fill value converted to the INPUT
    dtype), the set taps are walked in C order, tap 0 is evaluated in double (`double(window) + s0`), every later tap has its
    structure value truncated to the input dtype and added IN that dtype (unsigned types wrap) before it is widened, the
    running extremum is updated with a strict `<` / `>` on doubles and stored with a C cast into the output dtype;
  * `s` is the structure for a maximum and its negative for a minimum;
  * double -> integer dtype T is double -> int64 -> T: truncation toward zero, then wrap-around;
  * an all-ones window without a structure (`size`, or a footprint of ones) is what SciPy makes of it: one 1-D pass per axis
    whose extent is above 1, on a double line buffer (the fill value stays a double), each pass stored into the OUTPUT dtype
    and read back by the next.  Axes of extent 1 are skipped, their origin unchecked;
  * grey_dilation mirrors footprint and structure on every axis and uses origin -o - (1 if the extent is even else 0);
  * the composites are compositions of these two and NumPy arithmetic in the input dtype (integers wrap; the top-hats of
    bool images are an xor).
One pass is vectorised over voxels with a Python loop over taps: the shapes are small, clarity beats speed.

Left out of the draw by construction, because SciPy's own result rests there on a C conversion the language leaves undefined
(or, the last one, because SciPy raises): bool or uint64 input with a structure, 64-bit values beyond 2^53 (the draw stays
within +-2^40), int32 values within 200 of the ends of the range with a structure (tap 0, a double, would leave the range:
the one store SciPy's compiler does not make through int64; int8 / int16 and the unsigned types do wrap in the draw), a
negative fill value for an unsigned dtype (negative double -> unsigned), and bool input to morphological_gradient / morphological_laplace
(NumPy refuses bool - bool).  DESIGN.md, section 2, records the same list.

An illegal origin makes `reference` return a ValueError instance instead of an array; `judge` then wants the call to have
raised ValueError as well."""
import numpy as np

SIMPLE = ("grey_erosion", "grey_dilation", "minimum_filter", "maximum_filter")
COMPOSITES = ("grey_opening", "grey_closing", "morphological_gradient", "morphological_laplace", "white_tophat", "black_tophat")
FUNCS = SIMPLE + COMPOSITES
MODES = ("reflect", "grid-mirror", "mirror", "nearest", "wrap", "grid-wrap", "constant", "grid-constant")
PAD_MODE = {"reflect": "symmetric", "grid-mirror": "symmetric", "mirror": "reflect", "nearest": "edge", "wrap": "wrap",
            "grid-wrap": "wrap", "constant": "constant", "grid-constant": "constant"}
STRUCT_DTYPES = ("uint8", "int8", "uint16", "int16", "int32", "uint32", "int64", "float32", "float64")
IN_DTYPES = STRUCT_DTYPES + ("bool", "uint64")
WINDOW_KINDS = ("size", "ones", "holes", "structure", "footprint+structure")
STRUCT_KINDS = ("whole", "eighths", "uniform", "zero")
CVALS = (0, 3, -2, 1.5)
# output dtypes that hold every value of an input within +-100 (and every result of a structure on it)
WIDER = {"uint8": ("int16", "float32", "float64"), "int8": ("int16", "float64"), "uint16": ("int32", "float64"),
         "int16": ("int32", "float64"), "int32": ("int64", "float64"), "uint32": ("int64", "float64"), "float32": ("float64",)}
MUTATIONS = ("no_mirror", "no_even_shift", "first_tap_in_dtype", "erosion_adds", "cval_as_double")


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def to_dtype(a, dtype):
    """the C cast of doubles into `dtype`: double -> int64 -> T for the integer types (truncate, then wrap)"""
    dtype = np.dtype(dtype)
    a = np.asarray(a, dtype=np.float64)
    if dtype.kind == "f":
        return a.astype(dtype)
    if dtype.kind == "b":
        return a != 0
    with np.errstate(invalid="ignore"):
        return a.astype(np.int64).astype(dtype)


def _origins(origin, ndim):
    if np.ndim(origin) == 0:
        return [int(origin)] * ndim
    origin = [int(o) for o in origin]
    if len(origin) != ndim:
        raise RuntimeError("origin must have length equal to input rank")
    return origin


def _check_origin(f, o):
    if f // 2 + o < 0 or f // 2 + o >= f:
        raise ValueError("invalid origin")


def _pad(x, widths, mode, value):
    if PAD_MODE[mode] == "constant":
        return np.pad(x, widths, mode="constant", constant_values=value)
    return np.pad(x, widths, mode=PAD_MODE[mode])


def _pass_1d(x, axis, f, o, mode, cval, is_max, out_dtype):
    """SciPy's minimum_filter1d / maximum_filter1d: a double line buffer, the fill value a double"""
    _check_origin(f, o)
    widths = [(0, 0)] * x.ndim
    widths[axis] = (f // 2 + o, f - 1 - (f // 2 + o))
    big = _pad(x.astype(np.float64), widths, mode, float(cval))
    n = x.shape[axis]
    best = None
    for k in range(f):
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(k, k + n)
        v = big[tuple(sl)]
        best = v.copy() if best is None else np.where((v > best) if is_max else (v < best), v, best)
    return to_dtype(best, out_dtype)


def _pass_nd(x, footprint, structure, origins, mode, cval, is_max, out_dtype, first_tap_in_dtype=False,
             erosion_adds=False, cval_as_double=False):
    """SciPy's NI_MinOrMaxFilter"""
    T = x.dtype
    for f, o in zip(footprint.shape, origins):
        _check_origin(f, o)
    widths = [(f // 2 + o, f - 1 - (f // 2 + o)) for f, o in zip(footprint.shape, origins)]
    if cval_as_double:
        big = _pad(x.astype(np.float64), widths, mode, float(cval))
    else:
        big = _pad(x, widths, mode, to_dtype(cval, T)[()])
    best = None
    for idx in np.argwhere(footprint):
        window = big[tuple(slice(int(k), int(k) + n) for k, n in zip(idx, x.shape))]
        if structure is None:
            v = window.astype(np.float64)
        else:
            s = float(structure[tuple(idx)])
            if not is_max and not erosion_adds:
                s = -s
            if best is None and not first_tap_in_dtype:
                v = window.astype(np.float64) + s
            else:
                w = window if window.dtype == T else to_dtype(window, T)
                with np.errstate(over="ignore"):
                    v = (w + to_dtype(np.full(w.shape, s), T)).astype(np.float64)
        best = v.copy() if best is None else np.where((v > best) if is_max else (v < best), v, best)
    return to_dtype(best, out_dtype)


def min_or_max(x, size, footprint, structure, out_dtype, mode, cval, origin, is_max, **mut):
    """scipy.ndimage._filters._min_or_max_filter"""
    x = np.asarray(x)
    if structure is None and footprint is not None and np.asarray(footprint, bool).all():
        size, footprint = np.asarray(footprint).shape, None
    if structure is None and footprint is None:
        sizes = [int(size)] * x.ndim if np.ndim(size) == 0 else [int(s) for s in size]
        origins = _origins(origin, x.ndim)
        cur, done = x, False
        for ax in range(x.ndim):
            if sizes[ax] > 1:
                cur = _pass_1d(cur, ax, sizes[ax], origins[ax], mode, cval, is_max, out_dtype)
                done = True
        return cur if done else x.astype(out_dtype)
    if structure is not None:
        structure = np.asarray(structure, dtype=np.float64)
    footprint = np.ones(structure.shape, bool) if footprint is None else np.asarray(footprint, bool)
    return _pass_nd(x, footprint, structure, _origins(origin, x.ndim), mode, cval, is_max, out_dtype, **mut)


def _mirror(a):
    return None if a is None else np.asarray(a)[(slice(None, None, -1),) * np.ndim(a)]


def erosion(x, size=None, footprint=None, structure=None, out_dtype=None, mode="reflect", cval=0.0, origin=0,
            no_mirror=False, no_even_shift=False, **mut):
    x = np.asarray(x)
    return min_or_max(x, size, footprint, structure, x.dtype if out_dtype is None else out_dtype, mode, cval, origin, False, **mut)


def dilation(x, size=None, footprint=None, structure=None, out_dtype=None, mode="reflect", cval=0.0, origin=0,
             no_mirror=False, no_even_shift=False, **mut):
    x = np.asarray(x)
    if not no_mirror:
        footprint, structure = _mirror(footprint), _mirror(structure)
    if footprint is not None:
        ext = np.shape(footprint)
    elif structure is not None:
        ext = np.shape(structure)
    else:
        ext = [size] * x.ndim if np.ndim(size) == 0 else list(size)
    origin = [-o - (0 if (f & 1 or no_even_shift) else 1) for o, f in zip(_origins(origin, x.ndim), ext)]
    return min_or_max(x, size, footprint, structure, x.dtype if out_dtype is None else out_dtype, mode, cval, origin, True, **mut)


def _filter_only(is_max):
    def run(x, size=None, footprint=None, structure=None, out_dtype=None, mode="reflect", cval=0.0, origin=0,
            no_mirror=False, no_even_shift=False, **mut):
        x = np.asarray(x)
        return min_or_max(x, size, footprint, None, x.dtype if out_dtype is None else out_dtype, mode, cval, origin, is_max, **mut)
    return run


def _composite(name):
    def run(x, out_dtype=None, **kw):
        x = np.asarray(x)
        assert out_dtype is None or np.dtype(out_dtype) == x.dtype
        with np.errstate(over="ignore"):
            if name == "grey_opening":
                return dilation(erosion(x, **kw), **kw)
            if name == "grey_closing":
                return erosion(dilation(x, **kw), **kw)
            if name == "morphological_gradient":
                return dilation(x, **kw) - erosion(x, **kw)
            if name == "morphological_laplace":
                return dilation(x, **kw) + erosion(x, **kw) - x - x
            if name == "white_tophat":
                tmp = dilation(erosion(x, **kw), **kw)
                return x ^ tmp if x.dtype == np.bool_ else x - tmp
            tmp = erosion(dilation(x, **kw), **kw)
            return tmp ^ x if x.dtype == np.bool_ else tmp - x
    return run


_REF = dict(grey_erosion=erosion, grey_dilation=dilation, minimum_filter=_filter_only(False), maximum_filter=_filter_only(True))
_REF.update({name: _composite(name) for name in COMPOSITES})


# ---------------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------------
def _draw_structure(rng, ext, kind):
    if kind == "whole":
        return rng.integers(-3, 4, size=ext).astype(np.float64)
    if kind == "eighths":                               # k / 8 + 0.1: no float32 holds one of them
        return rng.integers(-24, 24, size=ext) / 8.0 + 0.1
    if kind == "uniform":
        return rng.uniform(0.0, 40.0, size=ext)
    return np.zeros(ext)


def _draw_holes(rng, ext):
    """a footprint with at least one hole and one set tap; one time in three without its centre"""
    fp = rng.random(ext) > rng.choice([0.25, 0.5])
    if fp.all():
        fp.flat[int(rng.integers(fp.size))] = False
    if rng.random() < 0.33:
        fp[tuple(f // 2 for f in ext)] = False
    if not fp.any():
        free = [k for k in range(fp.size) if np.unravel_index(k, ext) != tuple(f // 2 for f in ext)]
        fp.flat[free[int(rng.integers(len(free)))]] = True
    return fp


def _draw_values(rng, shape, dtype, wide, has_st=False):
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.random(shape) < 0.5
    if dt.kind == "f":
        x = rng.normal(0.0, 40.0, size=shape) if not wide else rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 9)
        return x.astype(dt)
    info = np.iinfo(dt)
    lo, hi = (max(info.min, -100), min(info.max, 100)) if not wide else (max(info.min, -2 ** 40), min(info.max, 2 ** 40))
    if wide and has_st and dt == np.int32:
        # tap 0 is a double: beyond the int32 range its store is the one C cast SciPy's compiler does not make through int64
        # (200: two passes of a structure of at most 40, with room)
        lo, hi = lo + 200, hi - 200
    x = rng.integers(lo, hi, size=shape, endpoint=True, dtype=np.int64 if dt != np.uint64 else np.uint64).astype(dt)
    if wide and x.size > 1:                             # the ends of the range are where a wrap shows
        x.flat[int(rng.integers(x.size))] = lo
        x.flat[int(rng.integers(x.size))] = hi
    return x


def draw_case(rng):
    """One random call: dict(func, x, kw, out_kind, out_dtype, out_layout, ...).  `x` is a contiguous host array; `kw` holds
    size / footprint / structure / mode / cval / origin as the function takes them."""
    func = str(rng.choice(FUNCS))
    nd = int(rng.choice([1, 2, 2, 3, 3, 3, 4, 5]))
    top_n, top_f = (8, 6 if nd <= 2 else 4) if nd <= 3 else (4, 2)
    shape = tuple(int(rng.integers(1, top_n + 1)) for _ in range(nd))
    ext = [int(rng.integers(1, top_f + 1)) for _ in range(nd)]

    kinds = WINDOW_KINDS[:3] if func in ("minimum_filter", "maximum_filter") else WINDOW_KINDS
    wkind = str(rng.choice(kinds))
    if wkind == "holes" and int(np.prod(ext)) < 2:
        ext[int(rng.integers(nd))] = 2
    ext = tuple(ext)
    has_st = wkind in ("structure", "footprint+structure")
    dtype = str(rng.choice(STRUCT_DTYPES if has_st else IN_DTYPES))
    if dtype == "bool" and func in ("morphological_gradient", "morphological_laplace"):
        dtype = "uint8"
    dt = np.dtype(dtype)

    kw = {}
    skind = None
    if wkind == "size":
        kw["size"] = ext[0] if len(set(ext)) == 1 and rng.random() < 0.5 else ext
    elif wkind == "ones":
        kw["footprint"] = np.ones(ext, bool)
    elif wkind == "holes":
        kw["footprint"] = _draw_holes(rng, ext)
    else:
        skind = str(rng.choice(STRUCT_KINDS))
        kw["structure"] = _draw_structure(rng, ext, skind)
        if wkind == "footprint+structure":
            kw["footprint"] = _draw_holes(rng, ext) if int(np.prod(ext)) >= 2 and rng.random() < 0.8 else np.ones(ext, bool)

    wide = rng.random() < 1.0 / 3.0
    x = _draw_values(rng, shape, dtype, wide, has_st)
    has_inf = False
    if dt.kind == "f" and func in SIMPLE and rng.random() < 1.0 / 7.0:
        spots = rng.random(shape) < 0.2
        if not spots.any():
            spots.flat[int(rng.integers(spots.size))] = True
        x[spots] = rng.choice([np.inf, -np.inf], size=int(spots.sum())).astype(dt)
        has_inf = True

    # the fill value only shows in the two constant modes: they get a third of the draw, the rest is spread over all eight
    kw["mode"] = str(rng.choice(MODES[6:])) if rng.random() < 0.25 else str(rng.choice(MODES))
    cvals = [c for c in CVALS if c >= 0] if dt.kind in "ub" else list(CVALS)
    kw["cval"] = cvals[int(rng.integers(len(cvals)))]

    # origins: the legal range of an extent f is -(f // 2) .. (f - 1) // 2, for the erosion and (mirrored) the dilation alike
    illegal = False
    if rng.random() < 0.45:
        kw["origin"] = 0
    else:
        kw["origin"] = [int(rng.integers(-(f // 2), (f - 1) // 2 + 1)) for f in ext]
    if rng.random() < 0.1:
        # outside the range on an axis whose extent is above 1 (an all-ones window skips the axes of extent 1)
        axes = [d for d in range(nd) if ext[d] > 1]
        if axes:
            d = axes[int(rng.integers(len(axes)))]
            o = _origins(kw["origin"], nd)
            o[d] = int(rng.choice([-(ext[d] // 2) - 1, (ext[d] - 1) // 2 + 1]))
            kw["origin"] = o
            illegal = True

    u = rng.random()
    out_dtype, out_layout = dtype, None
    if u < 0.4:
        out_kind = "none"
    elif u < 0.55 and func in SIMPLE:
        out_kind = "dtype"
    elif u < 0.55:
        out_kind = "none"
    else:
        out_kind = "array"
        layouts = ["c", "c", "strided"] + (["input"] if func in ("grey_erosion", "grey_dilation") else [])
        out_layout = str(rng.choice(layouts))
    if out_kind != "none" and out_layout != "input" and func in SIMPLE and not wide and dtype in WIDER and rng.random() < 0.7:
        out_dtype = str(rng.choice(WIDER[dtype]))

    case = dict(func=func, x=x, kw=kw, out_kind=out_kind, out_dtype=out_dtype, out_layout=out_layout, shape=shape,
                dtype=dtype, ext=ext, wkind=wkind, skind=skind, wide=wide, has_inf=has_inf, illegal=illegal)
    case["desc"] = (func, shape, dtype, "wide" if wide else "+-100", "inf" if has_inf else "", wkind, ext, skind, kw["mode"],
                    kw["cval"], kw["origin"], "out " + out_kind + ("" if out_kind == "none" else ":" + out_dtype +
                                                                  (":" + out_layout if out_layout else "")))
    return case


def make_case(func, x, out_kind="none", out_dtype=None, out_layout=None, **kw):
    """a hand-made case in the form of a drawn one"""
    x = np.ascontiguousarray(x)
    kw.setdefault("mode", "reflect")
    kw.setdefault("cval", 0.0)
    kw.setdefault("origin", 0)
    return dict(func=func, x=x, kw=kw, out_kind=out_kind, out_dtype=x.dtype.name if out_dtype is None else out_dtype,
                out_layout=out_layout, shape=x.shape, dtype=x.dtype.name, illegal=False,
                desc=(func, x.shape, x.dtype.name, out_kind, out_dtype, out_layout))


SEED, CASES = 38, 600
_DRAWN = []


def drawn():
    """the seeded draw the yardstick proves and the device runs (made once; nothing changes a case)"""
    if not _DRAWN:
        rng = np.random.default_rng(SEED)
        _DRAWN.extend(draw_case(rng) for _ in range(CASES))
        for case in _DRAWN:
            for a in [case["x"]] + [v for v in case["kw"].values() if isinstance(v, np.ndarray)]:
                a.setflags(write=False)
    return _DRAWN


def family(case):
    """the groups the device fuzz is parametrised by"""
    f = case["func"]
    if f in ("grey_erosion", "minimum_filter"):
        return "erosion"
    if f in ("grey_dilation", "maximum_filter"):
        return "dilation"
    if f in ("grey_opening", "grey_closing"):
        return "open-close"
    if f in ("morphological_gradient", "morphological_laplace"):
        return "gradient-laplace"
    return "tophat"


FAMILIES = ("erosion", "dilation", "open-close", "gradient-laplace", "tophat")


def has_structure(case):
    """a structure always ends in mi_minmax_nd's generic kernels: no separable, run or tiled route takes one"""
    return case["kw"].get("structure") is not None


def reference(case, **mutations):
    """the reference's result of a drawn case in the output dtype, or a ValueError instance for an illegal origin"""
    kw = dict(case["kw"])
    try:
        return _REF[case["func"]](case["x"], out_dtype=np.dtype(case["out_dtype"]), **kw, **mutations)
    except ValueError as e:
        return e


def call(mod, case, to_array=None, x=None):
    """Run the case through `mod` (scipy.ndimage or the device module; `to_array` puts a host array on the device; `x`: the
    input where the caller has put it there already).  Returns (what the function returned or the ValueError it raised, the
    array given as output or None, (the allocation that array lies in, the bytes between its samples before the call) or
    None), arrays as the module's own."""
    put = to_array or (lambda a: a)
    if x is None or case["out_layout"] == "input":      # a call that writes into its input gets an input of its own
        x = put(case["x"].copy())
    kw = dict(case["kw"])
    out = base = None
    if case["out_kind"] == "dtype":
        kw["output"] = np.dtype(case["out_dtype"])
    elif case["out_kind"] == "array":
        if case["out_layout"] == "input":
            out = x
        else:
            shape = tuple(case["shape"])
            if case["out_layout"] == "strided":
                shape = shape[:-1] + (2 * shape[-1],)
            host = (np.full(shape, 77, dtype=np.uint8).view(np.bool_) if case["out_dtype"] == "bool" else
                    np.full(shape, 77, dtype=case["out_dtype"]))
            base = (put(host), host[..., 1::2].tobytes())
            out = base[0][..., ::2] if case["out_layout"] == "strided" else base[0]
        kw["output"] = out
    try:
        ret = getattr(mod, case["func"])(x, **kw)
    except ValueError as e:
        ret = e
    return ret, out, base


def to_host(a):
    return a.get() if hasattr(a, "get") and not isinstance(a, np.ndarray) else np.asarray(a)


def judge(case, want, got):
    """(ok, why): the outcome `got` of call() against the reference's result `want`; dtype, shape and every element"""
    ret, out, base = got
    if isinstance(want, ValueError):
        return (True, "") if isinstance(ret, ValueError) else (False, "an illegal origin did not raise ValueError")
    if isinstance(ret, ValueError):
        return False, "raised ValueError: %s" % ret
    if ret is None:
        return False, "returned None"
    if case["out_kind"] == "array":
        if ret is not out:
            return False, "did not return the output array"
        if base is not None and case["out_layout"] == "strided" and to_host(base[0])[..., 1::2].tobytes() != base[1]:
            return False, "wrote between the samples of a strided output"
    res = to_host(ret)
    if res.dtype != want.dtype:
        return False, "dtype %s, not %s" % (res.dtype, want.dtype)
    if res.shape != want.shape:
        return False, "shape %s, not %s" % (res.shape, want.shape)
    if not np.array_equal(res, want, equal_nan=res.dtype.kind == "f"):
        bad = np.argwhere(~((res == want) | ((res != res) & (want != want))))
        at = tuple(int(v) for v in bad[0])
        return False, "%d of %d voxels differ, first at %s: %r, not %r" % (len(bad), want.size, at, res[at], want[at])
    return True, ""
