"""Randomised differential test of the HIP path against scipy.ndimage (run on the GPU box).
usage: python scripts/fuzz_vs_scipy.py [--ranges | --measure | --binary] [seconds] [seed] [max cases]   -- prints mismatches with
their parameters.
env FUZZ_ONLY=op1,op2 restricts the op families, FUZZ_TRACE=1 prints every case before it runs.
--ranges: a separate draw on the value ranges of real scans (MR 0 .. 4095, CT Hounsfield units with padding, 1e4 + noise,
full-range 16-bit integers; tests/helpers/value_ranges.py): float results are judged per voxel by |got - ref64| <= c u B,
integer results bit for bit.  Without it the draw is the seeded one tests/test_gpu_fuzz.py depends on.
--measure: a separate draw of ndimage.label (ranks 1-4, shapes either side of the 8x16x32 / 1x64x64 tiles, every
connectivity and random centrosymmetric structures, bool / integer / float inputs with NaN and -0.0, int32 / int64 /
uint32 outputs; bit-exact against SciPy, a share of them also against the generic route) and of every labelled
reduction (tests/helpers/measure_ref.py: the value ranges above with +-0, +-inf and NaN, every label dtype, index
None / scalar / list / host / device array with duplicates, absent, 0 and negative values, slot counts around the LDS
limits and index ranges either side of the lookup-table threshold).  Reductions are judged against a host float64
reference with the bounds derived in measure_ref's docstring, exact where the result is an integer, an extreme, a
position or a sum of integers; result type, shape, dtype and exceptions against SciPy.
--binary: a separate draw of binary morphology on real masks (tests/helpers/binary_ref.py draw_case: every binary_*
function, ranks 1-5, every input dtype with NaN / inf / -0.0 / subnormals / values that are zero in their low byte,
structures of every kind, origins, masks of several dtypes, iteration counts up to 13 and runs until stable, every form
of `output`, strided and transposed inputs).  Results are judged bit for bit against the plain NumPy reference of that
module (itself checked against SciPy by tests/test_binary_yardstick.py), together with the dtype, the return value and
the bytes between the samples of a strided output; where the reference raises, the exception type against SciPy's.
No case is skipped."""
import os, sys, time, traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RANGES = "--ranges" in sys.argv
if RANGES:
    sys.argv.remove("--ranges")
MEASURE = "--measure" in sys.argv
if MEASURE:
    sys.argv.remove("--measure")
BINARY = "--binary" in sys.argv
if BINARY:
    sys.argv.remove("--binary")
import numpy as np
import scipy.ndimage as sndi
import cupyimg_amd as ca
from cupyimg_amd.scipy import ndimage as ndi

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
max_cases = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 60
rng = np.random.default_rng(seed)
MODES = ["reflect", "constant", "nearest", "mirror", "wrap"]
DTYPES = ["float32", "float32", "float32", "float64", "uint8", "uint8", "int16", "uint16", "int32"]
if os.environ.get("FUZZ_BIG"):
    DTYPES = ["float32", "float32", "uint8", "uint8", "int16", "uint16", "float64"]

BIG = bool(os.environ.get("FUZZ_BIG"))      # mid-size volumes / images: the tiling and chunk planning of the fast kernels


def rand_shape():
    if BIG:
        if rng.random() < 0.7:
            return (int(rng.integers(20, 140)), int(rng.integers(30, 200)), int(rng.choice([4 * rng.integers(16, 160), 256, 512, 768, 1024])))
        return (int(rng.integers(200, 1500)), int(rng.choice([4 * rng.integers(60, 500), 1024, 2048, rng.integers(300, 1500)])))
    nd = int(rng.choice([1, 2, 2, 3, 3, 3]))
    if nd == 3:
        last = int(rng.choice([rng.integers(1, 40), 4 * rng.integers(2, 24), 256, 260, 264, 268, 272, 516, 520]))
        return (int(rng.integers(1, 24)), int(rng.integers(1, 40)), last)
    if nd == 2:
        return (int(rng.integers(1, 70)), int(rng.choice([rng.integers(1, 90), 4 * rng.integers(2, 40), 1024, 1028, 1032, 260, 264])))
    return (int(rng.integers(1, 300)),)

def rand_array(shape, dtype):
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal(shape).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(max(info.min, -200), min(info.max, 250) + 1, size=shape).astype(dtype)

def tol_for(dtype, ref):
    k = np.dtype(dtype).kind
    if k in "iub":
        return 0
    return (3e-6 if dtype == "float32" else 1e-11) * max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)

def origin_for(size):
    lo, hi = -(size // 2), (size - 1) // 2
    return int(rng.integers(lo, hi + 1))

def case():
    shape = rand_shape()
    dtype = str(rng.choice(DTYPES))
    x = rand_array(shape, dtype)
    mode = str(rng.choice(MODES))
    cval = float(rng.choice([0.0, 3.0, -2.0]))
    if np.dtype(dtype).kind == "u":
        cval = abs(cval)        # negative cval on unsigned data: SciPy's own paths disagree with each other
    op = str(rng.choice(["uniform", "gaussian", "correlate1d", "correlate", "minmax", "minmax_fp", "grey", "median", "binary",
                         "sobel", "laplace", "map1", "affine3", "zoom", "shift", "binary2", "grey_st", "percentile", "spline_filter",
                         "uniform1d", "convolve1d"]))
    if os.environ.get("FUZZ_ONLY"):
        op = str(rng.choice(os.environ["FUZZ_ONLY"].split(",")))
    nd = x.ndim
    kw = dict(mode=mode, cval=cval)
    if op == "uniform":
        size = [int(rng.integers(1, 8)) for _ in range(nd)]
        origin = [origin_for(s) for s in size]
        odt = rng.choice([None, "float32", "float64", "int16"])
        okw = dict(kw) if odt is None else dict(kw, output=np.dtype(str(odt)))
        return op, (shape, dtype, size, origin, okw), lambda m, a: m.uniform_filter(a, size=size, origin=origin, **okw), 1
    if op == "gaussian":
        sigma = [float(rng.choice([0.0, 0.6, 1.0, 1.7])) for _ in range(nd)]
        order = [int(rng.integers(0, 3)) for _ in range(nd)]
        odt = rng.choice([None, None, "float32", "float64"])
        okw = dict(kw) if odt is None else dict(kw, output=np.dtype(str(odt)))
        return op, (shape, dtype, sigma, order, okw), lambda m, a: m.gaussian_filter(a, sigma, order=order, **okw), 4
    if op == "correlate1d":
        w = rng.standard_normal(int(rng.integers(1, 9)))
        ax = int(rng.integers(0, nd))
        origin = origin_for(len(w))
        return op, (shape, dtype, w.tolist(), ax, origin, kw), lambda m, a: m.correlate1d(a, w, axis=ax, origin=origin, **kw) if m is sndi else m.correlate1d(a, w, axis=ax, origin=origin, dtype_mode="ndimage", **kw), 4
    if op == "correlate":
        wshape = tuple(int(rng.integers(1, 5)) for _ in range(nd))
        w = rng.standard_normal(wshape)
        origin = [origin_for(s) for s in wshape]
        f = "correlate" if rng.random() < 0.5 else "convolve"
        if f == "convolve":
            origin = [o if -(s // 2) <= -o - (1 if s % 2 == 0 else 0) <= (s - 1) // 2 else 0 for o, s in zip(origin, wshape)]
        return op + ":" + f, (shape, dtype, wshape, origin, kw), lambda m, a: getattr(m, f)(a, w, origin=origin, **kw), 8
    if op == "minmax":
        size = [int(rng.integers(1, 8)) for _ in range(nd)]
        origin = [origin_for(s) for s in size]
        f = str(rng.choice(["minimum_filter", "maximum_filter"]))
        odt = rng.choice([None, None, "float32", "float64", "int32"])
        okw = dict(kw) if odt is None else dict(kw, output=np.dtype(str(odt)))
        return op + ":" + f, (shape, dtype, size, origin, okw), lambda m, a: getattr(m, f)(a, size=size, origin=origin, **okw), 0
    if op == "minmax_fp":
        fshape = tuple(int(rng.integers(1, 5)) for _ in range(nd))
        fp = rng.random(fshape) > 0.4
        if not fp.any():
            fp.flat[0] = True
        f = str(rng.choice(["minimum_filter", "maximum_filter"]))
        return op + ":" + f, (shape, dtype, fp.astype(int).tolist(), kw), lambda m, a: getattr(m, f)(a, footprint=fp, **kw), 0
    if op == "grey":
        size = [int(rng.integers(1, 8))] * nd
        f = str(rng.choice(["grey_erosion", "grey_dilation"]))
        return op + ":" + f, (shape, dtype, size, kw), lambda m, a: getattr(m, f)(a, size=size, **kw), 0
    if op == "median":
        size = int(rng.integers(2, 4 if nd == 3 else 6))
        if nd == 1 and shape[0] < size:
            # SciPy 1.15's 1-D rank filter returns garbage for arrays shorter than the window (median_filter([7], 5)
            # -> 1; its own n-D path on the same data as a (1, n) image is right): compare with that embedding
            return op, (shape, dtype, size, kw), lambda m, a: (m.median_filter(a[None, :], size=(1, size), **kw)[0]
                                                               if m is sndi else m.median_filter(a, size=size, **kw)), 0
        return op, (shape, dtype, size, kw), lambda m, a: m.median_filter(a, size=size, **kw), 0
    if op == "binary":
        st = sndi.generate_binary_structure(nd, int(rng.integers(1, nd + 1)))
        it = int(rng.choice([1, 1, 2, 3]))
        bv = int(rng.integers(0, 2))
        f = str(rng.choice(["binary_erosion", "binary_dilation"]))
        return op + ":" + f, (shape, dtype, it, bv), lambda m, a: getattr(m, f)(a, structure=st, iterations=it, border_value=bv), 0
    if op == "binary2":
        sshape = tuple(int(rng.integers(1, 5)) for _ in range(nd))
        st = rng.random(sshape) > 0.35
        if not st.any():
            st.flat[0] = True
        origin = [origin_for(k) for k in sshape]
        mask = rng.random(shape) > 0.3 if rng.random() < 0.5 else None
        it = int(rng.choice([1, 2]))
        bv = int(rng.integers(0, 2))
        f = str(rng.choice(["binary_erosion", "binary_dilation"]))
        if f == "binary_dilation":      # dilation mirrors the structure: keep the mirrored origin legal for even sizes
            origin = [o if -(k // 2) <= -o - (1 if k % 2 == 0 else 0) <= (k - 1) // 2 else 0 for o, k in zip(origin, sshape)]
        return op + ":" + f, (shape, dtype, st.astype(int).tolist(), origin, it, bv, mask is not None), \
            lambda m, a: getattr(m, f)(a, structure=st, iterations=it, border_value=bv, origin=origin, brute_force=True,
                                       mask=(mask if (m is sndi or mask is None) else ca.asarray(mask))), 0
        # brute_force=True: SciPy 1.15's coordinate-list path (iterations > 1) corrupts the heap for even-sized
        # structures with an origin ("double free or corruption" in pure SciPy); the reference only has brute force
    if op == "grey_st":
        sshape = tuple(int(rng.integers(1, 4)) for _ in range(nd))
        fp = rng.random(sshape) > 0.3
        if not fp.any():
            fp.flat[0] = True
        stv = rng.integers(0, 5, size=sshape).astype(np.float64)
        f = str(rng.choice(["grey_erosion", "grey_dilation"]))
        return op + ":" + f, (shape, dtype, fp.astype(int).tolist(), stv.tolist(), kw), \
            lambda m, a: getattr(m, f)(a, footprint=fp, structure=stv, **kw), 0
    if op == "percentile":
        size = int(rng.integers(2, 4 if nd == 3 else 5))
        pct = float(rng.choice([0, 10, 35.5, 50, 80, 100, -20]))
        if nd == 1 and shape[0] < size:     # see "median"
            return op, (shape, dtype, size, pct, kw), lambda m, a: (m.percentile_filter(a[None, :], pct, size=(1, size), **kw)[0]
                                                                    if m is sndi else m.percentile_filter(a, pct, size=size, **kw)), 0
        return op, (shape, dtype, size, pct, kw), lambda m, a: m.percentile_filter(a, pct, size=size, **kw), 0
    if op == "spline_filter":
        order = int(rng.integers(2, 6))
        smode = str(rng.choice(["mirror", "reflect", "grid-wrap", "nearest", "constant"]))
        return op, (shape, "float64", order, smode), lambda m, a: m.spline_filter(a.astype(np.float64) if m is sndi else a, order=order, mode=smode), 1000
    if op == "uniform1d":
        size = int(rng.integers(1, 9))
        ax = int(rng.integers(0, nd))
        origin = origin_for(size)
        return op, (shape, dtype, size, ax, origin, kw), lambda m, a: m.uniform_filter1d(a, size, axis=ax, origin=origin, **kw), 1
    if op == "convolve1d":
        w = rng.integers(-3, 4, size=int(rng.integers(1, 8))).astype(np.float64)
        ax = int(rng.integers(0, nd))
        origin = origin_for(len(w))
        if not (-(len(w) // 2) <= -origin - (1 if len(w) % 2 == 0 else 0) <= (len(w) - 1) // 2):
            origin = 0
        return op, (shape, dtype, w.tolist(), ax, origin, kw), lambda m, a: m.convolve1d(a, w, axis=ax, origin=origin, **kw) if m is sndi else m.convolve1d(a, w, axis=ax, origin=origin, dtype_mode="ndimage", **kw), 4
    if op == "sobel":
        ax = int(rng.integers(0, nd))
        return op, (shape, dtype, ax, kw), lambda m, a: m.sobel(a, axis=ax, **kw), 4
    if op == "laplace":
        return op, (shape, dtype, kw), lambda m, a: m.laplace(a, **kw), 8
    imode = str(rng.choice(["constant", "nearest", "mirror", "reflect", "wrap", "grid-wrap", "grid-constant"]))
    ikw = dict(mode=imode, cval=cval)
    if op == "map1":
        npts = int(rng.integers(1, 500))
        coords = (rng.random((nd, npts)) * (np.array(shape)[:, None] + 4) - 2)
        order = int(rng.choice([0, 1, 1, 3]))
        if order == 0:
            coords = np.floor(coords * 4) / 4 + 0.1      # keep away from the .5 ties (documented deviation of the reference)
        return op, (shape, dtype, npts, order, ikw), lambda m, a: m.map_coordinates(a, coords if m is sndi else ca.asarray(coords), order=order, **ikw), 40
    if op == "affine3":
        A = np.eye(nd) + 0.15 * rng.standard_normal((nd, nd))
        off = rng.standard_normal(nd) * 2
        order = int(rng.choice([1, 3, 3, 2, 5]))
        return op, (shape, dtype, order, ikw), lambda m, a: m.affine_transform(a, A, offset=off, order=order, **ikw), 40
    if op == "zoom":
        zf = float(rng.choice([0.5, 0.8, 1.0, 1.3, 2.0]))
        order = int(rng.choice([0, 1, 3, 3]))
        return op, (shape, dtype, zf, order, ikw), lambda m, a: m.zoom(a, zf, order=order, **ikw), 40
    sh = [float(rng.choice([0.0, 1.5, -2.25, 0.3])) for _ in range(nd)]
    order = int(rng.choice([0, 1, 3, 3]))
    return "shift", (shape, dtype, sh, order, ikw), lambda m, a: m.shift(a, sh, order=order, **ikw), 40

def ndi_gt0(a):
    return a          # binary ops treat any non-zero as foreground


def ranges_case():
    """(name, params, x, device call, SciPy call, bound or None for bit-exact) of the --ranges draw."""
    from helpers import value_ranges as vr
    nd = int(rng.choice([2, 3, 3]))
    shape = (tuple(int(v) for v in rng.integers(8, 48, size=2)) if nd == 3 else (int(rng.integers(8, 200)),)) + \
        (int(rng.choice([rng.integers(8, 130), 4 * rng.integers(2, 40), 256])),)
    gen = str(rng.choice(["mr_u12", "ct_hu", "offset_1e4", "extremes", "mr_u12_u16", "ct_hu_i16"]))
    seed = int(rng.integers(1 << 30))
    if gen in ("mr_u12", "ct_hu", "offset_1e4"):
        x = vr.offset_1e4(shape, seed) if gen == "offset_1e4" else getattr(vr, gen)(shape, seed, dtype=np.float32)
        mode = str(rng.choice(MODES + ["grid-wrap", "grid-constant"]))
        cval = float(rng.choice([0.0, -1024.0, -1000.3, 4095.0]))
        kind = str(rng.choice(["uniform", "gaussian", "sobel", "prewitt", "correlate"]))
        if kind == "uniform":
            size = [int(rng.choice([1, 3, 5, 7, 9, 13])) for _ in range(nd)]
            w = vr.box_spec(nd, size)
            f = lambda m, a: m.uniform_filter(a, size, mode=mode, cval=cval)
            params = (shape, gen, kind, size, mode, cval)
        elif kind == "gaussian":
            sig = [float(rng.choice([0.0, 0.7, 1.0, 1.5, 2.0, 3.0])) for _ in range(nd)]
            od = [int(rng.choice([0, 0, 1, 2])) for _ in range(nd)]
            if not any(s_ > 0 for s_ in sig):
                sig[-1] = 1.0
            w = vr.gaussian_spec(nd, sig, od)
            f = lambda m, a: m.gaussian_filter(a, sig, od, mode=mode, cval=cval)
            params = (shape, gen, kind, sig, od, mode, cval)
        elif kind in ("sobel", "prewitt"):
            ax = int(rng.integers(nd))
            w = vr.deriv_spec(nd, ax, [1, 2, 1] if kind == "sobel" else [1, 1, 1])
            f = lambda m, a: getattr(m, kind)(a, ax, mode=mode, cval=cval)
            params = (shape, gen, kind, ax, mode, cval)
            return kind, params, x, f, (vr.abs_separable(w, mode, cval, vr.deriv_order(nd, ax)), vr.sep_c(w))
        else:
            wt = rng.standard_normal((3,) * nd)
            f = lambda m, a: m.correlate(a, wt, mode=mode, cval=cval, dtype_mode="float") if m is ndi else \
                m.correlate(a.astype(np.float64), wt, mode=mode, cval=cval)
            params = (shape, gen, "correlate(float mode)", mode, cval)
            return kind, params, x, f, (vr.abs_dense(wt, mode, cval), vr.dense_c(wt))
        return kind, params, x, f, (vr.abs_separable(w, mode, cval), vr.sep_c(w))
    dt = np.uint16 if gen in ("mr_u12_u16",) or (gen == "extremes" and rng.random() < 0.5) else np.int16
    x = vr.mr_u12(shape, seed) if gen == "mr_u12_u16" else vr.ct_hu(shape, seed) if gen == "ct_hu_i16" else vr.int_extremes(shape, dt, seed)
    info = np.iinfo(x.dtype)
    mode = str(rng.choice(MODES))
    cval = float(rng.choice([0.0, float(info.min), float(info.max)]))
    kind = str(rng.choice(["uniform", "minimum", "maximum", "median3", "grey_erosion"]))
    size = [int(rng.choice([1, 3, 5, 7, 9])) for _ in range(nd)]
    if kind == "uniform":
        f = lambda m, a: m.uniform_filter(a, size, mode=mode, cval=cval)
    elif kind in ("minimum", "maximum"):
        f = lambda m, a: getattr(m, kind + "_filter")(a, size, mode=mode, cval=cval)
    elif kind == "median3":
        f = lambda m, a: m.median_filter(a, 3, mode=mode, cval=cval)
    else:
        f = lambda m, a: m.grey_erosion(a, size=size, mode=mode, cval=cval)
    return kind, (shape, gen, str(x.dtype), kind, size, mode, cval), x, f, None


def run_ranges():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from helpers import value_ranges as vr
    t_end = time.time() + budget
    n = fails = 0
    worst = {}
    while time.time() < t_end and n < max_cases:
        name, params, x, f, bound = ranges_case()
        if os.environ.get("FUZZ_TRACE"):
            print("TRACE", name, params, flush=True)
        got = f(ndi, ca.asarray(x)).get()
        n += 1
        if bound is None:
            ok = np.array_equal(got, f(sndi, x))
            r = 0.0 if ok else float("inf")
        else:
            x64 = x.astype(np.float64)
            r, at = vr.ratio_of(got, np.asarray(f(sndi, x64), np.float64), bound[0](np.abs(x64)), bound[1])
            ok = r <= 1.0
        key = name + (" exact" if bound is None else " bound")
        worst[key] = max(worst.get(key, 0.0), r)
        if not ok:
            fails += 1
            print("MISMATCH", name, params, "ratio", r, "kernel", ca.last_kernel(), flush=True)
    print("ranges: cases %d, failures %d, worst ratio per op %s" % (n, fails, {k: round(v, 4) for k, v in sorted(worst.items())}))
    return fails


def label_case():
    """(params, x, structure, output dtype) of the --measure draw's label cases"""
    nd = int(rng.choice([1, 2, 2, 3, 3, 4]))
    near = lambda: int(rng.choice([1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, rng.integers(2, 40)]))
    if nd == 1:
        shape = (int(rng.choice([1, 63, 64, 65, rng.integers(2, 5000)])),)
    elif nd == 2:
        shape = (near(), int(rng.choice([63, 64, 65, 127, 128, 129, near()])))
    elif nd == 3:
        shape = (int(rng.choice([1, 7, 8, 9, 15, 16, 17, rng.integers(2, 24)])), near(), int(rng.choice([31, 32, 33, 64, near()])))
    else:
        shape = tuple(int(rng.integers(1, 10)) for _ in range(4))
    density = float(rng.choice([0.0, 1.0, rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7)]))
    fg = rng.random(shape) < density
    dtype = str(rng.choice(["bool", "uint8", "int16", "int32", "float32", "float64"]))
    x = (fg * rng.integers(1, 4, shape)).astype(dtype)
    if x.dtype.kind == "f":
        x[fg & (rng.random(shape) < 0.1)] = np.nan               # NaN is foreground
        x[~fg & (rng.random(shape) < 0.5)] = -0.0                # -0.0 is background
    if rng.random() < 0.3:
        st = rng.random((3,) * nd) > 0.5
        st = st | st[(slice(None, None, -1),) * nd]
        st[(1,) * nd] = True
        sname = "random"
    else:
        conn = int(rng.integers(1, nd + 1))
        st = sndi.generate_binary_structure(nd, conn)
        sname = "conn%d" % conn
    out = rng.choice([None, np.int64, np.uint32])
    return (shape, dtype, round(density, 2), sname, None if out is None else np.dtype(out).name), x, st, out


def run_measure():
    import warnings
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from helpers import measure_ref as mr
    from cupyimg_amd import _lib
    lib = _lib.load()
    warnings.simplefilter("ignore")
    t_end = time.time() + budget
    n = fails = 0
    worst, counts = {}, {}
    while time.time() < t_end and n < max_cases:
        n += 1
        if rng.random() < 0.3:
            params, x, st, out = label_case()
            if os.environ.get("FUZZ_TRACE"):
                print("TRACE label", params, flush=True)
            ref, rn = sndi.label(x, st, output=out)
            got, gn = ndi.label(ca.asarray(x), st, output=out)
            ok = gn == rn and got.dtype == ref.dtype and np.array_equal(got.get(), ref)
            if ok and out is None and rng.random() < 0.35:      # the same labels from the generic route
                lib.mi_debug_set_label_generic(1)
                try:
                    gen, _ = ndi.label(ca.asarray(x), st, output=out)
                    ok = np.array_equal(gen.get(), got.get()) and ("label_connect_kernel" in ca.last_kernel() or x.size == 0 or x.ndim == 0)
                finally:
                    lib.mi_debug_set_label_generic(0)
            counts["label"] = counts.get("label", 0) + 1
            if not ok:
                fails += 1
                print("MISMATCH label", params, "num", gn, rn, "kernel", ca.last_kernel(), flush=True)
            continue
        case = mr.draw_reduction(rng)
        desc = (case["func"], case["x"].shape, str(case["x"].dtype), case["gen"],
                None if case["labels"] is None else str(case["labels"].dtype), case["index_kind"],
                None if case["index"] is None else np.size(case["index"]), case["kw"])
        if os.environ.get("FUZZ_TRACE"):
            print("TRACE", desc, flush=True)
        want = want_exc = got = got_exc = None
        try:
            want = mr.call(sndi, case)
        except Exception as e:
            want_exc = e
        try:
            got = mr.call(ndi, case, ca.asarray)
        except Exception as e:
            got_exc = e
        ok, r, why = mr.judge(case, got, want, want_exc, got_exc)
        counts[case["func"]] = counts.get(case["func"], 0) + 1
        if r != float("inf"):
            worst[case["func"]] = max(worst.get(case["func"], 0.0), r)
        if not ok:
            fails += 1
            print("MISMATCH", desc, why, "kernel", ca.last_kernel(), flush=True)
    print("measure: cases %d, failures %d, per op %s" % (n, fails, counts))
    print("measure: worst bound ratio per op %s" % {k: round(v, 4) for k, v in sorted(worst.items())})
    return fails


def run_binary():
    import warnings
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from helpers import binary_ref as br
    warnings.simplefilter("ignore")
    t_end = time.time() + budget
    n = fails = 0
    counts = {}
    while time.time() < t_end and n < max_cases:
        case = br.draw_case(rng)
        n += 1
        counts[case["func"]] = counts.get(case["func"], 0) + 1
        if os.environ.get("FUZZ_TRACE"):
            print("TRACE", case["desc"], flush=True)
        want = want_exc = got_exc = None
        try:
            want = br.reference(case)
        except Exception as e:
            want_exc = e
        try:
            ret, out, base = br.call(ndi, case, ca.asarray)
        except Exception as e:
            got_exc = e
        if want_exc is not None:
            # the reference refuses: SciPy decides what the call should have done
            try:
                sret, sout, sbase = br.call(sndi, case, f16_as_f32=True)
                ok = got_exc is None
                why = "SciPy answers, the reference raised %r" % (want_exc,)
                if ok:
                    ok, why = br.judge(case, br.truth(br.to_host(sout if sout is not None else sret)), ret, out, base)
            except Exception as se:
                ok, why = type(got_exc) is type(se), "raised %r, SciPy %r" % (got_exc, se)
        elif got_exc is not None:
            ok, why = False, "raised %r" % (got_exc,)
        else:
            ok, why = br.judge(case, want, ret, out, base)
        if not ok:
            fails += 1
            print("MISMATCH", case["desc"], why, "kernel", ca.last_kernel(), flush=True)
    print("binary: cases %d, failures %d, per op %s" % (n, fails, counts))
    return fails


if RANGES:
    sys.exit(1 if run_ranges() else 0)
if MEASURE:
    sys.exit(1 if run_measure() else 0)
if BINARY:
    sys.exit(1 if run_binary() else 0)

t_end = time.time() + budget
n = fails = skipped = 0
counts = {}
cats = {}
while time.time() < t_end and n < max_cases:
    st = rng.bit_generator.state
    try:
        name, params, fn, slack = case()
        shape, dtype = params[0], params[1]
        x = rand_array(shape, dtype)
    except Exception:
        traceback.print_exc()
        break
    if os.environ.get("FUZZ_TRACE"):
        print("TRACE", name, params, flush=True)
    try:
        view = int(rng.integers(0, 4))           # 0/1: contiguous, 2: every other sample of a larger array, 3: transposed
        if view == 2 and x.ndim >= 2:
            big = np.repeat(x, 2, axis=-1)
            big[..., 1::2] = 77
            xh, xd = big[..., ::2], ca.asarray(big)[..., ::2]
        elif view == 3 and x.ndim >= 2:
            xt = np.ascontiguousarray(np.swapaxes(x, 0, -1))
            xh, xd = np.swapaxes(xt, 0, -1), ca.asarray(xt).transpose(*([x.ndim - 1] + list(range(1, x.ndim - 1)) + [0]))
        else:
            xh, xd = x, ca.asarray(x)
        assert xh.shape == tuple(xd.shape) == x.shape
        want = fn(sndi, xh)
        got = fn(ndi, xd).get()
    except (NotImplementedError, RuntimeError, ValueError, ZeroDivisionError) as exc:
        # both sides are allowed to refuse; a refusal on one side only is worth a look
        try:
            fn(sndi, x)
            print("REFUSED by the HIP path only:", name, params, type(exc).__name__, str(exc)[:100], flush=True)
            fails += 1
        except Exception:
            skipped += 1
        continue
    n += 1
    counts[name.split(":")[0]] = counts.get(name.split(":")[0], 0) + 1
    ok = got.shape == want.shape and got.dtype == want.dtype
    if ok and want.size:
        in_dtype, dtype = dtype, str(want.dtype)
        mixed_int = np.dtype(dtype).kind in "iu" and np.dtype(in_dtype).kind == "f"
        tol = tol_for(dtype, want)
        if np.dtype(dtype).kind == "f" and in_dtype == "float32":
            tol = max(tol, tol_for("float32", want))
        if mixed_int:
            # a float result truncated into an integer output: one unit at values that sit on an integer
            diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
            ok = (diff <= 1).all() and (diff > 0).mean() <= 2e-3
            tol = None
        if tol is None:
            pass
        elif tol == 0 and name.split(":")[0] in ("map1", "affine3", "zoom", "shift"):
            # integer outputs of interpolation: equal up to the rounding of a value that sits within 1e-9 of a tie
            diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
            ok = (diff <= 1).all() and (diff > 0).mean() <= (2e-2 if params[-2] >= 2 else 0.0)   # ties of spline orders only
        elif tol == 0:
            ok = np.array_equal(got, want)
        else:
            t = tol * (1 + slack)
            if dtype == "float32" and name.split(":")[0] in ("affine3", "zoom", "shift", "map1"):
                t = max(t, 8e-5 * max(1.0, float(np.abs(want).max())))
            ok = np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= t
    if not ok:
        fails += 1
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max() if got.shape == want.shape else "shape"
        key = (name, in_dtype if 'in_dtype' in dir() else dtype, dtype)
        cats[key] = cats.get(key, 0) + 1
        if cats[key] <= 3:
            nbad = int((got != want).sum()) if got.shape == want.shape else -1
            print("MISMATCH", name, params, "err", err, "nbad", nbad, "of", want.size, flush=True)
for k in sorted(cats):
    print("  failures", k, cats[k])
print("cases %d, refused on both sides %d, failures %d, per op %s" % (n, skipped, fails, counts))
