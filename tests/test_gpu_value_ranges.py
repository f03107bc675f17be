"""The kernels on the value ranges of real scans (tests/helpers/value_ranges.py): MR magnitudes 0 .. 4095, CT Hounsfield
units with a -32768 / -1024 padding border, 1e4 + N(0, 1), and full-range integers.

Every float case is judged per voxel by |got - ref64| <= c . u . B (the module docstring of helpers/value_ranges.py;
proved on SciPy's own float32 results by tests/test_value_range_harness.py); the smoothing filters keep, besides, the
max-norm contract of the rest of the suite (1e-6 . max|ref| against float64 SciPy).  Integer results and the default
(float64-accumulating) dense correlate are bit-identical to SciPy.  Every case names the kernel it expects (`last_kernel`),
so a routing change cannot move a case onto another path unseen.

With VALUE_RANGES_REPORT=<file>, the worst ratio per case family and the kernel it ran on are written there as JSON."""
import json
import os

import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import fullsize as fs
from helpers import value_ranges as vr

pytestmark = pytest.mark.gpu

ALIGNED = (32, 40, 64)
RAGGED = (181, 217, 181)
MODES = ("reflect", "nearest", "mirror", "wrap", "grid-wrap", "grid-mirror", "grid-constant", "constant")
CVALS = (-1024.0, -1000.3)            # the second is not a float32 value: the kernels round it
BURST = 24

_REPORT = {}


def _record(family, ratio, kernel):
    worst = _REPORT.get(family)
    if worst is None or ratio > worst[0]:
        _REPORT[family] = (float(ratio), kernel)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("VALUE_RANGES_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            json.dump({k: {"ratio": v[0], "kernel": v[1]} for k, v in sorted(_REPORT.items())}, f, indent=1)


@pytest.fixture(scope="module")
def ndi(gpu):
    from cupyimg_amd.scipy import ndimage
    return ndimage


@pytest.fixture(scope="module")
def sentinel(gpu, ndi):
    """A call whose note no case expects: run before every case, so a path that leaves no note of its own fails the
    kernel assertion instead of passing on the previous case's note."""
    b = gpu.asarray(np.ones((64, 64, 64), bool))

    def run():
        ndi.binary_erosion(b, iterations=3)
        assert "bitmorph3_kernel" in gpu.last_kernel(), gpu.last_kernel()
    return run


# What the sentinel leaves: the call that follows it ran a path that records no kernel of its own -- the generic
# per-axis passes (mi_correlate1d: float64 accumulation), the generic dense gather, and a few launches without a note.
NO_NOTE = "bitmorph3_kernel"


def launch(gpu, sentinel, fn):
    sentinel()
    out = fn()
    return out, gpu.last_kernel()


class Checks:
    """Every case of a test is run and every failed check listed at the end (`done`), instead of stopping at the first."""

    def __init__(self):
        self.failed = []

    def check(self, ok, what):
        if not ok:
            self.failed.append(what)

    def expect(self, kernel, *names, what=None):
        self.check(any(n in kernel for n in names), ("kernel", what, names, kernel))

    def done(self):
        assert not self.failed, "%d failed checks:\n%s" % (len(self.failed), "\n".join(map(repr, self.failed[:40])))


@pytest.fixture
def chk():
    return Checks()


# ---------------------------------------------------------------------------------------------------------------------
# separable float filters
# ---------------------------------------------------------------------------------------------------------------------
def _sep_filters(ndim):
    """name -> (device call(ndi, xd, mode, cval), SciPy float64 op(x, mode, cval), bound(mode, cval) -> (abs_op, c),
    smoothing?)"""
    F = {}
    for size in (3, 5, 7, 9, 13):
        w = vr.box_spec(ndim, size)
        F["uniform%d" % size] = (lambda d, a, m, cv, s=size: d.uniform_filter(a, s, mode=m, cval=cv),
                                 lambda a, m, cv, w=w: _direct(a, w, m, cv),
                                 lambda m, cv, w=w: (vr.abs_separable(w, m, cv), vr.sep_c(w)), True)
    sigmas = [1.0, 1.5, 2.0] + ([(1.0, 2.0, 2.0)] if ndim == 3 else [(1.0, 2.0)])
    for sg in sigmas:
        w = vr.gaussian_spec(ndim, sg)
        F["gauss_s%s" % (sg,)] = (lambda d, a, m, cv, s=sg: d.gaussian_filter(a, s, mode=m, cval=cv),
                                  lambda a, m, cv, s=sg: sndi.gaussian_filter(a, s, mode=m, cval=cv),
                                  lambda m, cv, w=w: (vr.abs_separable(w, m, cv), vr.sep_c(w)), True)
    orders = [(0, 0, 1), (0, 2, 0), (1, 0, 2)] if ndim == 3 else [(0, 1), (2, 0), (1, 2)]
    for od in orders:
        w = vr.gaussian_spec(ndim, 1.5, od)
        F["gauss_o%s" % "".join(map(str, od))] = (
            lambda d, a, m, cv, o=od: d.gaussian_filter(a, 1.5, o, mode=m, cval=cv),
            lambda a, m, cv, o=od: sndi.gaussian_filter(a, 1.5, o, mode=m, cval=cv),
            lambda m, cv, w=w: (vr.abs_separable(w, m, cv), vr.sep_c(w)), False)
    for name, sm in (("sobel", [1, 2, 1]), ("prewitt", [1, 1, 1])):
        for ax in range(ndim):
            w = vr.deriv_spec(ndim, ax, sm)
            F["%s%d" % (name, ax)] = (lambda d, a, m, cv, n=name, x=ax: getattr(d, n)(a, x, mode=m, cval=cv),
                                      lambda a, m, cv, n=name, x=ax: getattr(sndi, n)(a, x, mode=m, cval=cv),
                                      lambda m, cv, w=w, x=ax: (vr.abs_separable(w, m, cv, vr.deriv_order(ndim, x)), vr.sep_c(w)),
                                      False)
    F["ggm"] = (lambda d, a, m, cv: d.gaussian_gradient_magnitude(a, 1.5, mode=m, cval=cv),
                lambda a, m, cv: sndi.gaussian_gradient_magnitude(a, 1.5, mode=m, cval=cv),
                lambda m, cv: vr.ggm_bound(ndim, 1.5, m, cv), False)
    F["glaplace"] = (lambda d, a, m, cv: d.gaussian_laplace(a, 1.5, mode=m, cval=cv),
                     lambda a, m, cv: sndi.gaussian_laplace(a, 1.5, mode=m, cval=cv),
                     lambda m, cv: vr.glaplace_bound(ndim, 1.5, m, cv), False)
    return F


def _direct(a, w, mode, cval):
    """A separable filter as direct float64 sums (correlate1d per axis): SciPy's float64 uniform_filter keeps a running
    sum, whose rounding (~1e-14 relative) is not small against the float64 kernels' bound."""
    out = a
    for ax, wa in enumerate(w):
        if wa is not None:
            out = sndi.correlate1d(out, wa, ax, output=np.float64, mode=mode, cval=cval)
    return out


SEP3 = _sep_filters(3)
SEP2 = _sep_filters(2)
FUSED = ("sep3d_", "stream_pass_kernel")
SMOOTHING = ("uniform", "gauss_s")


CONSTANT = ("constant", "grid-constant")


def sep_route(name, mode):
    """The route a float32 volume filter takes: the fused kernels, except derivative filters (sobel, prewitt, Gaussian
    derivatives and what is built from them) in a constant mode, which run the generic float64-accumulating passes."""
    return (NO_NOTE,) if mode in CONSTANT and not name.startswith(SMOOTHING) else FUSED


def _check_sep(chk, gpu, ndi, sentinel, family, F, name, x, xd, mode, cval, kernels, u=vr.U32):
    call, op, bound, smoothing = F[name]
    got, k = launch(gpu, sentinel, lambda: call(ndi, xd, mode, cval))
    chk.expect(k, *kernels(name, mode), what=(family, name, mode, x.shape))
    got = got.get()
    assert got.dtype == x.dtype
    abs_op, c = bound(mode, cval)
    x64 = x.astype(np.float64)
    ref = op(x64, mode, cval)
    r, at = vr.ratio_of(got, ref, abs_op(np.abs(x64)), c, u)
    _record(family, r, k)
    chk.check(r <= 1.0, (family, name, mode, cval, r, at, got[at], ref[at], k))
    if smoothing and u == vr.U32:
        e = fs.maxnorm_rel(got, ref)
        chk.check(e <= 1e-6, (family, name, mode, cval, e, k))


def _gens_f32(shape):
    return {"ct_hu": vr.ct_hu(shape, seed=1, dtype=np.float32), "mr_u12": vr.mr_u12(shape, seed=2, dtype=np.float32),
            "offset_1e4": vr.offset_1e4(shape, seed=3)}


@pytest.mark.parametrize("gen", ["ct_hu", "mr_u12", "offset_1e4"])
def test_separable_f32_aligned(gpu, ndi, sentinel, chk, gen):
    """Every filter on an aligned volume, `reflect` and `constant` with a fill that is not a float32 value."""
    x = _gens_f32(ALIGNED)[gen]
    xd = gpu.asarray(x)
    for name in SEP3:
        for mode, cval in (("reflect", 0.0), ("constant", -1000.3)):
            _check_sep(chk, gpu, ndi, sentinel, "sep3d_f32 aligned", SEP3, name, x, xd, mode, cval, sep_route)
    chk.done()


@pytest.mark.parametrize("gen", ["ct_hu", "offset_1e4"])
def test_separable_f32_every_mode(gpu, ndi, sentinel, chk, gen):
    x = _gens_f32(ALIGNED)[gen]
    xd = gpu.asarray(x)
    for name in ("uniform5", "uniform13", "gauss_s1.5", "gauss_o001", "gauss_o020", "sobel2", "prewitt0"):
        for mode in MODES:
            for cval in (CVALS if mode == "constant" else (0.0,)):
                _check_sep(chk, gpu, ndi, sentinel, "sep3d_f32 modes", SEP3, name, x, xd, mode, cval, sep_route)
    chk.done()


def test_separable_f32_ragged(gpu, ndi, sentinel, chk):
    """181 x 217 x 181: the 3 / 5 / 7-tap kernel takes the rows as they are (direct route); longer kernels run on rows
    extended to 16 bytes (extended-rows route)."""
    x = vr.ct_hu(RAGGED, seed=4, dtype=np.float32)
    xd = gpu.asarray(x)
    cases = [("uniform5", "ragged direct"), ("sobel2", "ragged direct"), ("uniform9", "ragged extended"),
             ("gauss_s1.5", "ragged extended"), ("gauss_o001", "ragged extended")]
    for name, family in cases:
        call, op, bound, smoothing = SEP3[name]
        for mode, cval in (("mirror", 0.0), ("constant", -1000.3)):
            got, k = launch(gpu, sentinel, lambda: call(ndi, xd, mode, cval))
            chk.expect(k, *sep_route(name, mode), what=(name, mode))
            got = got.get()
            abs_op, c = bound(mode, cval)
            h = 8
            r, at = vr.whole_volume_bound(x, got, h, h, lambda a: op(a, mode, cval), abs_op, c, planes=16)
            _record("sep3d_f32 " + family, r, k)
            chk.check(r <= 1.0, (name, mode, r, at, k))
    chk.done()


def test_separable_f32_misaligned_view(gpu, ndi, sentinel, chk):
    """A contiguous view 4 bytes into its allocation with rows of 61 floats: the padded-rows route."""
    shape = (30, 40, 61)
    x = vr.ct_hu(shape, seed=5, dtype=np.float32)
    buf = gpu.asarray(np.concatenate([[np.float32(0)], x.ravel()]))
    xd = buf[1:].reshape(shape)
    assert xd.ptr % 16 != 0
    for name in ("uniform5", "gauss_s1.5", "gauss_o020", "sobel1"):
        for mode, cval in (("mirror", 0.0), ("constant", -1024.0), ("constant", -1000.3)):
            _check_sep(chk, gpu, ndi, sentinel, "sep3d_f32 misaligned", SEP3, name, x, xd, mode, cval, sep_route)
    chk.done()


def _image_route(name, mode):
    """Images: the streaming launches take kernels of up to 9 taps; longer ones run the generic passes."""
    long = name in ("uniform13", "gauss_s1.5", "gauss_s2.0", "gauss_s(1.0, 2.0)", "ggm", "glaplace") or name.startswith("gauss_o")
    return (NO_NOTE,) if long else sep_route(name, mode)


@pytest.mark.parametrize("gen", ["ct_hu", "offset_1e4"])
def test_separable_f32_images(gpu, ndi, sentinel, chk, gen):
    shape = (200, 264)
    x = {"ct_hu": vr.ct_hu(shape, seed=6, dtype=np.float32), "offset_1e4": vr.offset_1e4(shape, seed=7)}[gen]
    xd = gpu.asarray(x)
    for name in SEP2:
        for mode, cval in (("reflect", 0.0), ("wrap", 0.0), ("constant", -1000.3)):
            _check_sep(chk, gpu, ndi, sentinel, "sep3d_f32 image", SEP2, name, x, xd, mode, cval, _image_route)
    chk.done()


@pytest.mark.parametrize("gen", ["ct_hu", "offset_1e4"])
def test_separable_f64(gpu, ndi, sentinel, chk, gen):
    """float64 volumes (mi_separable3d_f64), u = 2^-53; rows of an odd number of doubles included."""
    for shape in (ALIGNED, (24, 30, 45)):
        x = (vr.ct_hu(shape, seed=8, dtype=np.float32) if gen == "ct_hu" else vr.offset_1e4(shape, seed=9)).astype(np.float64)
        xd = gpu.asarray(x)
        for name in ("uniform5", "gauss_s1.5", "gauss_o001", "sobel0", "prewitt2"):
            for mode, cval in (("reflect", 0.0), ("constant", -1000.3)):
                _check_sep(chk, gpu, ndi, sentinel, "separable f64", SEP3, name, x, xd, mode, cval,
                           lambda n, m: (NO_NOTE,) if shape[2] % 2 or NO_NOTE in sep_route(n, m) else ("stream_pass_f64_kernel",),
                           u=vr.U64)
    chk.done()


def test_plane_restricted_ct(gpu, ndi, sentinel, chk):
    """S.output_planes: the planes asked for meet the bound, the others are not written."""
    from cupyimg_amd.scipy.ndimage import _support as S
    x = vr.ct_hu((48, 40, 64), seed=10, dtype=np.float32)
    xd = gpu.asarray(x)
    fill = np.float32(-12345.0)
    for name in ("uniform5", "gauss_s1.5", "gauss_o001", "sobel0"):
        call, op, bound, _ = SEP3[name]
        for mode, cval in (("reflect", 0.0), ("constant", -1000.3)):
            out = gpu.asarray(np.full(x.shape, fill, np.float32))

            def run():
                with S.output_planes([(0, 5), (30, 48)]):
                    if name.startswith("uniform"):
                        ndi.uniform_filter(xd, 5, mode=mode, cval=cval, output=out)
                    elif name.startswith("sobel"):
                        ndi.sobel(xd, 0, mode=mode, cval=cval, output=out)
                    else:
                        ndi.gaussian_filter(xd, 1.5, order=(0, 0, 1) if name == "gauss_o001" else 0, mode=mode, cval=cval,
                                            output=out)
                return out
            if mode in CONSTANT and not name.startswith(SMOOTHING):
                # the fused kernels leave a derivative with a fill value to the generic passes, which cannot be
                # restricted to planes: refused, nothing written
                with pytest.raises(S.Unsupported):
                    run()
                assert np.all(out.get() == fill)
                continue
            got, k = launch(gpu, sentinel, run)
            chk.expect(k, "sep3d_")
            got = got.get()
            assert np.all(got[5:30] == fill)
            abs_op, c = bound(mode, cval)
            x64 = x.astype(np.float64)
            ref, B = op(x64, mode, cval), abs_op(np.abs(x64))
            sel = np.r_[0:5, 30:48]
            r, at = vr.ratio_of(got[sel], ref[sel], B[sel], c)
            _record("sep3d_f32 planes", r, k)
            chk.check(r <= 1.0, (name, mode, r, at, k))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# dense correlate
# ---------------------------------------------------------------------------------------------------------------------
def _laplace_cross(ndim):
    w = np.zeros((3,) * ndim)
    w[(1,) * ndim] = -2.0 * ndim
    for ax in range(ndim):
        for d in (0, 2):
            i = [1] * ndim
            i[ax] = d
            w[tuple(i)] = 1.0
    return w


@pytest.mark.parametrize("gen", ["ct_hu", "mr_u12", "offset_1e4"])
def test_dense_correlate(gpu, ndi, sentinel, chk, gen):
    """3^3 and 5^3 zero-sum weights (a 3-D Sobel kernel, a sampled LoG) and a dense 3^3 one: the default mode stays
    bit-identical to SciPy float32 (float64 accumulation), the float mode (float32 accumulation) meets the bound;
    aligned rows and rows of 61 floats."""
    rng = np.random.default_rng(12)
    weights = {"sobel3d": vr.sobel3d(), "log5": vr.log3d(5, 1.0), "dense3": rng.standard_normal((3, 3, 3))}
    for shape in (ALIGNED, (30, 40, 61)):
        x = _gens_f32(shape)[gen]
        xd = gpu.asarray(x)
        x64 = x.astype(np.float64)
        for wn, w in weights.items():
            for mode, cval in (("reflect", 0.0), ("wrap", 0.0), ("constant", -1000.3)):
                got, k = launch(gpu, sentinel, lambda: ndi.correlate(xd, w, mode=mode, cval=cval))
                chk.expect(k, *(("stencil3",) if mode != "constant" else (NO_NOTE,)), what=(wn, shape, mode, "default"))
                chk.check(np.array_equal(got.get(), sndi.correlate(x, w, mode=mode, cval=cval)), (wn, shape, mode, k))
                _record("correlate default (bit-exact)", 0.0, k)
                got, k = launch(gpu, sentinel, lambda: ndi.correlate(xd, w, mode=mode, cval=cval, dtype_mode="float"))
                chk.expect(k, *(("stencil3",) if mode != "constant" else (NO_NOTE,)), what=(wn, shape, mode, "float"))
                ref = sndi.correlate(x64, w, mode=mode, cval=cval)
                r, at = vr.ratio_of(got.get(), ref, vr.abs_dense(w, mode, cval)(np.abs(x64)), vr.dense_c(w))
                _record("correlate float mode", r, k)
                chk.check(r <= 1.0, (wn, shape, mode, r, at, k))
        # laplace on float32: one 7-point stencil through correlate
        cross = _laplace_cross(3)
        for mode, cval in (("reflect", 0.0), ("constant", -1000.3)):
            got, k = launch(gpu, sentinel, lambda: ndi.laplace(xd, mode=mode, cval=cval))
            chk.expect(k, *(("stencil3",) if mode != "constant" else (NO_NOTE,)), what=("laplace", shape, mode))
            got = got.get()
            chk.check(np.array_equal(got, sndi.correlate(x, cross, mode=mode, cval=cval)), (shape, mode, k))
            r, at = vr.bound_ratio(got, x, lambda a: sndi.laplace(a, mode=mode, cval=cval), vr.abs_dense(cross, mode, cval),
                                   vr.dense_c(cross))
            _record("laplace", r, k)
            chk.check(r <= 1.0, (shape, mode, r, at, k))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# interpolation
# ---------------------------------------------------------------------------------------------------------------------
def _m30():
    a = np.deg2rad(30.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return R @ np.diag([1.0, 0.97, 1.03])


def _centred(M, shape, extra=(0.5, -1.25, 2.0)):
    ctr = (np.asarray(shape, np.float64) - 1) / 2.0
    return ctr - M @ ctr + np.asarray(extra)


def _coef64(x64, order, mode, axes=None):
    if order < 2:
        return x64
    out = x64
    for ax in (range(x64.ndim) if axes is None else axes):
        out = sndi.spline_filter1d(out, order, ax, output=np.float64, mode=mode)
    return out


def _affine_coords(M, off, shape):
    idx = np.indices(shape, dtype=np.float64).reshape(len(shape), -1)
    return (M @ idx + np.asarray(off, np.float64)[:, None]).reshape((len(shape),) + tuple(shape))


def _rotate_coords(in_shape, out_shape, angle):
    """Input coordinates of SciPy's rotate(axes=(1, 0)): every (z, y) plane rotated about its centre (the x index
    is carried through exactly)."""
    a = np.deg2rad(angle)
    R = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
    in_c = (np.asarray(in_shape[:2], np.float64) - 1) / 2
    off = in_c - R @ ((np.asarray(out_shape[:2], np.float64) - 1) / 2)
    idx = np.indices(out_shape, dtype=np.float64)
    zy = np.tensordot(R, idx[:2], axes=1) + off[:, None, None, None]
    return np.concatenate([zy, idx[2:]], axis=0)


def _diag_coords(in_shape, out_shape, shift):
    """zoom (shift None: corners onto corners) or shift: the input coordinates along every axis."""
    idx = np.indices(out_shape, dtype=np.float64)
    for a in range(len(out_shape)):
        if shift is None:
            idx[a] *= (in_shape[a] - 1) / max(out_shape[a] - 1, 1)
        else:
            idx[a] -= shift[a]
    return idx


INTERP_SHAPES = [(128, 128, 128), (45, 54, 45)]


@pytest.mark.parametrize("gen", ["ct_hu", "mr_u12"])
@pytest.mark.parametrize("shape", INTERP_SHAPES, ids=["128", "ragged"])
def test_affine_and_map_coordinates(gpu, ndi, sentinel, chk, gen, shape):
    x = vr.ct_hu(shape, seed=13, dtype=np.float32) if gen == "ct_hu" else vr.mr_u12(shape, seed=14, dtype=np.float32)
    xd = gpu.asarray(x)
    x64 = x.astype(np.float64)
    Mb, _ = fs.affine_case(shape[0])
    for mname, M in (("baseline", Mb), ("general30", _m30())):
        off = _centred(M, shape)
        for order in (1, 3):
            for mode in ("constant", "mirror"):
                got, k = launch(gpu, sentinel, lambda: ndi.affine_transform(xd, M, off, order=order, mode=mode))
                chk.expect(k, "affine3d", "cubic", what=(mname, order, mode, shape))
                ref = sndi.affine_transform(x64, M, off, order=order, mode=mode, output=np.float64)
                coef = _coef64(x64, order, mode)
                B = sndi.affine_transform(np.abs(coef), M, off, order=order, mode=mode, output=np.float64, prefilter=False)
                T = vr.coord_term(coef, _affine_coords(M, off, shape), order, mode)
                r, at = vr.ratio_of(got.get(), ref, B, vr.interp_c(3, order), extra=T)
                _record("affine order %d" % order, r, k)
                chk.check(r <= 1.0, (mname, order, mode, r, at, k))
    # map_coordinates with the general matrix materialised as float32 coordinates
    M = _m30()
    off = _centred(M, shape)
    idx = np.indices(shape, dtype=np.float64).reshape(3, -1)
    coords = (M @ idx + off[:, None]).astype(np.float32).reshape((3,) + shape)
    cd = gpu.asarray(coords)
    for order in (1, 3):
        got, k = launch(gpu, sentinel, lambda: ndi.map_coordinates(xd, cd, order=order, mode="constant"))
        chk.expect(k, *((NO_NOTE,) if order == 1 and shape != INTERP_SHAPES[0] else ("map_coords", "cubic")),
                   what=("map", order, shape))
        c64 = coords.astype(np.float64)
        ref = sndi.map_coordinates(x64, c64, order=order, mode="constant", output=np.float64)
        coef = _coef64(x64, order, "constant")
        B = sndi.map_coordinates(np.abs(coef), c64, order=order, mode="constant", output=np.float64, prefilter=False)
        r, at = vr.ratio_of(got.get(), ref, B, vr.interp_c(3, order), extra=vr.coord_term(coef, c64, order))
        _record("map_coordinates order %d" % order, r, k)
        chk.check(r <= 1.0, (order, r, at, k))
    chk.done()


@pytest.mark.parametrize("gen", ["ct_hu", "mr_u12"])
def test_rotate_zoom_shift_spline_filter(gpu, ndi, sentinel, chk, gen):
    """Every default (order 3, mode `constant`) on 128^3 and a ragged shape; spline_filter with a float32 output."""
    for shape in INTERP_SHAPES:
        x = vr.ct_hu(shape, seed=15, dtype=np.float32) if gen == "ct_hu" else vr.mr_u12(shape, seed=16, dtype=np.float32)
        xd = gpu.asarray(x)
        x64 = x.astype(np.float64)
        # rotate, axes (1, 0): a 2-D transform of every (z, y) plane
        got, k = launch(gpu, sentinel, lambda: ndi.rotate(xd, 30.0))
        chk.expect(k, "cubic", what=("rotate", shape))
        ref = sndi.rotate(x64, 30.0, output=np.float64)
        coef2 = _coef64(x64, 3, "constant", axes=(0, 1))
        B = sndi.rotate(np.abs(coef2), 30.0, output=np.float64, prefilter=False)
        T = vr.coord_term(coef2, _rotate_coords(shape, ref.shape, 30.0), 3, axes=(0, 1))
        r, at = vr.ratio_of(got.get(), ref, B, vr.interp_c(2, 3), extra=T)
        _record("rotate", r, k)
        chk.check(r <= 1.0, (shape, r, at, k))
        coef = _coef64(x64, 3, "constant")
        sh = np.array([0.3, -1.6, 2.25])
        for what, call, op, coords in (
                ("zoom", lambda: ndi.zoom(xd, 1.3), lambda a, **kw: sndi.zoom(a, 1.3, output=np.float64, **kw),
                 lambda out_shape: _diag_coords(shape, out_shape, None)),
                ("shift", lambda: ndi.shift(xd, tuple(sh)), lambda a, **kw: sndi.shift(a, tuple(sh), output=np.float64, **kw),
                 lambda out_shape: _diag_coords(shape, out_shape, sh))):
            got, k = launch(gpu, sentinel, call)
            chk.expect(k, *(("cubic", "spline") if shape == INTERP_SHAPES[0] else (NO_NOTE,)), what=(what, shape))
            ref = op(x64)
            T = vr.coord_term(coef, coords(ref.shape), 3)
            r, at = vr.ratio_of(got.get(), ref, op(np.abs(coef), prefilter=False), vr.interp_c(3, 3), extra=T)
            _record(what, r, k)
            chk.check(r <= 1.0, (what, shape, r, at, k))
        # the prefilter on its own: B from the absolute impulse response of the two-pole filter, per axis
        got, k = launch(gpu, sentinel, lambda: ndi.spline_filter(xd, 3, output=np.float32))
        chk.expect(k, *(("spline",) if shape == INTERP_SHAPES[0] else (NO_NOTE,)), what=("spline_filter", shape))
        ref = sndi.spline_filter(x64, 3, output=np.float64)
        z = np.sqrt(3.0) - 2.0
        h = np.sqrt(3.0) * np.abs(z) ** np.abs(np.arange(-40, 41))
        B = vr.abs_separable([h, h, h], "mirror")(np.abs(x64))
        r, at = vr.ratio_of(got.get(), ref, B, 1.0 + 4 * 3)
        _record("spline_filter f32", r, k)
        chk.check(r <= 1.0, (shape, r, at, k))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# integers: bit-exact
# ---------------------------------------------------------------------------------------------------------------------
def _int_gens(shape):
    return {"ct_hu_i16": vr.ct_hu(shape, seed=17), "mr_u12_u16": vr.mr_u12(shape, seed=18),
            "extremes_i16": vr.int_extremes(shape, np.int16, seed=19), "extremes_u16": vr.int_extremes(shape, np.uint16, seed=20)}


@pytest.mark.parametrize("shape", [(24, 40, 64), (24, 40, 61)], ids=["aligned", "ragged"])
def test_integer_rank_minmax_uniform(gpu, ndi, sentinel, chk, shape):
    ragged = shape[2] % 8 != 0          # rows of 61 16-bit samples: not a multiple of 16 bytes
    for gname, x in _int_gens(shape).items():
        xd = gpu.asarray(x)
        lo = int(np.iinfo(x.dtype).min)
        # 3 x 3 x 3 median / rank / percentile
        for what, call, ref in (
                ("median", lambda m: ndi.median_filter(xd, 3, mode=m), lambda m: sndi.median_filter(x, 3, mode=m)),
                ("rank", lambda m: ndi.rank_filter(xd, 5, 3, mode=m), lambda m: sndi.rank_filter(x, 5, 3, mode=m)),
                ("percentile", lambda m: ndi.percentile_filter(xd, 80, 3, mode=m),
                 lambda m: sndi.percentile_filter(x, 80, 3, mode=m))):
            for mode in ("reflect", "nearest", "wrap"):
                got, k = launch(gpu, sentinel, lambda: call(mode))
                chk.expect(k, "median27_stream_kernel")
                chk.check(np.array_equal(got.get(), ref(mode)), (gname, what, mode, k))
                _record("rank 3x3x3 (bit-exact)", 0.0, k)
        # flat min / max and grey morphology
        for size in (3, 5, (3, 5, 7)):
            for mode, cval in (("reflect", 0.0), ("constant", float(lo)), ("mirror", 0.0)):
                for fn, rf in ((ndi.minimum_filter, sndi.minimum_filter), (ndi.maximum_filter, sndi.maximum_filter)):
                    got, k = launch(gpu, sentinel, lambda: fn(xd, size, mode=mode, cval=cval))
                    chk.expect(k, *(("mm3s16_ragged_kernel",) if ragged and np.isscalar(size) else (NO_NOTE,)),
                               what=(gname, size, mode, shape))
                    chk.check(np.array_equal(got.get(), rf(x, size, mode=mode, cval=cval)), (gname, size, mode, k))
                    _record("min/max 16-bit (bit-exact) " + ("ragged" if shape[2] % 8 else "aligned"), 0.0, k)
        for fn, rf in ((ndi.grey_erosion, sndi.grey_erosion), (ndi.grey_dilation, sndi.grey_dilation)):
            for size in (3, (5, 3, 7)):
                got, k = launch(gpu, sentinel, lambda: fn(xd, size=size))
                chk.expect(k, *(("mm3s16_ragged_kernel",) if ragged and np.isscalar(size) else (NO_NOTE,)),
                           what=(gname, fn.__name__, size, shape))
                chk.check(np.array_equal(got.get(), rf(x, size=size)), (gname, fn.__name__, size, k))
                _record("grey morphology 16-bit (bit-exact)", 0.0, k)
        # integer box filter: sums of either sign, exact multiples, at full range
        for size in (3, 5, 9, (3, 5, 7), (1, 9, 9)):
            for mode, cval in (("reflect", 0.0), ("wrap", 0.0), ("nearest", 0.0), ("constant", float(lo))):
                got, k = launch(gpu, sentinel, lambda: ndi.uniform_filter(xd, size, mode=mode, cval=cval))
                chk.expect(k, "box2d_16_kernel")
                chk.check(np.array_equal(got.get(), sndi.uniform_filter(x, size, mode=mode, cval=cval)), (gname, size, mode, k))
                _record("uniform 16-bit (bit-exact)", 0.0, k)
    chk.done()


def test_integer_uniform_exact_multiples_and_negative_sums(gpu, ndi, sentinel, chk):
    """Windows whose sums are exact multiples of the window (constant runs at iinfo.min / max, +-1 around them) and
    negative sums that must truncate toward zero, at full range: the 0.02 offset of div_trunc."""
    rng = np.random.default_rng(21)
    for dt in (np.int16, np.uint16):
        info = np.iinfo(dt)
        base = np.array([info.min, info.max, info.min + 1, info.max - 1, -1 if dt == np.int16 else 1, 0], np.int64)
        x = base[rng.integers(0, len(base), size=(16, 24, 64))]
        x[:, :, 8:24] = info.max
        x[:, 4:10, :] = info.min
        x[3:6, :, 30:40] = rng.integers(info.min, info.max + 1, size=(3, 24, 10))
        x = x.astype(dt)
        xd = gpu.asarray(x)
        for size in (3, 5, 7, 9, (3, 9, 5)):
            for mode in ("reflect", "constant"):
                cval = float(info.max) if mode == "constant" else 0.0
                got, k = launch(gpu, sentinel, lambda: ndi.uniform_filter(xd, size, mode=mode, cval=cval))
                chk.expect(k, "box2d_16_kernel")
                chk.check(np.array_equal(got.get(), sndi.uniform_filter(x, size, mode=mode, cval=cval)), (dt, size, mode, k))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# full size: every plane, the last of a burst
# ---------------------------------------------------------------------------------------------------------------------
def burst(fn):
    out = fn(None)
    for _ in range(BURST - 1):
        fn(out)
    return out


@pytest.fixture(scope="module")
def ct512(gpu):
    x = vr.ct_hu((fs.N_H,) * 3, seed=22, dtype=np.float32)
    xd = gpu.asarray(x)
    yield x, xd
    del xd
    gpu.free_all_blocks()


def test_full_H_uniform5_ct512(gpu, ndi, sentinel, chk, ct512):
    x, xd = ct512
    sentinel()
    out = burst(lambda o: ndi.uniform_filter(xd, size=5, output=o))
    k = gpu.last_kernel()
    chk.expect(k, "sep3d_long3_kernel<5,")
    out = out.get()
    w = vr.box_spec(3, 5)
    op = lambda a: sndi.uniform_filter(a, 5)              # noqa: E731
    r, at = vr.whole_volume_bound(x, out, 2, 2, op, vr.abs_separable(w), vr.sep_c(w))
    _record("full H uniform5 ct_hu 512^3", r, k)
    chk.check(r <= 1.0, (r, at))
    err = fs.whole_volume_filter(x, out, 2, 2, lambda s: sndi.uniform_filter(s.astype(np.float64), size=5))
    assert err <= 1e-6, err
    chk.done()


def test_full_B_gaussian2_ct512(gpu, ndi, sentinel, chk, ct512):
    x, xd = ct512
    sentinel()
    out = burst(lambda o: ndi.gaussian_filter(xd, sigma=2, output=o))
    k = gpu.last_kernel()
    chk.expect(k, "sep3d_long3_kernel<17,")
    out = out.get()
    w = vr.gaussian_spec(3, 2.0)
    r, at = vr.whole_volume_bound(x, out, 8, 8, lambda a: sndi.gaussian_filter(a, 2.0), vr.abs_separable(w), vr.sep_c(w),
                                  planes=16)
    _record("full B gaussian2 ct_hu 512^3", r, k)
    chk.check(r <= 1.0, (r, at))
    err = fs.whole_volume_filter(x, out, 8, 8, lambda s: sndi.gaussian_filter(s.astype(np.float64), sigma=2), planes=16)
    assert err <= 1e-6, err
    chk.done()


def test_full_ggm_offset_256(gpu, ndi, sentinel, chk):
    x = vr.offset_1e4((256, 256, 256), seed=23)
    xd = gpu.asarray(x)
    sentinel()
    out = burst(lambda o: ndi.gaussian_gradient_magnitude(xd, 1.5, output=o))
    k = gpu.last_kernel()
    chk.expect(k, *FUSED)
    abs_op, c = vr.ggm_bound(3, 1.5)
    r, at = vr.whole_volume_bound(x, out.get(), 6, 6, lambda a: sndi.gaussian_gradient_magnitude(a, 1.5), abs_op, c,
                                  planes=16)
    _record("full ggm offset_1e4 256^3", r, k)
    chk.check(r <= 1.0, (r, at))
    chk.done()

