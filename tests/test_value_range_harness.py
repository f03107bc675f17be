"""The yardstick of tests/test_gpu_value_ranges.py proved on the CPU: SciPy's own float32 results meet the per-voxel bound
|got - ref64| <= c . u . B on every generator of helpers/value_ranges.py, and results with a deliberate mistake in them
(a tap shifted by one, `reflect` computed as `mirror`, cval rounded to float16, one coefficient plane dropped) break it
by at least a factor of ten."""
import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import value_ranges as vr

SHAPE = (20, 24, 28)
M30 = np.array([[1.0, 0.0, 0.0],
                [0.0, np.cos(np.pi / 6), -np.sin(np.pi / 6)],
                [0.0, np.sin(np.pi / 6), np.cos(np.pi / 6)]]) @ np.diag([1.0, 0.97, 1.03])


def _gens():
    return {
        "mr_u12": vr.mr_u12(SHAPE, seed=1, dtype=np.float32),
        "ct_hu": vr.ct_hu(SHAPE, seed=2, dtype=np.float32),
        "offset_1e4": vr.offset_1e4(SHAPE, seed=3),
        "int16_extremes": vr.int_extremes(SHAPE, np.int16, seed=4).astype(np.float32),
    }


GENS = _gens()


def _affine_off(shape, M):
    ctr = (np.asarray(shape) - 1) / 2.0
    return ctr - M @ ctr + np.array([0.3, -0.7, 0.45])


def _filter_cases(ndim=3):
    """(name, f(x, dtype) -> result, op, abs_op, c) of the linear filters."""
    out = []
    for size in (3, 5):
        w = vr.box_spec(ndim, size)
        out.append(("uniform%d" % size, lambda a, dt, s=size: sndi.uniform_filter(a.astype(dt), s),
                    lambda a, s=size: sndi.uniform_filter(a, s), vr.abs_separable(w), vr.sep_c(w)))
    for order in (0, 1, 2, (0, 2, 1)):
        w = vr.gaussian_spec(ndim, 1.5, order)
        out.append(("gauss_o%s" % (order,), lambda a, dt, o=order: sndi.gaussian_filter(a.astype(dt), 1.5, o),
                    lambda a, o=order: sndi.gaussian_filter(a, 1.5, o), vr.abs_separable(w), vr.sep_c(w)))
    for name, fn, sm in (("sobel", sndi.sobel, [1, 2, 1]), ("prewitt", sndi.prewitt, [1, 1, 1])):
        for ax in range(ndim):
            w = vr.deriv_spec(ndim, ax, sm)
            out.append(("%s%d" % (name, ax), lambda a, dt, f=fn, x=ax: f(a.astype(dt), axis=x, mode="constant", cval=-1000.3),
                        lambda a, f=fn, x=ax: f(a, axis=x, mode="constant", cval=-1000.3),
                        vr.abs_separable(w, "constant", -1000.3, vr.deriv_order(ndim, ax)), vr.sep_c(w)))
    cross = np.zeros((3, 3, 3))
    cross[1, 1, 1] = -6.0
    for ax in range(3):
        for d in (0, 2):
            i = [1, 1, 1]
            i[ax] = d
            cross[tuple(i)] = 1.0
    out.append(("laplace", lambda a, dt: sndi.laplace(a.astype(dt)), sndi.laplace, vr.abs_dense(cross), vr.dense_c(cross)))
    k = vr.sobel3d()
    out.append(("correlate_sobel3d", lambda a, dt: sndi.correlate(a.astype(dt), k), lambda a: sndi.correlate(a, k),
                vr.abs_dense(k), vr.dense_c(k)))
    return out


FILTERS = _filter_cases()


@pytest.mark.parametrize("gen", sorted(GENS))
def test_scipy_float32_filters_meet_the_bound(gen):
    x = GENS[gen]
    for name, f, op, abs_op, c in FILTERS:
        r, at = vr.bound_ratio(f(x, np.float32), x, op, abs_op, c)
        assert r <= 1.0, (gen, name, r, at)
        # and float64 against itself (u = 2^-53) -- the bound is not vacuous at double precision either
        r64, _ = vr.bound_ratio(f(x, np.float64), x, op, abs_op, c, vr.U64)
        assert r64 <= 1.0, (gen, name, r64)


@pytest.mark.parametrize("gen", sorted(GENS))
def test_scipy_float32_affine_meets_the_bound(gen):
    x = GENS[gen]
    for M in (np.diag([1.02, 1.0, 1.0]), M30):
        off = _affine_off(x.shape, M)
        for order in (1, 3):
            coef64 = sndi.spline_filter(x.astype(np.float64), order, mode="mirror") if order > 1 else x.astype(np.float64)
            got = sndi.affine_transform(x, M, off, order=order, mode="mirror", output=np.float32)
            ref = sndi.affine_transform(x.astype(np.float64), M, off, order=order, mode="mirror", output=np.float64)
            B = sndi.affine_transform(np.abs(coef64), M, off, order=order, mode="mirror", output=np.float64, prefilter=False)
            r, at = vr.ratio_of(got, ref, B, vr.interp_c(3, order))
            assert r <= 1.0, (gen, order, r, at)


def _shift_tap(w):
    """The kernel with its taps moved one place (the window off by one voxel)."""
    return np.concatenate([[0.0], w[:-1]])


@pytest.mark.parametrize("gen", sorted(GENS))
def test_wrong_results_fail_by_ten(gen):
    x = GENS[gen]
    x64 = x.astype(np.float64)
    worst = {}
    # (1) a tap shifted by one along x: gaussian, uniform, sobel
    for name, w in (("gauss", vr.gaussian_spec(3, 1.5)), ("uniform", vr.box_spec(3, 5)),
                    ("sobel", vr.deriv_spec(3, 2, [1, 2, 1]))):
        bad = list(w[:2]) + [_shift_tap(w[2])]
        got = x64
        for ax, wa in enumerate(bad):
            got = sndi.correlate1d(got, wa, ax, output=np.float64)
        got = got.astype(np.float32)
        worst["shift_" + name] = vr.bound_ratio(got, x, lambda a, w=w: _sep(a, w), vr.abs_separable(w), vr.sep_c(w))[0]
    # (2) reflect computed as mirror
    w = vr.gaussian_spec(3, 1.0)
    got = sndi.gaussian_filter(x, 1.0, mode="mirror")
    worst["mirror_for_reflect"] = vr.bound_ratio(got, x, lambda a: sndi.gaussian_filter(a, 1.0, mode="reflect"),
                                                 vr.abs_separable(w, "reflect"), vr.sep_c(w))[0]
    # (3) cval rounded to float16 (-1000.3 -> -1000.0)
    cv = -1000.3
    got = sndi.gaussian_filter(x, 1.0, mode="constant", cval=float(np.float16(cv)))
    worst["cval_float16"] = vr.bound_ratio(got, x, lambda a: sndi.gaussian_filter(a, 1.0, mode="constant", cval=cv),
                                           vr.abs_separable(w, "constant", cv), vr.sep_c(w))[0]
    # (4) order-3 affine with one plane of coefficients dropped
    M = M30
    off = _affine_off(x.shape, M)
    coef64 = sndi.spline_filter(x64, 3, mode="mirror")
    bad = coef64.copy()
    bad[x.shape[0] // 2] = 0.0
    got = sndi.affine_transform(bad, M, off, order=3, mode="mirror", output=np.float32, prefilter=False)
    ref = sndi.affine_transform(x64, M, off, order=3, mode="mirror", output=np.float64)
    B = sndi.affine_transform(np.abs(coef64), M, off, order=3, mode="mirror", output=np.float64, prefilter=False)
    worst["coef_plane_dropped"] = vr.ratio_of(got, ref, B, vr.interp_c(3, 3))[0]
    for k, r in worst.items():
        assert r >= 10.0, (gen, k, r)


def _sep(a, w):
    out = a
    for ax, wa in enumerate(w):
        if wa is not None:
            out = sndi.correlate1d(out, wa, ax, output=np.float64)
    return out


def test_generators():
    """Ranges, dtypes and determinism of the generators (cheap at 512^3: built block-wise)."""
    m = vr.mr_u12((40, 50, 60), seed=5)
    assert m.dtype == np.uint16 and m.min() >= 0 and m.max() <= 4095 and m.max() > 3000
    assert np.array_equal(vr.mr_u12((40, 50, 60), seed=5, dtype=np.float32), m.astype(np.float32))
    c = vr.ct_hu((40, 50, 60), seed=5)
    assert c.dtype == np.int16 and c.min() == vr.PAD_I16
    inside = c[c != vr.PAD_I16]
    assert inside.min() >= -1024 and inside.max() <= 3071 and inside.max() > 1500 and (inside < -900).any()
    cf = vr.ct_hu((40, 50, 60), seed=5, dtype=np.float32)
    assert cf.min() == vr.PAD_F32 and np.array_equal(cf[c != vr.PAD_I16], inside.astype(np.float32))
    o = vr.offset_1e4((16, 20, 24))
    assert o.dtype == np.float32 and abs(float(o.mean()) - 1e4) < 0.1
    for dt in (np.int16, np.uint16, np.uint8):
        e = vr.int_extremes((16, 20, 24), dt, seed=1)
        info = np.iinfo(dt)
        assert e.dtype == dt and (e == info.min).sum() > 100 and (e == info.max).sum() > 100
    u = vr.int_extremes((16, 20, 24), np.uint16)
    assert ((u == 32767) | (u == 32768)).any()
    assert np.array_equal(vr.ct_hu((33, 20, 24), seed=9)[:17], vr.ct_hu((33, 20, 24), seed=9)[:17])
    img = vr.ct_hu((50, 60), seed=3, dtype=np.float32)
    assert img.shape == (50, 60)
