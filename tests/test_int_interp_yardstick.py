"""The yardstick of tests/test_gpu_int_interp.py, proved on the CPU: for every case of the table in
tests/helpers/int_interp.py, SciPy's integer-path result IS round_like_scipy(unrounded(...)) outside the tie band, the
band excuses no more than the cap, and the case exercises what it is in the table for.  The same table then holds the
CPU oracle (oracle.ndimage) to SciPy under the same comparison."""
import numpy as np
import pytest
import scipy.ndimage as sndi

from helpers import int_interp as ii

BUCKETS = ii.buckets()


@pytest.fixture(scope="module")
def orc():
    from oracle import ndimage as o
    o.build()
    return o


def _tags(case, want, u, failed):
    x = case.x
    dt = case.out_dtype
    if "saturates" in case.tags:
        info = np.iinfo(dt)
        share = float(((want == info.min) & (u < info.min) | (want == info.max) & (u > info.max)).mean())
        if not share > 0.01:
            failed.append((case.id, "saturates in %.4f of the outputs" % share))
    if "ties" in case.tags:
        tie = np.abs(u) % 1.0 == 0.5
        # order 1 at these positions gives multiples of 1/16 (shift), 1/64 (zoom) and 1/8 (the diagonal 0.5): the values are
        # exact in double, so `==` finds every tie
        if not tie.any() or (dt.kind == "i" and not ((tie & (u < 0)).any() and (tie & (u > 0)).any())):
            failed.append((case.id, "ties: %d, negative %d" % (int(tie.sum()), int((tie & (u < 0)).sum()))))
        if "dyadic" in case.tags and not tie.mean() > 0.10:
            failed.append((case.id, "exact ties in %.4f of the outputs" % tie.mean()))
    if "padcast" in case.tags:
        plain = sndi.affine_transform(x.astype(np.float64), *case.host_args(), **dict(case.kw, output=np.float64))
        if dt.kind == "f":
            differs = np.abs(plain - want).max() > 1e-6                 # the 1.4e-5 the other pad value costs
        else:
            differs = (ii.round_like_scipy(plain, dt) != want).any()
        if not differs:
            failed.append((case.id, "the cast pad value changes no output"))


@pytest.mark.parametrize("bucket", sorted(BUCKETS))
def test_scipy_is_the_rounded_unrounded_result_and_the_oracle_equals_it(bucket, orc):
    failed = []
    for case in BUCKETS[bucket]:
        want = case.scipy()
        assert want.dtype == case.out_dtype, (case.id, want.dtype)
        ev = None if case.exact else case.evidence()
        u = ii.unrounded(case.fn, case.x, *case.host_args(), **case.kw) if ev is None else ev[0]
        assert u.shape == want.shape
        for who, got in (("restatement", lambda: ii.round_like_scipy(u, case.out_dtype)),
                         ("oracle", lambda: case.call(orc, case.x, want.shape))):
            if who == "oracle" and not hasattr(orc, case.fn):
                continue                                              # the oracle has no rotate
            try:
                case.check(np.asarray(got()), want, ev)
            except AssertionError as e:
                failed.append((case.id, who, str(e)))
        _tags(case, want, u, failed)
    assert not failed, "%d failed checks:\n%s" % (len(failed), "\n".join(map(repr, failed[:20])))


def test_round_like_scipy_on_ties_and_limits():
    # the largest double below 0.5 rounds to 1: t + 0.5 is 1.0 in double, in SciPy's C as here
    t = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 32767.5, -32768.5, 1e9, -1e9, 0.0])
    assert ii.round_like_scipy(t, np.int16).tolist() == [1, 2, 3, -1, -2, -3, 1, -1, 32767, -32768, 32767, -32768, 0]
    assert ii.round_like_scipy(t, np.uint16).tolist() == [1, 2, 3, 0, 0, 0, 1, 0, 32768, 0, 65535, 0, 0]
    assert ii.round_like_scipy(t, bool).tolist() == [True] * 12 + [False]


def test_compare_excuses_only_the_band():
    want = np.array([3, -4, 10, 7], np.int16)
    u = np.array([2.5 + 1e-9, -3.5 - 1e-9, 10.2, 7.4])
    with pytest.raises(AssertionError, match="excuses"):             # one of four outputs: beyond the cap
        ii.compare(want, want, u, 1e-8)
    u = np.concatenate([u, np.full(4000, 7.4)])
    want = np.concatenate([want, np.full(4000, 7, np.int16)])
    got = want.copy()
    got[0] = 2                                                      # a tie inside the band may go either way
    assert ii.compare(got, want, u, 1e-8) == 2
    got[0] = 1
    with pytest.raises(AssertionError, match="more than one"):
        ii.compare(got, want, u, 1e-8)
    got[0], got[2] = 3, 11                                          # no tie there
    with pytest.raises(AssertionError, match="outside the band"):
        ii.compare(got, want, u, 1e-8)
    got[2], got[1] = 10, -3                                         # band 0: exact ties only
    with pytest.raises(AssertionError):
        ii.compare(got, want)


def test_cases_scipy_refuses_still_raise():
    for case in ii.refused_by_scipy():
        with pytest.raises(OverflowError):
            case.scipy()


def test_bool_cases_stay_off_the_half_integers():
    for case in ii.table():
        if case.group == "bool":
            c, _ = ii.positions(case.fn, case.x, case.shape, *case.host_args(), **case.kw)
            assert np.abs(np.abs(c) % 1.0 - 0.5).min() > 1e-6, case.id


def test_band_is_about_1e_8_on_16_bit_data():
    """Derived, not tuned: its size is what the module promises."""
    for case in ii.table():
        if case.group == "dtypes" and case.kind in ("ct_i16", "ext_u16") and case.shape == ii.SMALL and case.order in (1, 3):
            band = case.evidence()[1]
            assert 0 < band.max() < 1e-7, (case.id, band.max())
