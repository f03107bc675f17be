"""Integer images through affine_transform, map_coordinates, shift, zoom and rotate on the device, against SciPy's
integer path: every dtype, order and mode, fractional and out-of-range fill values, exact .5 ties of both signs, output
dtypes other than the input's, ranks 1, 2 and 4, unit axes, bool.

The contract, the tie band and the table of cases are those of tests/helpers/int_interp.py, each proved on SciPy alone by
tests/test_int_interp_yardstick.py: a result equals SciPy's at every output, except within the derived band (about 1e-8
on 16-bit data) around a .5 tie of the unrounded value, where it may differ by one; cases built on exact ties have no
band.  A float output is held to the same bound without the rounding."""
import numpy as np
import pytest

from helpers import int_interp as ii

pytestmark = pytest.mark.gpu

BUCKETS = ii.buckets()


@pytest.fixture(scope="module")
def ndi(gpu):
    from cupyimg_amd.scipy import ndimage
    return ndimage


@pytest.mark.parametrize("bucket", sorted(BUCKETS))
def test_equals_scipy(gpu, ndi, bucket):
    failed = []
    for case in BUCKETS[bucket]:
        want = case.scipy()
        got = case.device(gpu, ndi, want.shape)
        try:
            assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
            case.check(got, want)
        except AssertionError as e:
            failed.append((case.id, str(e)))
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(BUCKETS[bucket]), "\n".join(map(repr, failed[:20])))


def test_preallocated_output_is_the_result(gpu, ndi):
    """The array handed in as `output=` is the one returned, and it holds the rounded result."""
    x = ii.data("ct_i16", ii.SMALL)
    M, off = ii.general(ii.SMALL)
    out = gpu.asarray(np.full(ii.SMALL, 7, np.int16))
    ret = ndi.affine_transform(gpu.asarray(x), M, off, output=out, order=1, mode="mirror")
    assert ret is out
    case = next(c for c in ii.table() if c.group == "output" and isinstance(c.output, tuple) and c.order == 1
                and c.kw["mode"] == "mirror")
    case.check(out.get(), case.scipy())
