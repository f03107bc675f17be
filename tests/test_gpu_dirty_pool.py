"""Every kernel family on poisoned pool memory (tests/helpers/dirty_pool.py): with mi_debug_set_pool_fill on, each output and
each scratch block starts as 0xFF, 0x55 or 0xD5 bytes instead of the zeros of a fresh allocation or the right answer of the
call before.  Per case: the results under the three bytes are identical byte for byte (anything that depends on memory the
call did not write differs), they agree with the family's own reference within the family's own tolerance, and bool outputs
hold nothing but 0 and 1."""
import numpy as np
import pytest

from helpers import dirty_pool as dp

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def test_pool_fill_reaches_fresh_and_recycled_blocks_of_both_size_classes(gpu):
    """below 1 MiB blocks round to 512 B, above to multiples of 2 MiB; sizes no other test of this module asks for, so that the
    first request of each is a fresh block and the one after its release the recycled one"""
    gpu.free_all_blocks()
    for n in (7 * 512 + 13, MIB - 1, MIB + 1, 3 * MIB + 517):
        for byte in dp.FILLS:
            with dp.pool_fill(gpu, byte):
                cached = gpu.pool_stats()["cached"]
                a = gpu.empty((n,), np.uint8)
                fresh = gpu.pool_stats()["cached"] == cached          # nothing came off a free list
                ptr = a.ptr
                assert (a.get() == byte).all(), (n, byte, "fresh" if fresh else "recycled")
                a.fill((byte + 1) & 0xFF)
                del a
                b = gpu.empty((n,), np.uint8)                         # the block just freed (LIFO)
                assert b.ptr == ptr
                assert (b.get() == byte).all(), (n, byte, "recycled")
                b.fill(0x3C)
                del b
            if byte == dp.FILLS[0]:
                assert fresh, n
            # off again: the recycled block keeps what the last owner left in it
            c = gpu.empty((n,), np.uint8)
            assert c.ptr == ptr and (c.get() == 0x3C).all(), (n, byte, "knob off")
            del c
    # the slack of the rounded block is filled too: a request of 1 byte, then one of 512 out of the same block
    with dp.pool_fill(gpu, 0x55):
        gpu.empty((1,), np.uint8)
    d = gpu.empty((512,), np.uint8)
    assert (d.get() == 0x55).all()


@pytest.mark.parametrize("case", dp.CASES, ids=[c.name for c in dp.CASES])
def test_results_do_not_depend_on_what_the_pool_hands_out(gpu, case):
    outs, routes, host = dp.run_filled(gpu, case)
    first = outs[dp.FILLS[0]]
    assert first, "the case produced nothing"
    print("route:", case.name, "|", routes[dp.FILLS[0]])
    for part in (case.route,) if isinstance(case.route, str) else case.route or ():
        for byte in dp.FILLS:
            assert part in routes[byte], (part, hex(byte), routes[byte])
    # 1. bit identity across the fills
    for byte in dp.FILLS[1:]:
        other = outs[byte]
        assert len(other) == len(first)
        for k, (a, b) in enumerate(zip(first, other)):
            assert a.dtype == b.dtype and a.shape == b.shape, (k, hex(byte))
            if a.tobytes() != b.tobytes():
                diff = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)) // max(a.dtype.itemsize, 1)
                at = np.unravel_index(int(diff[0]), a.shape) if a.shape else ()
                raise AssertionError("output {}: {} elements differ between fills 0xff and {:#x}, first at {}: {} / {} ({})".format(
                    k, np.unique(diff).size, byte, at, a[at], b[at], routes[byte]))
    # 3. clean bools
    for k, a in enumerate(first):
        if a.dtype == np.bool_:
            assert a.view(np.uint8).max(initial=0) <= 1, k
    # 2. the family's reference, the family's tolerance
    want = dp.reference(case, host, first)
    assert len(want) == len(first), (len(want), len(first))
    per_output = isinstance(case.compare, (list, tuple))          # one comparison for every output, or one for each
    assert not per_output or len(case.compare) == len(first), (len(case.compare), len(first))
    for k, (g, w) in enumerate(zip(first, want)):
        try:
            (case.compare[k] if per_output else case.compare)(g, w)
        except AssertionError as e:
            raise AssertionError("output {} against the reference ({}): {}".format(k, routes[dp.FILLS[0]], e))
