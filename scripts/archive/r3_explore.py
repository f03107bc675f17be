"""Round-3 exploration sweep on the GPU box (not part of the product): copy ceilings, the lean kernel at 3 / 5 / 7 taps,
long-kernel chunking, sustained (60 launches) vs first-burst timings.   python scripts/r3_explore.py [what ...]"""
import ctypes
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cupyimg_amd as ca
from cupyimg_amd import _lib
from cupyimg_amd.scipy import ndimage as ndi

what = set(sys.argv[1:]) or {"copy", "lean", "long"}
lib = _lib.load()
n = 512
x = np.random.default_rng(0).standard_normal((n, n, n), dtype=np.float32)
xd = ca.asarray(x)
out = ca.empty(xd.shape, np.float32)
GB = 8 * xd.size / 1e9


def timeit(fn, reps=60, warm=5):
    for _ in range(warm):
        fn()
    ca.synchronize()
    e0, e1, e2 = ca.Event(), ca.Event(), ca.Event()
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    for _ in range(reps - 5):
        fn()
    e2.record()
    ca.synchronize()
    return e0.elapsed_ms(e1) / 5 * 1e3, e0.elapsed_ms(e2) / reps * 1e3        # first 5, all


def show(tag, t):
    print("%-58s first5 %7.1f us  sustained %7.1f us  %6.0f GB/s (%.3f of 8 TB/s)" % (tag, t[0], t[1], GB / t[1] * 1e6, GB / t[1] * 1e6 / 8000), flush=True)


if "copy" in what:
    lib.mi_debug_copy_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    for blocks in [256, 512, 1024, 2048, 4096, 8192, 16384, 65536]:
        show("copy_f4 blocks=%d" % blocks, timeit(lambda: lib.mi_debug_copy_f32(xd.ptr, out.ptr, xd.size, blocks, None)))
    def mc():
        out[...] = xd
    show("hipMemcpy d2d", timeit(mc))
    time.sleep(1)

if "lean" in what:
    lib.mi_debug_set_sep3d_long(1)        # the lean kernel also where the long kernel would be taken
    for size in (5, 3, 7):
        show("lean size=%d" % size, timeit(lambda: ndi.uniform_filter(xd, size=size, output=out)))
        time.sleep(0.3)
    lib.mi_debug_set_sep3d_long(0)

if "long" in what:
    for sigma, zch in [(2.0, 0), (2.0, 2), (2.0, 8), (1.0, 0), (1.5, 0)]:
        lib.mi_debug_set_long_zchunks(zch)
        show("gaussian sigma=%g long zchunks=%d" % (sigma, zch), timeit(lambda: ndi.gaussian_filter(xd, sigma, output=out), reps=40))
        time.sleep(0.5)
    lib.mi_debug_set_long_zchunks(0)
    for size in (9, 13, 17):
        show("uniform size=%d" % size, timeit(lambda: ndi.uniform_filter(xd, size=size, output=out), reps=40))
        time.sleep(0.5)
