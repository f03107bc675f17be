"""skimage.restoration.denoise_tv_chambolle (csrc/tv_chambolle.hip) on MRI-sized float32 volumes: one JSON line per shape with
the time of one iteration (hipEvents around a run of iterations queued straight through mi_tv_chambolle_step, warm, median and
spread of the repetitions; an iteration = the iteration kernel plus the one-workgroup energy step) for
  (a) the fused kernel under the planner's tiles,
  (b) the generic one-thread-per-voxel kernel forced through mi_debug_set_tv_chambolle,
  (c) the ceiling: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes a fused iteration must move, 7 volumes'
      worth (image once, 3 components of p read and written) = 3.5 volumes copied,
and the time of a whole call at a fixed iteration count (eps = 0 never stops early).  -> profiles/tv_chambolle.txt

    python scripts/bench_tv_chambolle.py [--reps 5] [--iters 20]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cupyimg_amd as ca  # noqa: E402
from cupyimg_amd import _lib  # noqa: E402
from cupyimg_amd.skimage import restoration as rest  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = ca.Event(), ca.Event()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_ms(b) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def test_volume(shape, seed):
    """a ball plus a step plus Gaussian noise of sigma 0.2"""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij", sparse=True)
    img = (sum(((a - 0.5) / 0.35) ** 2 for a in axes) <= 1.0) + 0.5 * (sum(axes) > 1.5)
    return (img + 0.2 * rng.standard_normal(shape)).astype(np.float32)


def emit(**rec):
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_tv_chambolle
    knob.argtypes = [ctypes.c_int] * 4
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    for shape in ((256, 256, 256), (181, 217, 181)):
        name = "x".join(map(str, shape))
        x = ca.asarray(test_volume(shape, 1))
        n = x.size
        p = [ca.zeros((3, n), np.float32), ca.zeros((3, n), np.float32)]
        work = ca.zeros((64 + 16 * 65536,), np.uint8)
        xd, pd = x._desc(), [p[0]._desc(), p[1]._desc()]

        def iterations():
            # iteration numbers from 1: the stop step compares energies but eps = 0 never stops
            for i in range(1, a.iters + 1):
                _lib.check(lib.mi_tv_chambolle_step(ctypes.byref(xd), ctypes.byref(pd[i & 1]), ctypes.byref(pd[(i + 1) & 1]), 0.1, 0.0,
                                                    i, ctypes.c_void_p(work.ptr), None))

        rec = {"case": "float32 " + name, "iterations_timed": a.iters}
        for label, setting in (("fused", (0, 0, 0, 0)), ("generic", (0, 0, 0, 1))):
            knob(*setting)
            us, spread = timed(iterations, a.reps)
            rec[label + "_us_per_iteration"] = round(us / a.iters, 1)
            rec[label + "_spread_us"] = round(spread / a.iters, 1)
            rec[label + "_kernel"] = ca.last_kernel()
        knob(0, 0, 0, 0)
        # the ceiling: 7 volumes' worth of bytes = a copy of 3.5 volumes between two buffers of their own
        m = (7 * n // 2) // 4 * 4
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        assert m <= src.size and m <= dst.size

        def copies():
            for _ in range(a.iters):
                _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None))

        us, spread = timed(copies, a.reps)
        rec["copy_7_volumes_us"] = round(us / a.iters, 1)
        rec["copy_spread_us"] = round(spread / a.iters, 1)
        rec["copy_TB_per_s"] = round(2 * m * 4 / (us / a.iters) / 1e6, 2)
        rec["fused_over_copy"] = round(rec["fused_us_per_iteration"] / rec["copy_7_volumes_us"], 2)
        rec["generic_over_fused"] = round(rec["generic_us_per_iteration"] / rec["fused_us_per_iteration"], 2)
        rec["fused_not_slower_than_generic"] = bool(rec["fused_us_per_iteration"] <= rec["generic_us_per_iteration"])
        emit(**rec)
        for label, setting in (("fused", (0, 0, 0, 0)), ("generic", (0, 0, 0, 1))):
            knob(*setting)
            us, spread = timed(lambda: rest.denoise_tv_chambolle(x, weight=0.1, eps=0, n_iter_max=50), a.reps)
            emit(case="whole call, 50 iterations, float32 " + name + ", " + label, call_us=round(us, 1), spread_us=round(spread, 1),
                 us_per_iteration=round(us / 50, 1), iterations=rest.last_tv_iterations())
        knob(0, 0, 0, 0)
        us, spread = timed(lambda: rest.denoise_tv_chambolle(x, weight=0.1), a.reps)
        emit(case="whole call, default eps and n_iter_max, float32 " + name, call_us=round(us, 1), spread_us=round(spread, 1),
             stopped_at=rest.last_tv_iterations(), kernel=ca.last_kernel())


if __name__ == "__main__":
    main()
