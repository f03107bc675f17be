"""skimage.segmentation morphological snakes (csrc/morphsnakes.hip) on MRI-sized float32 volumes: one JSON line per shape,
algorithm and smoothing count with the time of one iteration (hipEvents around a run of iterations queued straight through
mi_snake_acwe_step / mi_snake_gac_step, warm, median and spread of the repetitions) for
  (a) the fused route under the planner's boxes,
  (b) the generic route (one stage per launch, one thread per voxel) forced through mi_debug_set_morphsnakes,
  (c) the smoothing of the same iteration composed from this project's public device calls as the reference schedules it:
      per smoothing step 18 ndi.binary_erosion / binary_dilation calls with the nine plane elements, each with its astype(int8).
      The array layer has no maximum, comparison, masked store or gradient, so the two 9-deep stack reductions, the means and
      the update of the reference's iteration are NOT in (c): it is a lower bound of the reference's schedule on this chip,
      and a / c understates what the fused route saves,
  (d) the ceiling: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes a fused iteration must move, 6 per
      voxel (the float32 image once, u read and written) = 0.75 float32 volumes copied,
and the time of a whole 50-iteration call.  -> profiles/morphsnakes.txt

    python scripts/bench_morphsnakes.py [--reps 5] [--iters 10]
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
from cupyimg_amd.scipy import ndimage as ndi  # noqa: E402
from cupyimg_amd.skimage import segmentation as seg  # noqa: E402


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
    """a blob with an edge plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij", sparse=True)
    b = np.exp(-sum(((a - 0.45) / 0.3) ** 2 for a in axes))
    return (0.2 + 0.8 * (b > 0.5) * b + 0.1 * rng.standard_normal(shape)).astype(np.float32)


def plane_elements():
    i = np.arange(3)
    out = [np.zeros((3, 3, 3), np.uint8) for _ in range(9)]
    out[0][:, :, 1] = 1
    out[1][:, 1, :] = 1
    out[2][1, :, :] = 1
    out[3][:, i, i] = 1
    out[4][:, i, 2 - i] = 1
    out[5][i, :, i] = 1
    out[6][i, :, 2 - i] = 1
    out[7][i, i, :] = 1
    out[8][i, 2 - i, :] = 1
    return [ca.asarray(p) for p in out]


def emit(**rec):
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_morphsnakes
    knob.argtypes = [ctypes.c_int] * 2
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    elements = plane_elements()
    for shape in ((256, 256, 256), (181, 217, 181)):
        name = "x".join(map(str, shape))
        x = ca.asarray(test_volume(shape, 1))
        n = x.size
        u = [seg.checkerboard_level_set(shape), ca.zeros(shape, np.int8), ca.zeros(shape, np.int8)]
        work = ca.zeros((64 + 32 * 65536,), np.uint8)
        xd, ud = x._desc(), [v._desc() for v in u]
        _lib.check(lib.mi_snake_acwe_init(ctypes.byref(xd), ctypes.byref(ud[0]), ctypes.c_void_p(work.ptr), None))

        # the ceiling: 6 bytes per voxel = a copy of 0.75 float32 volumes between two buffers of their own
        m = (3 * n // 4) // 4 * 4
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)

        def copies():
            for _ in range(a.iters):
                _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None))

        copy_us, copy_spread = timed(copies, a.reps)

        for smoothing in (1, 3):
            def composed():
                # the reference's smoothing on this project's binary morphology (see (c) above)
                v = u[0]
                for _ in range(a.iters):
                    for _ in range(smoothing):
                        d = [ndi.binary_dilation(v, p).astype(np.int8, copy=False) for p in elements]
                        e = [ndi.binary_erosion(d[0], p).astype(np.int8, copy=False) for p in elements]
                        v = e[0]

            comp_us, comp_spread = timed(composed, a.reps)
            for algo in ("acwe", "gac"):
                def iterations():
                    for i in range(a.iters):
                        src_u, dst_u = ud[i & 1], ud[(i + 1) & 1]
                        if algo == "acwe":
                            _lib.check(lib.mi_snake_acwe_step(ctypes.byref(xd), ctypes.byref(src_u), ctypes.byref(dst_u), ctypes.byref(ud[2]),
                                                              1.0, 1.0, smoothing, (i * smoothing) & 1, ctypes.c_void_p(work.ptr), None))
                        else:
                            _lib.check(lib.mi_snake_gac_step(ctypes.byref(xd), ctypes.byref(src_u), ctypes.byref(dst_u), ctypes.byref(ud[2]),
                                                             0.5, 1, smoothing, (i * smoothing) & 1, None))

                rec = {"case": "{} float32 {} smoothing={}".format(algo, name, smoothing), "iterations_timed": a.iters}
                for label, setting in (("fused", (0, 0)), ("generic", (0, 1))):
                    knob(*setting)
                    u[0].set(seg.checkerboard_level_set(shape).get())
                    us, spread = timed(iterations, a.reps)
                    rec[label + "_us_per_iteration"] = round(us / a.iters, 1)
                    rec[label + "_spread_us"] = round(spread / a.iters, 1)
                    rec[label + "_kernel"] = ca.last_kernel()
                knob(0, 0)
                rec["composed_smoothing_us_per_iteration"] = round(comp_us / a.iters, 1)
                rec["composed_spread_us"] = round(comp_spread / a.iters, 1)
                rec["copy_6_bytes_per_voxel_us"] = round(copy_us / a.iters, 1)
                rec["copy_spread_us"] = round(copy_spread / a.iters, 1)
                rec["copy_TB_per_s"] = round(2 * m * 4 / (copy_us / a.iters) / 1e6, 2)
                rec["fused_over_composed"] = round(rec["fused_us_per_iteration"] / rec["composed_smoothing_us_per_iteration"], 3)
                rec["fused_over_copy"] = round(rec["fused_us_per_iteration"] / rec["copy_6_bytes_per_voxel_us"], 2)
                rec["generic_over_fused"] = round(rec["generic_us_per_iteration"] / rec["fused_us_per_iteration"], 2)
                emit(**rec)
        for algo, fn in (("acwe", lambda: seg.morphological_chan_vese(x, 50, "checkerboard", smoothing=1)),
                         ("gac", lambda: seg.morphological_geodesic_active_contour(x, 50, "disk", smoothing=1, threshold=0.5, balloon=1))):
            us, spread = timed(fn, a.reps)
            emit(case="whole call, 50 iterations, smoothing=1, {} float32 {}".format(algo, name), call_us=round(us, 1),
                 spread_us=round(spread, 1), us_per_iteration=round(us / 50, 1), launches=seg.last_snake_launches())


if __name__ == "__main__":
    main()
