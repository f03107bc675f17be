"""skimage.exposure (csrc/exposure.hip) on MRI-sized volumes: one JSON line per case with the time of a whole call (hipEvents
around the call, warm, median and spread of the repetitions) of
  (a) equalize_adapthist with its defaults (kernel = shape // 8, clip_limit 0.01, 256 bins) under the planner's route,
  (b) the same call with the blend forced onto the one-thread-per-voxel kernel (mi_debug_set_clahe(1, 0)),
  (c) equalize_hist with its defaults,
  (d) the ceiling of (a): the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes the three launches must move --
      the image read twice (mappings, blend), the uint16 result written and read, the float64 result written:
      2 * itemsize + 12 bytes per voxel, copied as half that many bytes between two buffers,
on 512^3 float32 and 181 x 217 x 181 uint16.  The min / max reduction of the input that precedes the three launches is part
of (a) and (b) and not of (d).  -> profiles/exposure.txt

    python scripts/bench_exposure.py [--reps 5]
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
from cupyimg_amd.skimage import exposure  # noqa: E402


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


def test_volume(shape, dtype, seed):
    """a ball plus a ramp plus noise, in [0, 1] (float32) or 12 bits on an offset (uint16)"""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[(np.arange(n, dtype=np.float32) + 0.5) / n for n in shape], indexing="ij", sparse=True)
    f = 0.5 * (sum(((a - 0.5) / 0.35) ** 2 for a in axes) <= 1.0) + 0.1 * sum(axes) + 0.2 * rng.random(shape, dtype=np.float32)
    f = (f - f.min()) / (f.max() - f.min())
    if np.dtype(dtype) == np.uint16:
        return np.rint(100 + 4000 * f).astype(np.uint16)
    return f.astype(dtype)


def emit(**rec):
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_clahe
    knob.argtypes = [ctypes.c_int] * 2
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    for shape, dtype in (((512, 512, 512), "float32"), ((181, 217, 181), "uint16")):
        name = "{} {}".format(dtype, "x".join(map(str, shape)))
        x = ca.asarray(test_volume(shape, dtype, 1))
        n = x.size
        rec = {"case": "equalize_adapthist, defaults, " + name}
        for label, setting in (("planned", (0, 0)), ("generic", (1, 0))):
            knob(*setting)
            us, spread = timed(lambda: exposure.equalize_adapthist(x), a.reps)
            rec[label + "_us"] = round(us, 1)
            rec[label + "_spread_us"] = round(spread, 1)
            rec[label + "_kernel"] = ca.last_kernel()
        knob(0, 0)
        nbytes = n * (2 * x.dtype.itemsize + 12)
        m = (nbytes // 2 // 4) // 4 * 4                     # floats copied: half the bytes read, half written
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        us, spread = timed(lambda: _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None)), a.reps)
        rec["copy_of_the_bytes_us"] = round(us, 1)
        rec["copy_spread_us"] = round(spread, 1)
        rec["copy_TB_per_s"] = round(2 * m * 4 / us / 1e6, 2)
        rec["planned_over_copy"] = round(rec["planned_us"] / us, 2)
        rec["generic_over_planned"] = round(rec["generic_us"] / rec["planned_us"], 2)
        del src, dst
        emit(**rec)
        us, spread = timed(lambda: exposure.equalize_hist(x), a.reps)
        emit(case="equalize_hist, defaults, " + name, call_us=round(us, 1), spread_us=round(spread, 1), kernel=ca.last_kernel())


if __name__ == "__main__":
    main()
