"""skimage.filters.frangi / sato / meijering (csrc/ridges.hip) on 256^3 and 512^3 float32 with the default five sigmas: one
JSON line per shape and filter with the time of a whole call (hipEvents, warm, median and spread of the repetitions) for
  (a) the fused kernel (one launch per scale after the Gaussian; meijering two),
  (b) the same call with mi_debug_set_ridges(0, 0, 1): unfused, the Hessian elements materialised, one thread per voxel,
  (c) the Gaussian passes of the five scales alone,
  (d) the ceiling of the fused steps: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes five fused steps
      must move -- per scale one float32 read plus one float64 read-modify-write = 20 bytes a voxel = a copy of 2.5 volumes,
and the fused steps alone (mi_ridge_scale on an already smoothed volume, five scales).  -> profiles/ridges.txt

    python scripts/bench_ridges.py [--reps 5] [--shapes 256,512]
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
from cupyimg_amd.skimage import filters  # noqa: E402

SIGMAS = tuple(range(1, 10, 2))


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


def test_volume(n, seed):
    """two crossing tubes and a plate on noise"""
    rng = np.random.default_rng(seed)
    t = (np.arange(n, dtype=np.float32) - n / 2) / (n / 16)
    z, y, x = t[:, None, None], t[None, :, None], t[None, None, :]
    v = np.exp(-(z * z + y * y) / 2) + np.exp(-(y * y + x * x) / 2) + 0.6 * np.exp(-(z - 3) ** 2 / 2)
    v = v + 0.05 * rng.standard_normal((n, n, n), dtype=np.float32)
    return (v / v.max()).astype(np.float32)


def emit(**rec):
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="256,512")
    a = ap.parse_args()
    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_ridges
    knob.argtypes = [ctypes.c_int] * 3
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    calls = {"frangi": lambda x: filters.frangi(x, mode="reflect"), "sato": lambda x: filters.sato(x, mode="reflect"),
             "meijering": lambda x: filters.meijering(x, mode="reflect")}
    kinds = {"frangi": (1, (0.5, 0.5, 450.0)), "sato": (2, (0, 0, 0)), "meijering": (3, (1 / 3, 0, 0))}
    for n in [int(s) for s in a.shapes.split(",")]:
        name = "{0}x{0}x{0}".format(n)
        x = ca.asarray(test_volume(n, 1))
        us_g, sp_g = timed(lambda: [ndi.gaussian_filter(x, sigma=float(s), mode="reflect") for s in SIGMAS], a.reps)
        m = (5 * x.size // 2) // 4 * 4
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)

        def copies():
            for _ in SIGMAS:
                _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None))

        us_c, sp_c = timed(copies, a.reps)
        del src, dst
        g = ndi.gaussian_filter(x, sigma=3.0, mode="reflect")
        for fname, call in calls.items():
            rec = {"case": fname + " float32 " + name, "sigmas": list(SIGMAS), "gaussians_us": round(us_g, 1),
                   "gaussians_spread_us": round(sp_g, 1), "copy_ceiling_5_scales_us": round(us_c, 1),
                   "copy_spread_us": round(sp_c, 1), "copy_TB_per_s": round(5 * 2 * m * 4 / us_c / 1e6, 2)}
            for label, setting in (("fused", (0, 0, 0)), ("generic", (0, 0, 1))):
                knob(*setting)
                us, spread = timed(lambda: call(x), a.reps)
                rec[label + "_call_us"] = round(us, 1)
                rec[label + "_spread_us"] = round(spread, 1)
                rec[label + "_kernel"] = ca.last_kernel()
                kind, p = kinds[fname]
                out = ca.zeros(x.shape, np.float64)
                scratch = ca.empty(x.shape, np.float32) if kind == 3 else None
                work = ca.empty((8,), np.uint8)

                def steps():
                    for s in SIGMAS:
                        if kind == 3:
                            _lib.check(lib.mi_memset(work.ptr, 0xFF, 8, None))
                        filters._ridge_scale(g, out, kind, 2, s, p, scratch, work.ptr if kind == 3 else None)

                us, spread = timed(steps, a.reps)
                rec[label + "_steps_us"] = round(us, 1)
                rec[label + "_steps_spread_us"] = round(spread, 1)
                del out, scratch
            knob(0, 0, 0)
            rec["fused_steps_over_gaussians"] = round(rec["fused_steps_us"] / us_g, 2)
            rec["fused_steps_over_copy"] = round(rec["fused_steps_us"] / us_c, 2)
            rec["generic_over_fused_steps"] = round(rec["generic_steps_us"] / rec["fused_steps_us"], 2)
            rec["fused_step_cheaper_than_its_gaussian"] = bool(rec["fused_steps_us"] < us_g)
            emit(**rec)
        del x, g
        ca.free_all_blocks()


if __name__ == "__main__":
    main()
