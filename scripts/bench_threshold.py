"""skimage.filters thresholding (csrc/threshold.hip): one JSON line per case with the time of one call (hipEvents around a
burst of calls, warm; median, minimum and maximum over the repetitions, the comparators alternating inside every repetition).

  window statistics: threshold_sauvola and threshold_niblack with the default window of 15 on a 4096 x 4096 uint8 and float32
      image, and with window_size=7 on a 256^3 uint16 volume, each
      (a) on the fused kernel (a tile and its halo in LDS, sums axis by axis, the threshold written straight out),
      (b) forced onto the generic kernel (one thread per output, the window summed directly) by mi_debug_set_threshold,
      (c) against the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes the fused route must move -- the sample
          read once and one double written: 9 bytes a pixel for uint8, 12 for float32, 10 a voxel for uint16 --
      (d) and against two ndimage.uniform_filter(image as float64, size=w) calls: the two box means a user could compose from
          what the library had before (m from one, the mean of x^2 from the other needs one more pass that is not counted).
  whole calls: threshold_li and threshold_otsu on the two 4096 x 4096 images (host round trips included: these end in a read
      of a few numbers), threshold_multiotsu with 3 and 4 classes on the uint8 image.
  comparison: one `image > t` launch on the float32 image against the copy kernel moving its 5 bytes a pixel.
`fused_stays_default`: the fused route's median beats the generic route's and the ranges of the repetitions do not overlap.

    python scripts/bench_threshold.py [--reps 7] [--burst 5] [--out profiles/threshold.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cupyimg_amd as ca  # noqa: E402
from cupyimg_amd import _lib  # noqa: E402
from cupyimg_amd.scipy import ndimage as ndi  # noqa: E402
from cupyimg_amd.skimage import filters  # noqa: E402


def burst_us(fn, burst):
    a, b = ca.Event(), ca.Event()
    a.record()
    for _ in range(burst):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) * 1e3 / burst


def host_us(fn, burst):
    """calls that read their result back: a host clock around calls that each end in a synchronising read"""
    ca.synchronize()
    t0 = time.perf_counter()
    for _ in range(burst):
        fn()
    return (time.perf_counter() - t0) * 1e6 / burst


def compare(fns, reps, burst, timer=burst_us):
    for fn in fns.values():
        fn()
        fn()
    ca.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timer(fn, burst))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def beats(res, fused, generic):
    return bool(res[fused][0] < res[generic][0] and res[fused][2] < res[generic][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_threshold
    knob.argtypes = [ctypes.c_int] * 2
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    emit(device=ca.device_name(), reps=a.reps, burst=a.burst)

    def copier(nbytes):
        m = (nbytes // 2) // 16 * 4                      # floats: read m, write m
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        return lambda: _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None)), 8 * m

    def routed(setting, fn, kernels=None, label=None):
        def run():
            knob(*setting)
            fn()
            if kernels is not None:
                kernels.setdefault(label, ca.last_kernel())
            knob(0, 0)
        return run

    def record(rec, res):
        for k, (us, lo, hi) in res.items():
            rec[k + "_us"] = round(us, 1)
            rec[k + "_min_us"] = round(lo, 1)
            rec[k + "_max_us"] = round(hi, 1)

    rng = np.random.default_rng(1)
    side, vol = a.side, a.volume
    img8 = ca.asarray(rng.integers(0, 256, size=(side, side)).astype(np.uint8))
    img32 = ca.asarray((rng.random((side, side)) * 1000).astype(np.float32))
    vol16 = ca.asarray(rng.integers(0, 65536, size=(vol, vol, vol)).astype(np.uint16))

    for name, x, w in (("uint8 {0}x{0}".format(side), img8, 15), ("float32 {0}x{0}".format(side), img32, 15),
                       ("uint16 {0}x{0}x{0}".format(vol), vol16, 7)):
        moved_per = x.dtype.itemsize + 8
        x64 = x.astype(np.float64)
        for fname, fn in (("threshold_sauvola", lambda: filters.threshold_sauvola(x, w, r=128.0)),
                          ("threshold_niblack", lambda: filters.threshold_niblack(x, w))):
            kernels = {}
            fns = {"fused": routed((0, 0), fn, kernels, "fused"), "generic": routed((0, 1), fn, kernels, "generic"),
                   "two_uniform_filters": lambda: (ndi.uniform_filter(x64, size=w), ndi.uniform_filter(x64, size=w))}
            fns["copy"], moved = copier(moved_per * x.size)
            res = compare(fns, a.reps, a.burst)
            rec = {"case": "{}, {}, window {}".format(fname, name, w), "bytes_per_sample_fused": moved_per}
            record(rec, res)
            rec["copy_TB_per_s"] = round(moved / res["copy"][0] / 1e6, 2)
            rec["fused_over_copy"] = round(res["fused"][0] / res["copy"][0], 2)
            rec["generic_over_fused"] = round(res["generic"][0] / res["fused"][0], 2)
            rec["two_uniform_filters_over_fused"] = round(res["two_uniform_filters"][0] / res["fused"][0], 2)
            rec["fused_Gsample_per_s"] = round(x.size / res["fused"][0] / 1e3, 2)
            rec["fused_stays_default"] = beats(res, "fused", "generic")
            rec.update({k + "_kernel": v for k, v in kernels.items()})
            emit(**rec)
        del x64

    for name, x in (("uint8 {0}x{0}".format(side), img8), ("float32 {0}x{0}".format(side), img32)):
        iters = []
        filters.threshold_li(x, iter_callback=iters.append)
        res = compare({"threshold_li": lambda: filters.threshold_li(x), "threshold_otsu": lambda: filters.threshold_otsu(x)}, a.reps, 2, host_us)
        rec = {"case": "whole calls, {}".format(name), "li_iterations": len(iters) - 1, "timer": "host clock, each call ends in a read"}
        record(rec, res)
        emit(**rec)
    res = compare({"multiotsu_3": lambda: filters.threshold_multiotsu(img8, 3), "multiotsu_4": lambda: filters.threshold_multiotsu(img8, 4)},
                  a.reps, 2, host_us)
    rec = {"case": "threshold_multiotsu, uint8 {0}x{0}, 256 bins".format(side), "tuples_3": 255 * 254 // 2, "tuples_4": 255 * 254 * 253 // 6,
           "timer": "host clock, each call ends in a read"}
    record(rec, res)
    emit(**rec)

    fns = {"greater": lambda: img32 > 500.0}
    fns["copy"], moved = copier(5 * img32.size)
    res = compare(fns, a.reps, a.burst)
    rec = {"case": "image > t, float32 {0}x{0}".format(side), "bytes_per_sample": 5, "kernel": ca.last_kernel()}
    record(rec, res)
    rec["copy_TB_per_s"] = round(moved / res["copy"][0] / 1e6, 2)
    rec["greater_over_copy"] = round(res["greater"][0] / res["copy"][0], 2)
    emit(**rec)
    out.close()


if __name__ == "__main__":
    main()
