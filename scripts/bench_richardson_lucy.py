"""skimage.restoration.richardson_lucy (csrc/richardson_lucy.hip): one JSON line per case with the time of ONE ITERATION
(hipEvents around a burst of mi_richardson_lucy_step calls on arrays already on the device, warm; median, minimum and maximum
over the repetitions, the comparators alternating inside every repetition) for
  (a) the fused kernel on the planner's tiles (mi_debug_set_richardson_lucy(3): wherever its rings fit, whatever the planner's
      table says) and the split route (mi_debug_set_richardson_lucy(1)) -- the same build, the same process,
  (b) what the planner itself takes (route 0), with the kernel it named,
  (c) a LOWER BOUND for any composition from this library's public calls: two scipy.signal.convolve(..., "same") calls on a
      volume of the same shape and dtype (the division and the multiply cannot be written publicly and are not timed),
  (d) the in-tree float4 copy kernel (mi_debug_copy_f32) moving three volumes' worth of bytes (image and u read, u written),
  (e) 2 * taps * voxels over the fused time as a double-precision multiply-add rate.
`fused_faster`: the fused kernel's median beats the split route's and the ranges of the repetitions do not overlap; the planner
(rl_planner_takes_fused) sends a case to the fused kernel only where this held.  The lines go to stdout and to --out.

    python scripts/bench_richardson_lucy.py [--reps 5] [--burst 3] [--out profiles/richardson_lucy.txt]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cupyimg_amd as ca  # noqa: E402
from cupyimg_amd import _lib  # noqa: E402
from cupyimg_amd.scipy import signal  # noqa: E402

CASES = [("float32", (4096, 4096), (5, 5)), ("float32", (4096, 4096), (15, 15)), ("float64", (2048, 2048), (5, 5)),
         ("float32", (256, 256, 256), (5, 5, 5)), ("float32", (256, 256, 256), (3, 7, 7)), ("float32", (181, 217, 181), (5, 5, 5))]


def burst_us(fn, burst):
    a, b = ca.Event(), ca.Event()
    a.record()
    for _ in range(burst):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) * 1e3 / burst


def compare(fns, reps, burst):
    """{label: (median us, min us, max us)}; every repetition times every comparator once, in turn"""
    for fn in fns.values():
        fn()
    ca.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(burst_us(fn, burst))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=3)
    ap.add_argument("--cases", default="", help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "richardson_lucy.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_richardson_lucy
    knob.argtypes = [ctypes.c_int]
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    emit(device=ca.device_name(), reps=a.reps, burst=a.burst)

    picked = [int(v) for v in a.cases.split(",") if v] or range(len(CASES))
    for dtype, ishape, pshape in [CASES[i] for i in picked]:
        rng = np.random.default_rng(1)
        image = ca.asarray((rng.random(ishape) + 0.1).astype(dtype))
        psf = rng.random(pshape).astype(dtype).astype(np.float64)
        psf /= psf.sum()
        u = [ca.full(ishape, 0.5, dtype), ca.empty(ishape, dtype)]
        scratch = ca.empty(ishape, dtype)
        idesc, udesc = image._desc(), [u[0]._desc(), u[1]._desc()]
        pshape_c = (ctypes.c_int64 * len(pshape))(*pshape)
        pptr = psf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        kernels = {}

        def routed(route, label):
            def run():
                knob(route)
                _lib.check(lib.mi_richardson_lucy_step(ctypes.byref(idesc), ctypes.byref(udesc[0]), ctypes.byref(udesc[1]), pptr, pshape_c,
                                                       0.0, 0, 0, ctypes.c_void_p(scratch.ptr), None))
                kernels.setdefault(label, ca.last_kernel())
                knob(0)
            return run

        fns = {"fused": routed(3, "fused"), "split": routed(1, "split"), "planner": routed(0, "planner")}
        m = (3 * image.nbytes // 2) // 16 * 4               # floats: read m, write m
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        fns["copy"] = lambda: _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None))
        res = compare(fns, a.reps, a.burst)
        del src, dst
        cres = compare({"convolve": lambda: signal.convolve(u[0], psf, mode="same")}, min(a.reps, 3), 1)

        taps = float(np.prod(ishape)) * float(np.prod(pshape))
        rec = {"case": "richardson_lucy iteration, {} {} psf {}".format(dtype, "x".join(map(str, ishape)), "x".join(map(str, pshape))),
               "three_volumes_bytes": int(3 * image.nbytes)}
        for k, (us, lo, hi) in list(res.items()) + list(cres.items()):
            rec[k + "_us"] = round(us, 1)
            rec[k + "_min_us"] = round(lo, 1)
            rec[k + "_max_us"] = round(hi, 1)
        rec["two_public_convolves_us"] = round(2 * cres["convolve"][0], 1)
        rec["two_public_convolves_over_planner"] = round(2 * cres["convolve"][0] / res["planner"][0], 2)
        rec["split_over_fused"] = round(res["split"][0] / res["fused"][0], 2)
        rec["fused_over_copy"] = round(res["fused"][0] / res["copy"][0], 2)
        rec["fused_f64_Gfma_per_s"] = round(2 * taps / res["fused"][0] / 1e3, 1)
        rec["split_f64_Gfma_per_s"] = round(2 * taps / res["split"][0] / 1e3, 1)
        rec["fused_faster"] = bool(res["fused"][0] < res["split"][0] and res["fused"][2] < res["split"][1])
        rec.update({k + "_kernel": v for k, v in kernels.items()})
        emit(**rec)
        del image, u, scratch, fns
    out.close()


if __name__ == "__main__":
    main()
