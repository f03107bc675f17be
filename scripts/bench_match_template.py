"""skimage.feature.match_template (csrc/template.hip): one JSON line per case with the time of one call (hipEvents around a
burst of calls, warm; median, minimum and maximum over the repetitions, the comparators alternating inside every repetition) for
  (a) the whole call under the planner (mt_fused_kernel) and forced to the per-output kernel through
      mi_debug_set_match_template(1) -- the same build, the same process,
  (b) the kernel alone either way: mi_match_template on arrays already on the device (no template statistics, no upload, no
      allocation),
  (c) a LOWER BOUND for the same quantity composed from this library's public calls: ndi.correlate of the image with the
      template into float64 plus ndi.uniform_filter of the image and of a float64 array of its size (standing in for its
      square: the library has no public pointwise product) into float64; the pointwise steps of the formula are not timed.
      _pad.pad of the image by the template's shape, which the composition needs with pad_input, is timed on its own,
  (d) the ceiling: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes the call must move (the image read
      once, the float64 result written once).
`fused_stays_default`: the fused kernel's median beats the per-output kernel's and the ranges of the repetitions do not
overlap.  `fused_Gtap_per_s`: outputs x template samples per second of the fused kernel alone; a tap is 3 float64 additions and
1 multiplication per output plus 1 multiplication per 4 outputs, so 39.3e12 float64 operations a second (256 CUs x 64 lanes x
2.4 GHz, no FMA: -ffp-contract=off) bound it at 9.25e12 taps a second.  The lines go to stdout and to --out.

    python scripts/bench_match_template.py [--reps 5] [--burst 3] [--out profiles/match_template.txt]
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
from cupyimg_amd import _lib, _pad  # noqa: E402
from cupyimg_amd.scipy import ndimage as ndi  # noqa: E402
from cupyimg_amd.skimage.feature import match_template  # noqa: E402

CASES = [("float32", (4096, 4096), (16, 16)), ("float32", (4096, 4096), (64, 64)), ("uint8", (2048, 2048), (32, 32)),
         ("float32", (256, 256, 256), (8, 8, 8)), ("float32", (181, 217, 181), (7, 9, 7))]
PEAK_TAPS = 256 * 64 * 2.4e9 / 4.25


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


def beats(res, fused, generic):
    return bool(res[fused][0] < res[generic][0] and res[fused][2] < res[generic][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=3)
    ap.add_argument("--cases", default="", help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_template.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_match_template
    knob.argtypes = [ctypes.c_int]
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    emit(device=ca.device_name(), reps=a.reps, burst=a.burst)

    def routed(route, fn, kernels=None, label=None):
        def run():
            knob(route)
            fn()
            if kernels is not None:
                kernels.setdefault(label, ca.last_kernel())
            knob(0)
        return run

    picked = [int(v) for v in a.cases.split(",") if v] or range(len(CASES))
    for dtype, ishape, tshape in [CASES[i] for i in picked]:
        rng = np.random.default_rng(1)
        host = rng.integers(0, 256, size=ishape).astype(dtype) if dtype == "uint8" else rng.random(ishape, dtype=np.float32)
        thost = rng.random(tshape)
        x, t = ca.asarray(host), ca.asarray(thost)
        oshape = tuple(n - k + 1 for n, k in zip(ishape, tshape))
        res_out = ca.empty(oshape, np.float64)
        mean = thost.mean()
        ssd = float(((thost - mean) ** 2).sum())
        xd, td, od = x._desc(), t._desc(), res_out._desc()
        kernels = {}

        def kernel():
            _lib.check(lib.mi_match_template(ctypes.byref(xd), ctypes.byref(td), ctypes.byref(od), 0, _lib.MODE_CODES["constant"], 0.0,
                                             float(mean), ssd, None))
        whole = lambda: match_template(x, t)                                          # noqa: E731
        fns = {"call_fused": routed(0, whole), "call_generic": routed(1, whole),
               "kernel_fused": routed(0, kernel, kernels, "fused"), "kernel_generic": routed(1, kernel, kernels, "generic")}
        moved = x.nbytes + res_out.nbytes
        m = (moved // 2) // 16 * 4                      # floats: read m, write m
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        fns["copy"] = lambda: _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None))
        res = compare(fns, a.reps, a.burst)
        del src, dst

        # the composition from public calls: one repetition fewer bursts, it is the slow one
        x64 = x.astype(np.float64)
        c_out, u_out = ca.empty(ishape, np.float64), ca.empty(ishape, np.float64)
        composed = {"correlate": lambda: ndi.correlate(x, thost, output=c_out, mode="constant"),
                    "box_image": lambda: ndi.uniform_filter(x, size=tshape, output=u_out, mode="constant"),
                    "box_square": lambda: ndi.uniform_filter(x64, size=tshape, output=u_out, mode="constant"),
                    "pad": lambda: _pad.pad(x, [(k, k) for k in tshape], mode="constant")}
        cres = compare(composed, min(a.reps, 3), 1)

        taps = float(np.prod(oshape)) * float(np.prod(tshape))
        rec = {"case": "match_template, {} {} template {}".format(dtype, "x".join(map(str, ishape)), "x".join(map(str, tshape))),
               "bytes_moved": int(moved)}
        for k, (us, lo, hi) in list(res.items()) + list(cres.items()):
            rec[k + "_us"] = round(us, 1)
            rec[k + "_min_us"] = round(lo, 1)
            rec[k + "_max_us"] = round(hi, 1)
        rec["composed_lower_bound_us"] = round(cres["correlate"][0] + cres["box_image"][0] + cres["box_square"][0], 1)
        rec["composed_lower_bound_over_call_fused"] = round(rec["composed_lower_bound_us"] / res["call_fused"][0], 2)
        rec["kernel_generic_over_fused"] = round(res["kernel_generic"][0] / res["kernel_fused"][0], 2)
        rec["kernel_fused_over_copy"] = round(res["kernel_fused"][0] / res["copy"][0], 2)
        rec["fused_Gtap_per_s"] = round(taps / res["kernel_fused"][0] / 1e3, 1)
        rec["fused_share_of_float64_peak"] = round(taps / (res["kernel_fused"][0] * 1e-6) / PEAK_TAPS, 3)
        rec["fused_stays_default"] = beats(res, "kernel_fused", "kernel_generic")
        rec.update({k + "_kernel": v for k, v in kernels.items()})
        emit(**rec)
        del x, t, x64, c_out, u_out, res_out, fns, composed
    out.close()


if __name__ == "__main__":
    main()
