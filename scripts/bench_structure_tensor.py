"""skimage.feature.structure_tensor on float32 volumes and a 4096 x 4096 image, and corner_harris on 4096 x 4096
(csrc/corners.hip): one JSON line per case with the time of one call (hipEvents around a burst of calls, warm; median, minimum
and maximum over the repetitions, the comparators alternating inside every repetition) for
  (a) the product stage (mi_structure_products: every Sobel derivative and their pairwise products) as the fused kernel under
      the planner's boxes,
  (b) the same stage forced pass by pass through mi_debug_set_corners (one st_pass_kernel launch per 1-D pass through scratch
      arrays, then st_product_kernel) -- the same build, the same process,
  (c) the whole structure_tensor call either way (the product stage plus one gaussian_filter per element),
  (d) the ceiling: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes the fused product stage must move
      (float32: 4 read + 4 per element written; rank 3: 28 bytes a voxel, rank 2: 16 bytes a pixel),
  and for corner_harris the whole call either way, the response launch alone, and the copy kernel moving its 16 bytes a pixel.
--dtype float64 runs the same cases on float64 arrays (twice the bytes).
`fused_stays_default` is the rule of DESIGN.md section 4.14: the fused route's median beats the forced route's and the ranges
of the repetitions do not overlap.  The lines go to stdout and to --out.

    python scripts/bench_structure_tensor.py [--reps 7] [--burst 5] [--dtype float32] [--out profiles/structure_tensor.txt]
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
from cupyimg_amd.skimage import feature  # noqa: E402


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
        fn()
    ca.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(burst_us(fn, burst))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def beats(res, fused, generic):
    """the fused median is the smaller one and the two ranges do not overlap"""
    return bool(res[fused][0] < res[generic][0] and res[fused][2] < res[generic][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--shapes", default="256x256x256,512x512x512,181x217x181,4096x4096")
    ap.add_argument("--harris", type=int, default=4096)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_tensor.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_corners
    knob.argtypes = [ctypes.c_int] * 2
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    dtype = np.dtype(a.dtype)
    emit(device=ca.device_name(), reps=a.reps, burst=a.burst, dtype=a.dtype)

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

    for shape in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]:
        name = "x".join(map(str, shape))
        x = ca.asarray(np.random.default_rng(1).random(shape, dtype=dtype))
        n, rank = x.size, len(shape)
        elements = rank * (rank + 1) // 2
        moved_per = dtype.itemsize * (1 + elements)
        block = feature._row_block(elements, n, dtype)
        kernels = {}
        stage = lambda: feature._sobel_block(x, True, False, "constant", 0.0, out=block)      # noqa: E731
        whole = lambda: feature.structure_tensor(x, sigma=1, order="rc")                      # noqa: E731
        fns = {"stage_fused": routed((0, 0), stage, kernels, "fused"), "stage_generic": routed((0, 1), stage, kernels, "generic"),
               "call_fused": routed((0, 0), whole), "call_generic": routed((0, 1), whole)}
        fns["copy"], moved = copier(moved_per * n)
        res = compare(fns, a.reps, a.burst)
        rec = {"case": "structure_tensor, {} {}".format(a.dtype, name), "rank": rank, "bytes_per_voxel_stage": moved_per}
        record(rec, res)
        rec["copy_TB_per_s"] = round(moved / res["copy"][0] / 1e6, 2)
        rec["stage_fused_over_copy"] = round(res["stage_fused"][0] / res["copy"][0], 2)
        rec["stage_generic_over_fused"] = round(res["stage_generic"][0] / res["stage_fused"][0], 2)
        rec["call_generic_over_fused"] = round(res["call_generic"][0] / res["call_fused"][0], 2)
        rec["stage_fused_Gvoxel_per_s"] = round(n / res["stage_fused"][0] / 1e3, 2)
        rec["fused_stays_default"] = beats(res, "stage_fused", "stage_generic")
        rec.update({k + "_kernel": v for k, v in kernels.items()})
        emit(**rec)
        del x, block, fns

    if a.harris:
        side = a.harris
        image = ca.asarray(np.random.default_rng(2).random((side, side), dtype=dtype))
        block, shape = feature._structure_tensor_block(image, [1.0, 1.0], "constant", 0, "rc")
        kernels = {}
        whole = lambda: feature.corner_harris(image)                                                 # noqa: E731
        response = lambda: feature._corner_response(block, shape, "harris_k", dtype, 0.05)      # noqa: E731
        fns = {"call_fused": routed((0, 0), whole), "call_generic": routed((0, 1), whole), "response": routed((0, 0), response, kernels, "response")}
        fns["copy"], moved = copier(4 * dtype.itemsize * image.size)
        res = compare(fns, a.reps, a.burst)
        rec = {"case": "corner_harris, {} {}x{}".format(a.dtype, side, side), "bytes_per_pixel_response": 4 * dtype.itemsize}
        record(rec, res)
        rec["response_over_copy"] = round(res["response"][0] / res["copy"][0], 2)
        rec["call_generic_over_fused"] = round(res["call_generic"][0] / res["call_fused"][0], 2)
        rec["fused_stays_default"] = beats(res, "call_fused", "call_generic")
        rec.update({k + "_kernel": v for k, v in kernels.items()})
        emit(**rec)
    out.close()


if __name__ == "__main__":
    main()
