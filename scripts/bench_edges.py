"""skimage.filters.sobel on float32 volumes and a 4096 x 4096 image, and skimage.feature.canny on 4096 x 4096 images
(csrc/edges.hip): one JSON line per case with the time of one call (hipEvents around a burst of calls, warm; median and spread over the repetitions, the
comparators alternating inside every repetition) for
  sobel (magnitude, float32 in, float64 out):
  (a) the fused kernel under the planner's boxes,
  (b) the library's unfused route forced through mi_debug_set_edges (one dense correlate per axis plus per-voxel passes),
  (c) the composition of the same result from public calls that exist without the edge family: ndi.convolve per axis,
      _support.elementwise multiply / add / sqrt and scale_shift by 1 / ndim (a multiplication where the operator divides: the
      same bytes moved, not the same last bit) -- this script builds it itself, so it also runs on a tree without the family,
  (d) the ceiling: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the 12 bytes per voxel a fused call must move;
  canny (float32 and uint8 images, default thresholds):
  (a) the whole call with the fused stage kernel, (b) the whole call with the stage forced to its unfused route, (c) the
      stage alone either way, (d) the copy kernel moving the stage's 21 bytes per pixel.  (The non-maximum suppression cannot
      be composed from public calls that exist without the family: there is no comparison or division among them.)
The lines go to stdout and to --out.

    python scripts/bench_edges.py [--reps 7] [--burst 5] [--out profiles/edges.txt]
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
from cupyimg_amd.scipy import ndimage as ndi  # noqa: E402
from cupyimg_amd.scipy.ndimage import _support as S  # noqa: E402
from cupyimg_amd.skimage import feature, filters  # noqa: E402


def burst_us(fn, burst):
    a, b = ca.Event(), ca.Event()
    a.record()
    for _ in range(burst):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) * 1e3 / burst


def compare(fns, reps, burst):
    """{label: (median us, spread us)}; every repetition times every comparator once, in turn"""
    for fn in fns.values():
        fn()
        fn()
    ca.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(burst_us(fn, burst))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in ts.items()}


def sobel_kernels(ndim):
    """per edge axis the dense 3^ndim kernel: [1, 0, -1] along it times [1, 2, 1] / 4 along every other axis"""
    def along(weights, axis):
        return np.asarray(weights).reshape([3 if a == axis else 1 for a in range(ndim)])

    kernels = []
    for edge in range(ndim):
        k = along([1, 0, -1], edge)
        for other in range(ndim):
            if other != edge:
                k = k * along(np.array([1, 2, 1]) / 4, other)
        kernels.append(k)
    return kernels


def sobel_composition(x):
    """the magnitude from public calls: ndim convolves, as many squares in float32 and accumulations into float64, a scaling, a root"""
    out = None
    for k in sobel_kernels(x.ndim):
        r = ndi.convolve(x, k)
        S.elementwise("multiply", r, r, r)
        if out is None:
            out = r.astype(np.float64)
        else:
            S.elementwise("add", out, r, out)
    out = S.scale_shift(out, 1.0 / x.ndim, 0.0)
    return S.elementwise("sqrt", out, None, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--shapes", default="256x256x256,512x512x512,181x217x181,4096x4096")
    ap.add_argument("--canny", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edges.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    have = hasattr(filters, "sobel") and hasattr(lib, "mi_debug_set_edges")
    if have:
        knob = lib.mi_debug_set_edges
        knob.argtypes = [ctypes.c_int] * 2
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    emit(device=ca.device_name(), reps=a.reps, burst=a.burst, edge_family=have)

    def copier(nbytes):
        m = (nbytes // 2) // 16 * 4                      # floats: read m, write m
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        return lambda: _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None)), 8 * m

    for shape in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]:
        name = "x".join(map(str, shape))
        x = ca.asarray(np.random.default_rng(1).random(shape, dtype=np.float32))
        n = x.size
        kernels = {}
        fns = {}
        if have:
            def fused():
                knob(0, 0)
                filters.sobel(x)
                kernels.setdefault("fused", ca.last_kernel())

            def generic():
                knob(0, 1)
                filters.sobel(x)
                kernels.setdefault("generic", ca.last_kernel())
                knob(0, 0)
            fns["fused"], fns["generic"] = fused, generic
        fns["composition"] = lambda: sobel_composition(x)
        fns["copy"], moved = copier(12 * n)
        res = compare(fns, a.reps, a.burst)
        rec = {"case": "sobel magnitude, float32 " + name, "rank": len(shape), "bytes_per_voxel_fused": 12}
        for k, (us, spread) in res.items():
            rec[k + "_us"] = round(us, 1)
            rec[k + "_spread_us"] = round(spread, 1)
        rec["copy_TB_per_s"] = round(moved / res["copy"][0] / 1e6, 2)
        if have:
            rec["fused_over_copy"] = round(res["fused"][0] / res["copy"][0], 2)
            rec["composition_over_fused"] = round(res["composition"][0] / res["fused"][0], 2)
            rec["generic_over_fused"] = round(res["generic"][0] / res["fused"][0], 2)
            rec["fused_faster_than_composition"] = bool(res["fused"][0] < res["composition"][0])
            rec["fused_Gvoxel_per_s"] = round(n / res["fused"][0] / 1e3, 2)
            rec.update({k + "_kernel": v for k, v in kernels.items()})
        emit(**rec)
        del x, fns

    if have and a.canny:
        side = a.canny
        base = np.random.default_rng(2).random((side, side))
        for dtype in ("float32", "uint8"):
            image = ca.asarray(base.astype(np.float32) if dtype == "float32" else np.round(base * 255).astype(np.uint8))
            smoothed = feature._canny_smooth(image, None, 1.0)
            eroded = ndi.binary_erosion(ca.ones(image.shape, np.bool_), ndi.generate_binary_structure(2, 2), border_value=0)
            kernels = {}

            def call(setting, label, stage):
                def fn():
                    knob(*setting)
                    if stage:
                        feature._canny_stage(smoothed, eroded, 0.2, 0.1)
                        kernels.setdefault(label, ca.last_kernel())
                    else:
                        feature.canny(image)
                    knob(0, 0)
                return fn
            fns = {"call_fused": call((0, 0), "fused", False), "call_generic": call((0, 1), "generic", False),
                   "stage_fused": call((0, 0), "fused", True), "stage_generic": call((0, 1), "generic", True)}
            fns["copy"], moved = copier(21 * image.size)
            res = compare(fns, a.reps, max(1, a.burst // 2))
            rec = {"case": "canny, {} {}x{}".format(dtype, side, side), "bytes_per_pixel_stage": 21}
            for k, (us, spread) in res.items():
                rec[k + "_us"] = round(us, 1)
                rec[k + "_spread_us"] = round(spread, 1)
            rec["stage_fused_over_copy"] = round(res["stage_fused"][0] / res["copy"][0], 2)
            rec["stage_generic_over_fused"] = round(res["stage_generic"][0] / res["stage_fused"][0], 2)
            rec["call_generic_over_fused"] = round(res["call_generic"][0] / res["call_fused"][0], 2)
            rec["fused_faster_than_generic"] = bool(res["stage_fused"][0] < res["stage_generic"][0])
            rec.update({k + "_kernel": v for k, v in kernels.items()})
            emit(**rec)
            del image, smoothed, eroded
    out.close()


if __name__ == "__main__":
    main()
