"""skimage.registration.optical_flow_tvl1 (csrc/tvl1.hip) on MRI-sized float32 volumes: one JSON line per shape with the time
of one fixed-point iteration (hipEvents around a run of iterations queued through registration._iterate's entry points, warm,
median and spread of the repetitions; an iteration = the data-term kernel plus the regularisation) for
  (a) the fused regularisation kernel under the planner's tiles,
  (b) the per-voxel kernels forced through mi_debug_set_tvl1 (four launches, u^1 and p^1 through memory),
  (c) the ceiling: the in-tree float4 copy kernel (mi_debug_copy_f32) moving the bytes a fused iteration must move, 35 volumes'
      worth (data term: grad, NI, rho_0 and the flow read, the flow written = 11; regularisation: the flow and proj read and
      written = 24) = 17.5 volumes copied,
and the time of a whole default call.  The lines go to stdout and to --out.

    python scripts/bench_optical_flow.py [--reps 5] [--iters 10] [--out profiles/optical_flow.txt]
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
from cupyimg_amd.skimage import registration as reg  # noqa: E402


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


def test_pair(shape, seed):
    """smoothed noise (sigma 2) and the same displaced by 1.5 voxels along axis 0, on the device"""
    x = ca.asarray(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))
    ref = ndi.gaussian_filter(x, 2.0)
    lo, hi = S.min_max(ref)
    ref = S.scale_shift(ref, 1.0 / (hi - lo), -lo / (hi - lo))
    mov = ndi.shift(ref, [1.5, 0, 0], order=1, mode="nearest")
    return ref, mov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optical_flow.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    knob = lib.mi_debug_set_tvl1
    knob.argtypes = [ctypes.c_int] * 2
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    emit(device=ca.device_name(), reps=a.reps)
    for shape in ((256, 256, 256), (181, 217, 181)):
        name = "x".join(map(str, shape))
        ref, mov = test_pair(shape, 1)
        n = ref.size
        flow = ca.zeros((3,) + shape, np.float32)
        grad, NI, rho_0 = reg._prepare(mov, ref, flow)
        flows = [flow, ca.zeros((3,) + shape, np.float32)]
        projs = [ca.zeros((3, 3) + shape, np.float32), ca.zeros((3, 3) + shape, np.float32)]
        gdesc, ndesc, r0desc = grad._desc(), NI._desc(), rho_0._desc()
        dt = 0.5 / 3
        rec = {"case": "one fixed-point iteration, float32 " + name, "iterations_timed": a.iters}
        for label, setting in (("fused", (0, 0)), ("generic", (0, 1))):
            knob(*setting)
            scratch = reg._scratch(lib, flow)
            launches = []

            def iterations():
                del launches[:]
                for i in range(a.iters):
                    launches.append(reg._fixed_point(lib, gdesc, ndesc, r0desc, flows[i & 1], flows[(i + 1) & 1], projs[i & 1]._desc(),
                                                     projs[(i + 1) & 1]._desc(), scratch, 4.5, dt, dt / 0.3))

            us, spread = timed(iterations, a.reps)
            rec[label + "_us_per_iteration"] = round(us / a.iters, 1)
            rec[label + "_spread_us"] = round(spread / a.iters, 1)
            rec[label + "_launches_per_iteration"] = launches[0]
            rec[label + "_kernel"] = ca.last_kernel()
            del scratch
        knob(0, 0)
        # the ceiling: 35 volumes' worth of bytes = a copy of 17.5 volumes between two buffers of their own
        m = (35 * n // 2) // 4 * 4
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)

        def copies():
            for _ in range(a.iters):
                _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None))

        us, spread = timed(copies, a.reps)
        rec["copy_35_volumes_us"] = round(us / a.iters, 1)
        rec["copy_spread_us"] = round(spread / a.iters, 1)
        rec["copy_TB_per_s"] = round(2 * m * 4 / (us / a.iters) / 1e6, 2)
        rec["fused_over_copy"] = round(rec["fused_us_per_iteration"] / rec["copy_35_volumes_us"], 2)
        rec["generic_over_fused"] = round(rec["generic_us_per_iteration"] / rec["fused_us_per_iteration"], 2)
        rec["fused_faster_than_generic"] = bool(rec["fused_us_per_iteration"] < rec["generic_us_per_iteration"])
        emit(**rec)
        del src, dst, flows, projs, grad, NI, rho_0, flow
        for label, setting in (("fused", (0, 0)), ("generic", (0, 1))):
            knob(*setting)
            us, spread = timed(lambda: reg.optical_flow_tvl1(ref, mov), max(2, a.reps // 2))
            emit(case="whole default call, float32 " + name + ", " + label, call_ms=round(us / 1e3, 2), spread_ms=round(spread / 1e3, 2),
                 levels=[dict(s, shape=list(s["shape"])) for s in reg.last_tvl1_stats()])
        knob(0, 0)
    out.close()


if __name__ == "__main__":
    main()
