"""peak_local_max / corner_peaks and the primitives under them (csrc/select.hip): one JSON line per case with the time of one
call (hipEvents around a burst of calls, warm; median, minimum and maximum over the repetitions, the comparators alternating
inside every repetition) for
  (a) the candidate stage (mi_peak_count + mi_peak_write: the fused predicate through count, scan and scatter) on the Harris
      response of a seeded 4096 x 4096 float32 texture and on a seeded 256^3 float32 volume, min_distance 1 and 5, against
      the in-tree float4 copy kernel (mi_debug_copy_f32) moving the same bytes: image and image_max read twice;
  (b) argsort of 10^5 and 10^7 float32 keys against the copy kernel moving passes x 2 x 12 bytes an element (a pass reads the
      (key, index) pair for the histogram, reads it again and writes it for the scatter);
  (c) whole peak_local_max and corner_peaks calls on the same inputs, with the launches of csrc/select.hip and the host
      read-backs counted (threshold reduction, candidate count, one per batch of spacing rounds, the survivors' count);
  (d) the plateau: a 1024 x 1024 constant square inside a 1536 x 1536 image, min_distance 5: rounds and time.
The lines go to stdout and to --out.

    python scripts/bench_peaks.py [--reps 5] [--burst 3] [--out profiles/peaks.txt]
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
    ca.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(burst_us(fn, burst))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def texture(shape, seed):
    """smoothed seeded noise, float32, on the device"""
    x = ca.asarray(np.random.default_rng(seed).random(shape, dtype=np.float32))
    return ndi.gaussian_filter(x, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=3)
    ap.add_argument("--image", type=int, default=4096)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--plateau", type=int, default=1024)
    ap.add_argument("--sort", default="100000,10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ca.set_device(0)
    lib = _lib.load()
    copy = lib.mi_debug_copy_f32
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    emit(device=ca.device_name(), reps=a.reps, burst=a.burst)

    def copier(nbytes):
        m = (nbytes // 2) // 16 * 4                      # floats: read m, write m
        src, dst = ca.zeros((m,), np.float32), ca.zeros((m,), np.float32)
        return lambda: _lib.check(copy(ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), m, 2048, None)), 8 * m

    def record(rec, res):
        for k, (us, lo, hi) in res.items():
            rec[k + "_us"] = round(us, 1)
            rec[k + "_min_us"] = round(lo, 1)
            rec[k + "_max_us"] = round(hi, 1)

    inputs = []
    if a.image:
        inputs.append(("harris response {0}x{0}".format(a.image), feature.corner_harris(texture((a.image, a.image), 1))))
    if a.volume:
        inputs.append(("volume {0}x{0}x{0}".format(a.volume), texture((a.volume,) * 3, 2)))
    for name, image in inputs:
        lo, hi = (float(v) for v in (image.get().min(), image.get().max()))
        for min_distance in (1, 5):
            image_max = ca.ascontiguousarray(ndi.maximum_filter(image, size=2 * min_distance + 1, mode="constant"))
            border = (min_distance,) * image.ndim
            kernels = {}

            def stage():
                coords, _ = feature._peak_candidates(image, image_max, lo, border)
                kernels.setdefault("write", ca.last_kernel())
                return coords
            k = stage().shape[0]
            fns = {"candidates": stage, "peak_local_max": lambda: feature.peak_local_max(image, min_distance=min_distance),
                   "corner_peaks": lambda: feature.corner_peaks(image, min_distance=min_distance),
                   "maximum_filter": lambda: ndi.maximum_filter(image, size=2 * min_distance + 1, mode="constant")}
            fns["copy"], moved = copier(4 * image.itemsize * image.size)
            res = compare(fns, a.reps, a.burst)
            rec = {"case": "{}, float32, min_distance {}".format(name, min_distance), "candidates": k, "bytes_per_voxel_candidates": 16}
            record(rec, res)
            rec["copy_TB_per_s"] = round(moved / res["copy"][0] / 1e6, 2)
            rec["candidates_over_copy"] = round(res["candidates"][0] / res["copy"][0], 2)
            feature.peak_local_max(image, min_distance=min_distance)
            rec["peak_local_max_select_launches"] = feature.last_peak_launches()
            rec["peaks"] = int(feature.peak_local_max(image, min_distance=min_distance).shape[0])
            feature.corner_peaks(image, min_distance=min_distance)
            rec["corner_peaks_select_launches"] = feature.last_peak_launches()
            rec["threshold"] = lo
            rec["image_max_value"] = hi
            rec.update({k_ + "_kernel": v for k_, v in kernels.items()})
            emit(**rec)
            del image_max, fns

    for n in [int(v) for v in a.sort.split(",") if v]:
        keys = ca.asarray(np.random.default_rng(3).standard_normal(n).astype(np.float32))
        passes = 4
        fns = {"argsort": lambda: ca.argsort(keys), "argsort_descending": lambda: ca.argsort(keys, descending=True)}
        fns["copy"], moved = copier(passes * 2 * 12 * n)
        res = compare(fns, a.reps, a.burst)
        rec = {"case": "argsort, float32, {} keys".format(n), "passes": passes, "bytes_per_key_modelled": passes * 2 * 12,
               "kernel": ca.last_kernel()}
        record(rec, res)
        rec["argsort_over_copy"] = round(res["argsort"][0] / res["copy"][0], 2)
        rec["Mkeys_per_s"] = round(n / res["argsort"][0], 1)
        emit(**rec)
        del keys, fns

    if a.plateau:
        side = a.plateau
        host = np.zeros((side + side // 2,) * 2, np.float32)
        host[side // 4:side // 4 + side, side // 4:side // 4 + side] = 1.0
        image = ca.asarray(host)
        fn = lambda: feature.peak_local_max(image, min_distance=5)          # noqa: E731
        peaks = fn()
        launches = feature.last_peak_launches()
        res = compare({"peak_local_max": fn}, max(a.reps // 2, 1), 1)
        rec = {"case": "plateau {0}x{0} inside {1}x{1}, float32, min_distance 5".format(side, host.shape[0]), "candidates": side * side,
               "peaks": int(peaks.shape[0]), "select_launches": launches, "rounds_queued_at_most": launches // 2}
        record(rec, res)
        emit(**rec)
    out.close()


if __name__ == "__main__":
    main()
