"""find_objects, regionprops_table and remove_small_objects (csrc/regionprops.hip) on MRI-sized label images: one JSON line per
case with the device time (median of event-timed repetitions, read-backs included), the bytes the passes must move (labels
read once per sweep, plus what a pointwise pass writes), their rate against the same run's float4 copy-kernel rate (the
practical ceiling for that byte count), the launches the call queued and the kernel the library recorded last.  Where today's
public calls can compose the same answer -- area from ndimage.sum_labels, centroid from center_of_mass, the box from
minimum / maximum of one coordinate volume per axis, all with an index -- that composition is timed next to it (up to 10^5
regions: the public functions build host tuples per region).  -> profiles/regionprops.txt

    python scripts/bench_regionprops.py [--reps 5] > profiles/regionprops.txt
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
from cupyimg_amd.scipy.ndimage import measurements as meas  # noqa: E402
from cupyimg_amd.skimage import measure, morphology  # noqa: E402

MOMENT_SET = ("label", "area", "bbox", "centroid", "moments", "moments_central", "moments_normalized", "inertia_tensor",
              "inertia_tensor_eigvals", "major_axis_length", "minor_axis_length")


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
    return float(np.median(ts))


def copy_rate(reps):
    n = 1 << 27                                   # 512 MiB of float32 each way
    src, dst = ca.empty((n,), np.float32), ca.empty((n,), np.float32)
    fn = _lib.load().mi_debug_copy_f32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    us = timed(lambda: fn(src.ptr, dst.ptr, n, 4096, None), reps)
    return 2 * 4 * n / (us * 1e-6)


def smooth_mask(shape, seed):
    rng = np.random.default_rng(seed)
    small = rng.standard_normal(tuple(-(-s // 16) for s in shape)).astype(np.float32)
    big = np.kron(small, np.ones((16,) * len(shape), np.float32))[tuple(slice(0, s) for s in shape)]
    import scipy.ndimage as sndi            # host-side test data only
    return sndi.uniform_filter(big, 9) > 0.6


def launches():
    lib = _lib.load()
    return lib.mi_debug_regionprops_launches() + lib.mi_debug_select_launches()


def emit(case, fn, reps, nbytes, rate, **extra):
    try:
        before = launches()
        fn()
        queued = launches() - before
        us = timed(fn, reps)
    except (ValueError, MemoryError) as exc:
        print(json.dumps({"case": case, "refused": str(exc)[:160]}), flush=True)
        return
    rec = {"case": case, "device_us": round(us, 1), "bytes_moved": int(nbytes), "GBs": round(nbytes / (us * 1e-6) / 1e9, 1),
           "of_copy_kernel": round(nbytes / (us * 1e-6) / rate, 3), "launches": queued, "kernel": ca.last_kernel()[:140]}
    rec.update(extra)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ca.set_device(0)
    rate = copy_rate(a.reps)
    print(json.dumps({"copy_kernel_TBs": round(rate / 1e12, 3)}), flush=True)
    rng = np.random.default_rng(0)
    inputs = (("smooth 512^3", smooth_mask((512,) * 3, 0)), ("noise30 512^3", rng.random((512,) * 3) > 0.7),
              ("smooth 181x217x181", smooth_mask((181, 217, 181), 1)), ("smooth 4096^2", smooth_mask((4096, 4096), 2)))
    for name, mask in inputs:
        md = ca.asarray(mask)
        lab, n = ndi.label(md)
        nvox = mask.size
        extra = dict(regions=n)
        few = n <= 100000
        if few:
            emit("find_objects " + name, lambda: ndi.find_objects(lab, n), a.reps, nvox * 4, rate, **extra)
        else:
            # the list of millions of slice tuples is host time: the device part (the sweep, no read-back of the table)
            emit("find_objects " + name + " (extent table on the device)", lambda: meas._region_extents(lab, n), a.reps, nvox * 4, rate, **extra)
        emit("regionprops_table area,bbox,centroid " + name, lambda: measure.regionprops_table(lab, properties=("label", "area", "bbox", "centroid")),
             a.reps, nvox * 4, rate, **extra)
        emit("regionprops_table moment set " + name, lambda: measure.regionprops_table(lab, properties=MOMENT_SET), a.reps, nvox * 8, rate,
             **extra)
        emit("remove_small_objects(labels, 64) " + name, lambda: morphology.remove_small_objects(lab, 64), a.reps, nvox * 12, rate, **extra)
        emit("remove_small_objects(mask, 64) " + name + " (label included)", lambda: morphology.remove_small_objects(md, 64), a.reps, nvox * 11,
             rate, **extra)
        if few:
            # today's public calls: area = sum_labels of ones, centroid = center_of_mass of ones, the box = minimum and maximum
            # of one coordinate volume per axis: 2 + 2 ndim sweeps, each reading labels and values
            ones = ca.ones(mask.shape, np.float32)
            idx = ca.asarray(np.arange(1, n + 1, dtype=np.int64))
            coords = [ca.asarray(c.astype(np.int32)) for c in np.indices(mask.shape, dtype=np.int32)]

            def composed():
                ndi.sum_labels(ones, lab, idx)
                ndi.center_of_mass(ones, lab, idx)
                for c in coords:
                    ndi.minimum(c, lab, idx)
                    ndi.maximum(c, lab, idx)
            emit("composed area, bbox, centroid from public calls " + name, composed, a.reps, nvox * 8 * (2 + 2 * mask.ndim), rate, **extra)
            del ones, idx, coords
        del md, lab


if __name__ == "__main__":
    main()
