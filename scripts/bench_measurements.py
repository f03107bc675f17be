"""label and the labelled reductions (csrc/label.hip, csrc/measure.hip) on MRI-sized volumes: one JSON line per case with
the device time (median of event-timed repetitions; label includes its one read-back of the feature count), the
algorithmic bytes (what a single pass must move: input read + result written), their fraction of 8 TB/s, the same run's
float4 copy-kernel rate, and the kernels the call dispatched (as the library recorded them: mi_debug_last_kernel).  -> profiles/label_measurements.txt

    python scripts/bench_measurements.py [--reps 10]
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

PEAK = 8.0e12


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
    lib = _lib.load()
    fn = lib.mi_debug_copy_f32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    us = timed(lambda: fn(src.ptr, dst.ptr, n, 4096, None), reps)
    return 2 * 4 * n / (us * 1e-6)


def smooth_mask(shape, seed):
    rng = np.random.default_rng(seed)
    small = rng.standard_normal(tuple(-(-s // 16) for s in shape)).astype(np.float32)
    big = np.kron(small, np.ones((16, 16, 16), np.float32))[tuple(slice(0, s) for s in shape)]
    import scipy.ndimage as sndi            # host-side test data only
    return sndi.uniform_filter(big, 9) > 0.6


def emit(case, us, nbytes, rate, kernel, **extra):
    rec = {"case": case, "device_us": round(us, 1), "alg_bytes": int(nbytes), "frac_8TBs": round(nbytes / (us * 1e-6) / PEAK, 4),
           "copy_TBs": round(rate / 1e12, 3), "kernel": kernel}
    rec.update(extra)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    ca.set_device(0)
    rate = copy_rate(a.reps)
    rng = np.random.default_rng(0)
    labels_noise = None
    for name, x in (("smooth 512^3", smooth_mask((512,) * 3, 0)), ("noise30 512^3", rng.random((512,) * 3) > 0.7),
                    ("smooth 181x217x181", smooth_mask((181, 217, 181), 1))):
        xd = ca.asarray(x)
        out = ca.empty(x.shape, np.int32)
        us = timed(lambda: ndi.label(xd, output=out), a.reps)
        n = ndi.label(xd, output=out)
        emit("label " + name, us, x.size * 5, rate, ca.last_kernel(), num_features=n)
        if name.startswith("noise"):
            labels_noise, n_noise = out, n
    x4 = rng.random((64, 64, 64, 16)) > 0.7
    xd = ca.asarray(x4)
    out = ca.empty(x4.shape, np.int32)
    us = timed(lambda: ndi.label(xd, output=out), a.reps)
    emit("label 4-D 64x64x64x16 (generic)", us, x4.size * 5, rate, ca.last_kernel(), num_features=ndi.label(xd, output=out))

    vals = ca.asarray(rng.random((512,) * 3).astype(np.float32))
    few = ca.asarray(rng.integers(0, 16, (512,) * 3).astype(np.int32))
    idx16 = np.arange(1, 16)
    nvox = 512 ** 3
    us = timed(lambda: ndi.sum_labels(vals, few, idx16), a.reps)
    emit("sum_labels f32, 15 labels", us, nvox * 8, rate, ca.last_kernel())
    us = timed(lambda: ndi.center_of_mass(vals, few, idx16), a.reps)
    emit("center_of_mass f32, 15 labels", us, nvox * 8, rate, ca.last_kernel())
    idx_many = ca.asarray(np.arange(1, n_noise + 1, dtype=np.int64))
    us = timed(lambda: ndi.sum_labels(vals, labels_noise, idx_many), a.reps)
    emit("sum_labels f32, %d labels" % n_noise, us, nvox * 8, rate, ca.last_kernel())
    # the device part (the public function then builds 7.7 M host tuples, which is Python time)
    us = timed(lambda: meas._reduce(meas._OPS["com"], vals, labels_noise, idx_many), a.reps)
    emit("center_of_mass f32, %d labels (device result)" % n_noise, us, nvox * 8, rate, ca.last_kernel())
    k1000 = ca.asarray(rng.integers(0, 1001, (512,) * 3).astype(np.int32))
    idx1000 = np.arange(1, 1001)
    us = timed(lambda: ndi.minimum_position(vals, k1000, idx1000), a.reps)
    emit("minimum_position f32, 1000 labels", us, nvox * 8 * 2, rate, ca.last_kernel())


if __name__ == "__main__":
    main()
