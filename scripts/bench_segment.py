"""find_boundaries, map_array / relabel_sequential and unique (csrc/segment.hip) at the sizes a segmentation pipeline runs: one JSON
line per case with the device time (median, smallest and largest of event-timed repetitions), against the same run's float4
copy kernel moving the bytes the operation must move (find_boundaries: itemsize + 1 bytes a voxel).  `*_us` of a public call
holds the Python layer of that call; `*_kernel*_us` is the library called on ready descriptors, 20 calls between two events.

  * find_boundaries thick / outer on a 4096^2 and a 256^3 int32 `label` result: the fused LDS-tile route against the generic
    one-thread-per-voxel route of the same build (mi_debug_set_boundaries), alternated;
  * map_array on 4096^2 int32 voxels at 10^2, 10^4 and 10^6 keys over every route that can hold them (the figures behind
    TABLE_MAX_RANGE and LDS_MAX_RANGE of cupyimg_amd/skimage/util/_map_array.py), dense keys and keys spread over 2^24 values,
    and relabel_sequential at the same label counts;
  * unique on 10^7 int32 labels against `sort` alone.
-> profiles/segment.txt

    python scripts/bench_segment.py [--reps 7] > profiles/segment.txt
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
from cupyimg_amd.skimage import segmentation as seg  # noqa: E402
from cupyimg_amd.skimage import util  # noqa: E402
from cupyimg_amd.skimage.util import _map_array  # noqa: E402


BURST = 20


def timed(fn, reps):
    """(median, min, max) device microseconds of `reps` event-timed calls after two warm-up calls"""
    fn()
    fn()
    ts = []
    for _ in range(reps):
        a, b = ca.Event(), ca.Event()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_ms(b) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def copy_us(nbytes, reps):
    """the float4 copy kernel moving `nbytes` in all (half read, half written)"""
    n = max(int(nbytes) // 8, 1024)
    src, dst = ca.empty((n,), np.float32), ca.empty((n,), np.float32)
    fn = _lib.load().mi_debug_copy_f32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    return timed(lambda: fn(src.ptr, dst.ptr, n, 4096, None), reps)[0]


def stats(prefix, t):
    return {prefix + "_us": round(t[0], 1), prefix + "_min_us": round(t[1], 1), prefix + "_max_us": round(t[2], 1)}


def smooth_mask(shape, seed):
    rng = np.random.default_rng(seed)
    small = rng.standard_normal(tuple(-(-s // 16) for s in shape)).astype(np.float32)
    big = np.kron(small, np.ones((16,) * len(shape), np.float32))[tuple(slice(0, s) for s in shape)]
    import scipy.ndimage as sndi            # host-side test data only
    return sndi.uniform_filter(big, 9) > 0.6


def bench_boundaries(reps):
    knob = _lib.load().mi_debug_set_boundaries
    knob.argtypes = [ctypes.c_int] * 2
    for name, shape in (("4096x4096", (4096, 4096)), ("256x256x256", (256, 256, 256))):
        labels, n = ndi.label(ca.asarray(smooth_mask(shape, len(shape))))
        nbytes = labels.size * (labels.itemsize + 1)
        for mode in ("thick", "outer"):
            rec = {"case": "find_boundaries {} {} int32".format(mode, name), "regions": int(n), "bytes_moved": nbytes}
            knob(0, 0)
            fused = seg.find_boundaries(labels, mode=mode)
            rec["fused_kernel"] = ca.last_kernel()[:120]
            knob(0, 1)
            generic = seg.find_boundaries(labels, mode=mode)
            rec["generic_kernel"] = ca.last_kernel()[:120]
            rec["routes_agree"] = not ca.arrays_differ(fused, generic)
            rec["boundary_fraction"] = round(ca.count_nonzero(fused) / labels.size, 4)
            for rnd in range(2):                   # the two routes alternated, twice
                knob(0, 0)
                rec.update(stats("fused_round{}".format(rnd), timed(lambda: seg.find_boundaries(labels, mode=mode), reps)))
                knob(0, 1)
                rec.update(stats("generic_round{}".format(rnd), timed(lambda: seg.find_boundaries(labels, mode=mode), reps)))
            # the kernels alone: the library called on ready descriptors, BURST launches between two events (a public call
            # spends tens of microseconds in Python, during which a kernel this short has already finished)
            lib = _lib.load()
            ld, od = labels._desc(), fused._desc()
            code = {"thick": 0, "outer": 2}[mode]

            def burst():
                for _ in range(BURST):
                    lib.mi_find_boundaries(ctypes.byref(ld), 1, code, 1, 0, ctypes.byref(od), None)
            for rnd in range(2):
                knob(0, 0)
                rec.update({k: round(v / BURST, 1) for k, v in stats("fused_kernel_round{}".format(rnd), timed(burst, reps)).items()})
                knob(0, 1)
                rec.update({k: round(v / BURST, 1) for k, v in stats("generic_kernel_round{}".format(rnd), timed(burst, reps)).items()})
            knob(0, 0)
            rec["copy_us"] = round(copy_us(nbytes, reps), 1)
            best = lambda key: min(rec[key.format(0)], rec[key.format(1)])
            rec["fused_kernel_over_copy"] = round(best("fused_kernel_round{}_us") / rec["copy_us"], 2)
            rec["generic_over_fused_kernel"] = round(best("generic_kernel_round{}_us") / best("fused_kernel_round{}_us"), 2)
            rec["generic_over_fused_call"] = round(best("generic_round{}_us") / best("fused_round{}_us"), 2)
            print(json.dumps(rec), flush=True)


def bench_map_array(reps):
    shape = (4096, 4096)
    rng = np.random.default_rng(5)
    for nkeys in (100, 10000, 1000000):
        for spread, span in (("dense", nkeys), ("spread", max(nkeys, 1 << 24))):
            keys_h = rng.permutation(span)[:nkeys].astype(np.int32) if spread == "spread" else rng.permutation(nkeys).astype(np.int32)
            voxels = ca.asarray(keys_h[rng.integers(0, nkeys, size=shape)])
            keys, vals = ca.asarray(keys_h), ca.asarray(np.arange(1, nkeys + 1, dtype=np.int32))
            out = ca.empty(shape, np.int32)
            rec = {"case": "map_array 4096x4096 int32, {} {} keys".format(nkeys, spread), "key_range": int(keys_h.max()) - int(keys_h.min()) + 1}
            routes = ["search", "table"] + (["table_lds"] if rec["key_range"] <= 16384 else [])
            want = None
            for rnd in range(2):
                for r in routes:
                    _map_array.set_route(r)
                    util.map_array(voxels, keys, vals, out=out)
                    if want is None:
                        want = out.copy()
                    elif ca.arrays_differ(out, want):
                        rec["routes_agree"] = False
                    rec.update(stats("{}_round{}".format(r, rnd), timed(lambda: util.map_array(voxels, keys, vals, out=out), reps)))
            rec.setdefault("routes_agree", True)
            # the library alone on ready descriptors, BURST calls between two events: the table routes with their fill and
            # atomicMin launches, the search without the sort of the keys (timed on its own)
            lib = _lib.load()
            lo, hi = _map_array._key_range(keys)
            kmin, span = _map_array._ordered(lo, keys.dtype), hi - lo + 1
            perm, srt = ca.core._argsort(keys, False, True, True)
            ind, kd, vd, od = voxels.reshape(-1)._desc(), keys._desc(), vals._desc(), out.reshape(-1)._desc()
            sd, pd = srt._desc(), perm._desc()
            calls = {"search": lambda: lib.mi_map_array_search(ctypes.byref(ind), ctypes.byref(sd), ctypes.byref(pd), ctypes.byref(vd), ctypes.byref(od), None),
                     "table": lambda: lib.mi_map_array_table(ctypes.byref(ind), ctypes.byref(kd), ctypes.byref(vd), ctypes.byref(od), kmin, span, 0, None),
                     "table_lds": lambda: lib.mi_map_array_table(ctypes.byref(ind), ctypes.byref(kd), ctypes.byref(vd), ctypes.byref(od), kmin, span, 1, None)}
            for rnd in range(2):
                for r in routes:
                    def burst(call=calls[r]):
                        for _ in range(BURST):
                            call()
                    rec.update({k: round(v / BURST, 1) for k, v in stats("{}_kernels_round{}".format(r, rnd), timed(burst, max(3, reps // 2))).items()})
            rec.update(stats("sort_keys", timed(lambda: ca.core._argsort(keys, False, True, True), reps)))
            _map_array.set_route("auto")
            util.map_array(voxels, keys, vals, out=out)
            rec["auto_kernel"] = ca.last_kernel()[:100]
            rec["copy_us"] = round(copy_us(voxels.nbytes * 2, reps), 1)
            print(json.dumps(rec), flush=True)
        # relabel_sequential of a field with `nkeys` labels spread over a range ten times as wide (holes in the numbering)
        field = ca.asarray((rng.permutation(10 * nkeys)[:nkeys].astype(np.int32) + 1)[rng.integers(0, nkeys, size=shape)])
        rec = {"case": "relabel_sequential 4096x4096 int32, {} labels".format(nkeys)}
        rec.update(stats("relabel", timed(lambda: seg.relabel_sequential(field), max(3, reps // 2))))
        rec.update(stats("unique", timed(lambda: ca.unique(field), max(3, reps // 2))))
        seg.relabel_sequential(field)
        rec["map_kernel"] = ca.last_kernel()[:100]
        print(json.dumps(rec), flush=True)


def bench_unique(reps):
    n = 10 ** 7
    rng = np.random.default_rng(6)
    labels = ca.asarray(rng.integers(0, 10 ** 5, size=n).astype(np.int32))
    rec = {"case": "unique, int32, 10000000 labels of 100000 values"}
    rec.update(stats("sort", timed(lambda: ca.sort(labels), reps)))
    rec.update(stats("unique", timed(lambda: ca.unique(labels), reps)))
    rec.update(stats("unique_all", timed(lambda: ca.unique(labels, True, True, True), reps)))
    rec["copy_us"] = round(copy_us(8 * n, reps), 1)
    rec["unique_over_sort"] = round(rec["unique_us"] / rec["sort_us"], 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["boundaries", "map_array", "unique"], default=None)
    a = ap.parse_args()
    ca.set_device(0)
    print(json.dumps({"device": ca.device_name(), "reps": a.reps}), flush=True)
    if a.only in (None, "boundaries"):
        bench_boundaries(a.reps)
    if a.only in (None, "map_array"):
        bench_map_array(a.reps)
    if a.only in (None, "unique"):
        bench_unique(a.reps)


if __name__ == "__main__":
    main()
