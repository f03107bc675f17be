"""skimage.morphology.reconstruction (csrc/reconstruct.hip) on MRI-sized volumes: one JSON line per case with the time of
a WHOLE call (hipEvents around it, warm, median and spread of the repetitions), its number of launches, the kernel, and the
comparators taken in the same process from code that does not depend on the new kernel:
  (a) ndi.binary_propagation on the {0, 1} problem (the bit kernel: a floor, the grey kernel moves 8x the bytes);
  (b) T_step = one ndi.grey_dilation(size=3) of the same volume and dtype: the least one step of a
      one-voxel-per-launch loop could cost.
The condition: on a 256^3 serpentine whose geodesic length D is known by construction, the whole call takes less than
D x T_step by more than the spread of the repetitions.  -> profiles/reconstruction.txt

    python scripts/bench_reconstruction.py [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cupyimg_amd as ca  # noqa: E402
from cupyimg_amd.scipy import ndimage as ndi  # noqa: E402
from cupyimg_amd.skimage import morphology as morph  # noqa: E402


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


def smooth_volume(shape, seed):
    import scipy.ndimage as sndi            # host-side test data only
    g = sndi.gaussian_filter(np.random.default_rng(seed).standard_normal(shape).astype(np.float32), 4.0, mode="nearest")
    return ((g - g.min()) / (g.max() - g.min()) * 100.0).astype(np.float32)


def serpentine(n):
    """one-voxel corridor through every second row of the middle plane of an n^3 uint8 volume; returns seed, mask, D"""
    mask = np.zeros((n, n, n), np.uint8)
    z = n // 2
    mask[z, 0::2, :] = 200
    for k, y in enumerate(range(1, n - 1, 2)):
        mask[z, y, n - 1 if k % 2 == 0 else 0] = 200
    seed = np.zeros_like(mask)
    seed[z, 0, 0] = 150
    return seed, mask, int((mask == 200).sum()) - 1


def emit(**rec):
    print(json.dumps(rec), flush=True)


def run(case, seed, mask, reps, **kw):
    sd, md = ca.asarray(seed), ca.asarray(mask)
    us, spread = timed(lambda: morph.reconstruction(sd, md, **kw), reps)
    launches = morph.last_reconstruction_launches()
    kernel = ca.last_kernel()
    t_step, _ = timed(lambda: ndi.grey_dilation(md, size=3), reps)
    emit(case=case, call_us=round(us, 1), spread_us=round(spread, 1), launches=launches, us_per_launch=round(us / launches, 1),
         T_step_us=round(t_step, 1), call_over_T_step=round(us / t_step, 1), kernel=kernel)
    return us, spread, t_step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ca.set_device(0)
    cross = ndi.generate_binary_structure(3, 1)
    for shape in ((256, 256, 256), (181, 217, 181)):
        name = "x".join(map(str, shape))
        vol = smooth_volume(shape, 1)
        run("h-dome float32 " + name + " (seed = mask - 10, box)", vol - np.float32(10.0), vol, a.reps)
        img = np.clip(vol * 2.0, 0, 255).astype(np.uint8)
        seed = np.full(shape, 255, np.uint8)
        for ax in range(3):
            for side in (0, -1):
                idx = [slice(None)] * 3
                idx[ax] = side
                seed[tuple(idx)] = img[tuple(idx)]
        run("fill holes uint8 " + name + " (erosion, seed = max inside, box)", seed, img, a.reps, method="erosion")
    rng = np.random.default_rng(2)
    m = (smooth_volume((256,) * 3, 3) > 50.0)
    s = m & (rng.random(m.shape) < 0.0005)
    us, spread, _ = run("binary {0,1} uint8 256^3 (cross)", s.astype(np.uint8), m.astype(np.uint8), a.reps, selem=cross)
    sd, md = ca.asarray(s), ca.asarray(m)
    bp, bp_spread = timed(lambda: ndi.binary_propagation(sd, mask=md), a.reps)
    emit(case="comparator (a): ndi.binary_propagation on the same {0,1} problem", call_us=round(bp, 1), spread_us=round(bp_spread, 1),
         kernel=ca.last_kernel(), grey_over_bit=round(us / bp, 1))
    seed, mask, dist = serpentine(256)
    us, spread, t_step = run("serpentine uint8 256^3 (cross), D = %d" % dist, seed, mask, a.reps, selem=cross)
    emit(case="condition: call < D x T_step by more than the spread", D=dist, call_us=round(us, 1), spread_us=round(spread, 1),
         D_x_T_step_us=round(dist * t_step, 1), shortfall_us=round(dist * t_step - us, 1),
         holds=bool(dist * t_step - us > spread))


if __name__ == "__main__":
    main()
