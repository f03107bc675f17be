"""Writes tests/golden/rl_kat.json: known answers for skimage.restoration.richardson_lucy from a loop that shares no code with
this repository -- SciPy's own scipy.signal.convolve(..., "same", method="direct") with np.flip(psf), in float64.

    python tests/golden/make_rl_kat.py

Ranks 2 and 3 only (SciPy's 1-D path sums in another order).  SciPy's direct N-D convolution visits the taps in the order of the
contract and adds every product in float64, so its results are compared for equal bits (tests/test_richardson_lucy_yardstick.py);
the file was written with SciPy 1.15.3.  JSON floats are written with repr(), which round-trips every float64."""
import json
import os

import numpy as np
import scipy.signal as ssig

# (image shape, psf shape, iterations, clip, filter_epsilon, zero taps in the PSF)
CASES = [
    ((13, 67), (3, 5), 7, True, None, False),
    ((17, 30), (4, 5), 3, False, 1e-3, False),
    ((5, 7), (2, 3), 30, True, None, False),
    ((12, 30), (5, 5), 5, True, 0.2, True),
    ((6, 6), (9, 9), 2, False, None, False),
    ((5, 11, 23), (3, 4, 5), 2, True, 1e-3, False),
    ((3, 5, 7), (2, 2, 3), 4, False, 0.2, True),
]


def inputs(seed, shape, pshape, zero_taps):
    rng = np.random.default_rng(seed)
    psf = rng.random(pshape) + 0.05
    if zero_taps:
        psf[rng.random(pshape) < 0.3] = 0.0
        psf.flat[0] = 0.25
    psf /= psf.sum()
    image = rng.random(shape) * 1.5 + 0.05                  # bright enough that some results exceed 1
    image[tuple(slice(0, max(1, n // 3)) for n in shape)] *= 1e-4       # a dark corner: some c fall below filter_epsilon
    return image, psf


def loop(image, psf, iterations, clip, filter_epsilon):
    u = np.full(image.shape, 0.5)
    mirror = np.flip(psf)
    for _ in range(iterations):
        c = ssig.convolve(u, psf, "same", method="direct")
        r = image / c
        if filter_epsilon:
            r = np.where(c < filter_epsilon, 0.0, r)
        u = u * ssig.convolve(r, mirror, "same", method="direct")
    if clip:
        u[u > 1] = 1
        u[u < -1] = -1
    return u


def main():
    out = []
    for k, (shape, pshape, iterations, clip, eps, zero_taps) in enumerate(CASES):
        image, psf = inputs(4000 + k, shape, pshape, zero_taps)
        with np.errstate(all="ignore"):
            want = loop(image, psf, iterations, clip, eps)
        assert np.isfinite(want).all()
        out.append({"shape": list(shape), "psf_shape": list(pshape), "iterations": iterations, "clip": clip, "filter_epsilon": eps,
                    "image": image.ravel().tolist(), "psf": psf.ravel().tolist(), "want": want.ravel().tolist()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rl_kat.json")
    with open(path, "w") as f:
        json.dump(out, f)
        f.write("\n")


if __name__ == "__main__":
    main()
