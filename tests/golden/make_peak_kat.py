"""Writes tests/golden/peak_kat.json: the literal inputs and the stated expectations of the reference's label-free
peak_local_max tests (cupyimg/skimage/feature/tests/test_peak.py) and of its peak-counting corner tests that need no
skimage.data image (cupyimg/skimage/feature/tests/test_corner.py:399-476), as data, each with its file:line.  Nothing here
calls the library or the reference; the expectations are the ones the reference's tests state.

An image is {"shape", "dtype", "fill", "pre": [[index, value], ...], "noise": {"seed", "scale"}, "set": [[index, value], ...]}:
`fill` everywhere, the entries of `pre` assigned, uniform noise in [0, scale) from numpy.random.RandomState(seed) added (the
reference's noisy cases draw from the legacy global generator after seeding it; they are stored with a generator of their own
and the same seed), then the entries of `set` assigned (an index entry may be [start, stop] or [start, stop, step] for a
slice; a value may be {"arange": n}).  "detector" names the corner function the
image goes through first.  tests/helpers/peak_ref.py (`kat_image`, `kat_check`) reads this format.

The squared dot of test_corner.py:459-476 states `(results == [[6, 6]]).all()`, which an empty result meets (the square lies
inside the border that min_distance=10 excludes): it is stored as "all_rows_equal", literally.

Left out: every case with labels= (out of scope: NotImplementedError), _prominent_peaks, and the skimage.data images.

    python tests/golden/make_peak_kat.py
"""
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def image(shape, dtype="float64", fill=0, set=(), noise=None, pre=()):
    return dict(shape=list(shape), dtype=dtype, fill=fill, pre=[list(e) for e in pre], noise=noise, set=[list(e) for e in set])


def main():
    cases = []

    def add(name, ref, img, kwargs, **expect):
        cases.append(dict(name=name, ref=ref, image=img, kwargs=kwargs, expect=expect))

    T = "test_peak.py:"
    add("trivial", T + "19-23", image((25, 25)), dict(min_distance=1), size=0)
    add("trivial_mask", T + "24-26", image((25, 25)), dict(min_distance=1, indices=False), warns="indices argument is deprecated",
        mask_equals_image=True)
    peaks4 = [[7, 7], [7, 13], [13, 7], [13, 13]]
    add("noisy_peaks", T + "28-40", image((20, 20), set=[[p, 1] for p in peaks4], noise=dict(seed=21, scale=0.8)), dict(min_distance=5),
        len=4, subset_of=peaks4)
    two = [[[1, 1], 10], [[3, 3], 20]]
    add("relative_threshold", T + "42-48", image((5, 5), "uint8", set=two), dict(min_distance=1, threshold_rel=0.5), coords=[[3, 3]])
    add("absolute_threshold", T + "50-56", image((5, 5), "uint8", set=two), dict(min_distance=1, threshold_abs=10), coords=[[3, 3]])
    add("constant_image", T + "58-61", image((20, 20), "uint8", fill=128), dict(min_distance=1), len=0)
    add("flat_peak", T + "63-67", image((5, 5), "uint8", set=[[[[1, 3], [1, 3]], 10]]), dict(min_distance=1), len=4)
    add("sorted_peaks_uint8", T + "69-74", image((5, 5), "uint8", set=[[[1, 1], 20], [[3, 3], 10]]), dict(min_distance=1), coords=[[1, 1], [3, 3]])
    add("sorted_peaks_row", T + "76-86", image((3, 10), set=[[[1, 1], 1], [[1, 3], 2], [[1, 5], 3], [[1, 7], 4]]), dict(min_distance=1),
        coords=[[1, 7], [1, 5], [1, 3], [1, 1]])
    five = [[[1, 1], 10], [[1, 3], 11], [[1, 5], 12], [[3, 5], 8], [[5, 3], 7]]
    add("num_peaks_all", T + "88-98", image((7, 7), "uint8", set=five), dict(min_distance=1, threshold_abs=0), len=5)
    add("num_peaks_2", T + "99-105", image((7, 7), "uint8", set=five), dict(min_distance=1, threshold_abs=0, num_peaks=2), len=2,
        contains=[[1, 3], [1, 5]])
    add("num_peaks_4", T + "107-116", image((7, 7), "uint8", set=five), dict(min_distance=1, threshold_abs=0, num_peaks=4), len=4,
        contains=[[1, 3], [1, 5], [1, 1], [3, 5]])
    add("num_peaks3D", T + "168-174", image((10, 10, 100), set=[[[5, 5, [0, 100, 5]], dict(arange=20)]]), dict(min_distance=1, num_peaks=2), len=2)
    add("ndarray_indices_false", T + "227-232", image((5, 5, 5), set=[[[2, 2, 2], 1]]), dict(min_distance=1, indices=False),
        warns="indices argument is deprecated", mask_equals_image=True)
    nd = [[[1, 0, 0], 1], [[0, 1, 0], 1], [[0, 0, 1], 1], [[3, 0, 0], 1], [[2, 2, 2], 1]]
    for tag, border in (("2", 2), ("true", True)):
        add("ndarray_exclude_border_" + tag, T + "234-259", image((5, 5, 5), set=nd), dict(min_distance=2, exclude_border=border, indices=False),
            warns="indices argument is deprecated", mask_true_at=[[2, 2, 2]])
    for tag, border in (("0", 0), ("false", False)):
        add("ndarray_exclude_border_" + tag, T + "260-277", image((5, 5, 5), set=nd), dict(min_distance=2, exclude_border=border, indices=False),
            warns="indices argument is deprecated", mask_true_at=[[2, 2, 2], [0, 0, 1], [3, 0, 0]])
    add("ndarray_no_border_default_distance", T + "278-283", image((5, 5, 5), set=nd), dict(exclude_border=False, indices=False),
        warns="indices argument is deprecated", mask_equals_image=True)
    add("empty_non2d_indices", T + "300-309", image((10, 10, 10)), dict(footprint=dict(ones=[3, 3, 3]), min_distance=1, threshold_rel=0, exclude_border=False),
        shape=[0, 3])
    add("disk", T + "457-482", image((10, 20), noise=dict(seed=21, scale=1.0)), dict(footprint=dict(ones=[1, 1]), threshold_abs=-1, indices=False, exclude_border=False),
        warns="indices argument is deprecated", all_true=True)
    for ndim, ref in ((3, T + "484-503"), (4, T + "505-524")):
        img = image((30,) * ndim, set=[[[15] * ndim, 1], [[5] * ndim, 1]])
        add("{}D_distance_10".format(ndim), ref, img, dict(min_distance=10, threshold_rel=0), coords=[[15] * ndim])
        add("{}D_distance_6".format(ndim), ref, img, dict(min_distance=6, threshold_rel=0), coords=[[15] * ndim])
        add("{}D_distance_10_no_border".format(ndim), ref, img, dict(min_distance=10, threshold_rel=0, exclude_border=False),
            sorted_coords=[[5] * ndim, [15] * ndim])
        add("{}D_distance_5".format(ndim), ref, img, dict(min_distance=5, threshold_rel=0), sorted_coords=[[5] * ndim, [15] * ndim])
    add("threshold_rel_default_flat", T + "526-530", image((5, 5), fill=1), {}, len=0)
    add("threshold_rel_default_peak", T + "532-533", image((5, 5), fill=1, set=[[[2, 2], 2]]), {}, coords=[[2, 2]])
    add("threshold_rel_default_distance_0", T + "535-540", image((5, 5), fill=1, set=[[[2, 2], 0]]), dict(min_distance=0), warns="When min_distance < 1",
        len=24)
    for r, c in itertools.product(range(5), range(5)):
        img = image((5, 5), set=[[[r, c], 1]])
        ref = T + "543-586"
        tag = "exclude_border_{}{}_".format(r, c)
        add(tag + "false", ref, img, dict(exclude_border=False), len=1)
        add(tag + "0", ref, img, dict(exclude_border=0), len=1)
        add(tag + "true", ref, img, dict(min_distance=1, exclude_border=True), len=0 if r in (0, 4) or c in (0, 4) else 1)
        add(tag + "10", ref, img, dict(exclude_border=[1, 0]), len=0 if r in (0, 4) else 1)
        add(tag + "01", ref, img, dict(exclude_border=[0, 1]), len=0 if c in (0, 4) else 1)
    E = T + "589-612"
    add("exclude_border_wrong_cardinality", E, image((5, 5)), dict(exclude_border=[1]), raises="ValueError")
    add("exclude_border_float", E, image((5, 5)), dict(exclude_border=1.0), raises="TypeError")
    add("exclude_border_non_integer", E, image((5, 5)), dict(exclude_border=[1, "a"]), raises="ValueError")
    add("exclude_border_negative_in_tuple", E, image((5, 5)), dict(exclude_border=[1, -1]), raises="ValueError")
    add("exclude_border_negative", E, image((5, 5)), dict(exclude_border=-1), raises="ValueError")

    C = "test_corner.py:"
    square = image((50, 50), set=[[[[0, 25], [0, 25]], 1.0]])
    noisy = image((50, 50), pre=[[[[0, 25], [0, 25]], 1.0]], noise=dict(seed=1234, scale=0.2))
    for name, ref, img in (("square_image", C + "399-427", square), ("noisy_square_image", C + "430-456", noisy)):
        for det, dk in (("corner_harris", dict(method="k")), ("corner_harris", dict(method="eps")),
                        ("corner_shi_tomasi", dict(sigma=1.5) if name.startswith("noisy") else {})):
            cases.append(dict(name="{}_{}_{}".format(name, det, dk.get("method", "")), ref=ref, image=img, detector=det, detector_kwargs=dk,
                              kwargs=dict(min_distance=10, threshold_rel=0), expect=dict(len=1)))
    dot = image((50, 50), set=[[[[4, 8], [4, 8]], 1]])
    for det in ("corner_harris", "corner_shi_tomasi"):
        cases.append(dict(name="squared_dot_" + det, ref=C + "459-476", image=dot, detector=det, detector_kwargs={},
                          kwargs=dict(min_distance=10, threshold_rel=0), expect=dict(all_rows_equal=[6, 6])))
    kat = {"source": "cupyimg/skimage/feature/tests/test_peak.py, test_corner.py", "function": "peak_local_max", "cases": cases}
    with open(os.path.join(HERE, "peak_kat.json"), "w") as f:
        json.dump(kat, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
