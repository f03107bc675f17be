"""Host transcription of the reference's peak_local_max without labels (cupyimg/skimage/feature/peak.py), of ensure_spacing
(cupyimg/skimage/_shared/coord.py) and of the greedy loop of corner_peaks (cupyimg/skimage/feature/corner.py:909-953), on
NumPy / SciPy, plus the round-based greedy the device runs, in NumPy.

One thing is pinned down that the reference leaves open: candidates are ordered by `np.argsort(-values, kind="stable")`, so
ties come in raster order (the reference's tie order is whatever cupy.argsort gives)."""
import numpy as np
import scipy.ndimage as sndi
from scipy.spatial import cKDTree, distance


def ensure_spacing(coord, spacing=1, p_norm=np.inf):
    """_shared/coord.py:7-58: every point not yet rejected rejects the points closer than `spacing`"""
    coord = np.asarray(coord)
    if not len(coord):
        return coord
    tree = cKDTree(coord)
    indices = tree.query_ball_point(coord, r=spacing, p=p_norm)
    rejected = set()
    for idx, candidates in enumerate(indices):
        if idx not in rejected:
            candidates = list(candidates)
            candidates.remove(idx)
            dist = distance.cdist([coord[idx]], coord[candidates], distance.minkowski, p=p_norm).reshape(-1)
            rejected.update(c for c, d in zip(candidates, dist) if d < spacing)
    return np.delete(coord, tuple(rejected), axis=0)


def corner_spacing(coords, min_distance=1, p_norm=np.inf):
    """corner.py:925-945 (before `[:num_peaks]`): every point not yet rejected rejects the points within `min_distance`"""
    coords = np.asarray(coords)
    if not len(coords):
        return coords
    tree = cKDTree(coords)
    rejected = set()
    for idx, point in enumerate(coords):
        if idx not in rejected:
            candidates = tree.query_ball_point(point, r=min_distance, p=p_norm)
            candidates.remove(idx)
            rejected.update(candidates)
    return np.delete(coords, tuple(rejected), axis=0)


def integer_distance(delta, p_norm):
    """the device's distance of an integer offset: max |d| (inf), sum |d| (1), sum d^2 (2: compared with spacing^2)"""
    delta = np.abs(np.asarray(delta, dtype=np.int64))
    if p_norm == np.inf:
        return delta.max(axis=-1)
    if p_norm == 1:
        return delta.sum(axis=-1)
    if p_norm == 2:
        return (delta * delta).sum(axis=-1)
    raise ValueError(p_norm)


def conflicts(coords, spacing, p_norm, inclusive):
    """(K, K) bool: the pairs of distinct points the integer rule holds to be too close"""
    coords = np.asarray(coords, dtype=np.int64)
    dist = integer_distance(coords[:, None, :] - coords[None, :, :], p_norm)
    limit = spacing * spacing if p_norm == 2 else spacing
    out = dist <= limit if inclusive else dist < limit
    np.fill_diagonal(out, False)
    return out


def greedy_rounds(coords, spacing, p_norm=np.inf, inclusive=False):
    """(kept points in order, rounds): a live point is kept when no live point of lower rank conflicts with it, live points
    in conflict with a kept one are rejected, until no point is live"""
    coords = np.asarray(coords, dtype=np.int64)
    k = len(coords)
    if not k:
        return coords, 0
    c = conflicts(coords, spacing, p_norm, inclusive)
    lower = np.tril(np.ones((k, k), bool), -1)          # lower[i, j]: j < i
    live, kept = np.ones(k, bool), np.zeros(k, bool)
    rounds = 0
    while live.any():
        rounds += 1
        assert rounds <= k
        new = live & ~(c & lower & live[None, :]).any(axis=1)
        kept |= new
        live &= ~new
        live &= ~(c & kept[None, :]).any(axis=1)
    return coords[kept], rounds


def get_threshold(image, threshold_abs, threshold_rel):
    threshold = threshold_abs if threshold_abs is not None else image.min()
    if threshold_rel is not None:
        threshold = max(threshold, threshold_rel * float(image.max()))
    return float(threshold)


def excluded_border_width(ndim, min_distance, exclude_border):
    if isinstance(exclude_border, bool):
        return (min_distance if exclude_border else 0,) * ndim
    if isinstance(exclude_border, int):
        if exclude_border < 0:
            raise ValueError("`exclude_border` cannot be a negative value")
        return (exclude_border,) * ndim
    if isinstance(exclude_border, tuple):
        if len(exclude_border) != ndim:
            raise ValueError("`exclude_border` should have the same length as the dimensionality of the image.")
        for exclude in exclude_border:
            if not isinstance(exclude, int):
                raise ValueError("`exclude_border`, when expressed as a tuple, must only contain ints.")
            if exclude < 0:
                raise ValueError("`exclude_border` can not be a negative value")
        return exclude_border
    raise TypeError("`exclude_border` must be bool, int, or tuple")


def peak_mask(image, footprint, threshold):
    """peak.py:37-60 without a mask"""
    if footprint.size == 1 or image.size == 1:
        return image > threshold
    image_max = sndi.maximum_filter(image, footprint=footprint, mode="constant")
    out = image == image_max
    if np.all(out):
        out[:] = False
    out &= image > threshold
    return out


def peak_local_max(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, indices=True, num_peaks=np.inf,
                   footprint=None, p_norm=np.inf):
    image = np.asarray(image)
    border_width = excluded_border_width(image.ndim, min_distance, exclude_border)
    threshold = get_threshold(image, threshold_abs, threshold_rel)
    if footprint is None:
        footprint = np.ones((2 * min_distance + 1,) * image.ndim, dtype=bool)
    else:
        footprint = np.asarray(footprint)
    mask = peak_mask(image, footprint, threshold)
    for i, width in enumerate(border_width):
        if width == 0:
            continue
        mask[(slice(None),) * i + (slice(None, width),)] = 0
        mask[(slice(None),) * i + (slice(-width, None),)] = 0
    coord = np.nonzero(mask)
    intensities = image[coord]
    order = np.argsort(-intensities, kind="stable")
    coord = np.column_stack(coord)[order].astype(np.int64).reshape(-1, image.ndim)
    coord = ensure_spacing(coord, spacing=min_distance, p_norm=p_norm)
    if len(coord) > num_peaks:
        coord = coord[:num_peaks]
    if indices:
        return coord
    out = np.zeros(image.shape, dtype=bool)
    out[tuple(coord.T)] = True
    return out


def corner_peaks(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, indices=True, num_peaks=np.inf,
                 footprint=None, p_norm=np.inf):
    image = np.asarray(image)
    if np.isinf(num_peaks):
        num_peaks = None
    coords = peak_local_max(image, min_distance=min_distance, threshold_abs=threshold_abs, threshold_rel=threshold_rel,
                            exclude_border=exclude_border, num_peaks=np.inf, footprint=footprint)
    coords = corner_spacing(coords, min_distance, p_norm)[:num_peaks]
    if indices:
        return coords
    peaks = np.zeros(image.shape, dtype=bool)
    peaks[tuple(coords.T)] = True
    return peaks


# ------------------------------------------------------------------ tests/golden/peak_kat.json (format: make_peak_kat.py)
def _kat_index(index):
    return tuple(slice(*e) if isinstance(e, list) else e for e in index)


def kat_image(spec):
    image = np.full(spec["shape"], spec["fill"], dtype=spec["dtype"])
    for index, value in spec.get("pre", ()):
        image[_kat_index(index)] = value
    if spec.get("noise"):
        image = image + np.random.RandomState(spec["noise"]["seed"]).uniform(size=image.shape) * spec["noise"]["scale"]
    for index, value in spec.get("set", ()):
        image[_kat_index(index)] = np.arange(value["arange"]) if isinstance(value, dict) else value
    return image


def kat_kwargs(kwargs):
    out = dict(kwargs)
    if isinstance(out.get("exclude_border"), list):
        out["exclude_border"] = tuple(out["exclude_border"])
    if isinstance(out.get("footprint"), dict):
        out["footprint"] = np.ones(out["footprint"]["ones"], bool)
    return out


def kat_check(result, expect, image):
    """`result` (a host array) meets what the reference's test states"""
    result = np.asarray(result)
    for key, want in expect.items():
        if key == "size":
            assert result.size == want
        elif key == "len":
            assert len(result) == want, (len(result), want)
        elif key == "shape":
            assert list(result.shape) == want
        elif key == "coords":
            assert result.tolist() == want, (result.tolist(), want)
        elif key == "all_rows_equal":
            assert (result == np.asarray([want])).all()
        elif key == "sorted_coords":
            assert sorted(result.tolist()) == want
        elif key == "contains":
            assert all(w in result.tolist() for w in want)
        elif key == "subset_of":
            assert all(r in want for r in result.tolist())
        elif key == "mask_equals_image":
            assert result.dtype == bool and np.array_equal(result, image.astype(bool))
        elif key == "mask_true_at":
            mask = np.zeros(image.shape, bool)
            mask[tuple(np.array(want).T)] = True
            assert result.dtype == bool and np.array_equal(result, mask)
        elif key == "all_true":
            assert result.dtype == bool and result.shape == image.shape and result.all()
        elif key not in ("warns", "raises"):
            raise KeyError(key)


def squared_dot_image():
    """the image of the reference's test_squared_dot (test_corner.py:459-462): a 4 x 4 square of ones on 50 x 50 zeros"""
    im = np.zeros((50, 50))
    im[4:8, 4:8] = 1
    return im
