"""Host reference of skimage.morphology.reconstruction, independent of the code under test, and the input builders of the
reconstruction tests.

`reconstruct` iterates the defining rule with scipy.ndimage until nothing changes:

    R <- minimum(mask, maximum(R, grey_dilation(R, footprint)))          (erosion: the mirror image)

with the footprint padded so that its centre sits at `offset`, mode="constant" and cval = the current minimum (maximum),
which never raises (lowers) anything: neighbours outside the image contribute nothing.  The operator is monotone and only
compares and copies values, so the fixed point is unique and any correct implementation reproduces it bit for bit.
scipy.ndimage's footprint filters compute in float64, which cannot hold every 64-bit integer: for int64 / uint64 the same
neighbourhood maximum (minimum) is taken with NumPy over shifted views of the padded array."""
import zlib

import numpy as np
import scipy.ndimage as sndi


def centred_footprint(selem, offset):
    """`selem` (centre cell removed) inside the smallest odd-sided array whose geometric centre is the cell `offset`."""
    selem = np.array(selem, dtype=bool)
    offset = [int(o) for o in offset]
    selem[tuple(offset)] = False
    half = [max(o, n - 1 - o) for o, n in zip(offset, selem.shape)]
    fp = np.zeros([2 * h + 1 for h in half], bool)
    fp[tuple(slice(h - o, h - o + n) for h, o, n in zip(half, offset, selem.shape))] = selem
    return fp


def _neighbour_extreme(r, fp, dilation):
    """max (min) over the true cells t of fp (centre c) of r[q - (t - c)], outside the array: nothing"""
    if not (r.dtype.kind in "iu" and r.dtype.itemsize == 8):
        if dilation:
            return sndi.grey_dilation(r, footprint=fp, mode="constant", cval=r.min())
        return sndi.grey_erosion(r, footprint=fp[(slice(None, None, -1),) * fp.ndim], mode="constant", cval=r.max())
    half = [n // 2 for n in fp.shape]
    padded = np.pad(r, [(h, h) for h in half], mode="constant", constant_values=r.min() if dilation else r.max())
    out = r.copy()
    for t in zip(*np.nonzero(fp)):
        view = padded[tuple(slice(2 * h - ti, 2 * h - ti + n) for h, ti, n in zip(half, t, r.shape))]
        out = np.maximum(out, view) if dilation else np.minimum(out, view)
    return out


def reconstruct(seed, mask, method="dilation", selem=None, offset=None, max_iter=None):
    seed = np.asarray(seed)
    mask = np.asarray(mask)
    dtype = np.promote_types(seed.dtype, mask.dtype)
    r = seed.astype(dtype)
    m = mask.astype(dtype)
    if selem is None:
        selem = np.ones((3,) * r.ndim, bool)
    selem = np.asarray(selem).astype(bool)
    if offset is None:
        offset = [n // 2 for n in selem.shape]
    fp = centred_footprint(selem, offset)
    as_bool = dtype == np.bool_
    if as_bool:
        r, m = r.astype(np.uint8), m.astype(np.uint8)
    elif dtype == np.float16:           # scipy.ndimage has no float16; float32 holds every float16 value
        r, m = r.astype(np.float32), m.astype(np.float32)
    n = 0
    while True:
        if not fp.any():
            break
        if method == "dilation":
            nxt = np.minimum(m, np.maximum(r, _neighbour_extreme(r, fp, True)))
        else:
            nxt = np.maximum(m, np.minimum(r, _neighbour_extreme(r, fp, False)))
        n += 1
        if np.array_equal(nxt, r):
            break
        r = nxt
        if max_iter is not None and n >= max_iter:
            raise RuntimeError("no fixed point after {} iterations".format(n))
    return r.astype(dtype)


# ---------------------------------------------------------------- input builders
def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def extreme(dtype, method):
    """the value that never spreads: the lowest of the dtype for dilation, the highest for erosion (finite for floats)"""
    dtype = np.dtype(dtype)
    info = np.finfo(dtype) if dtype.kind == "f" else np.iinfo(dtype)
    return dtype.type(info.min if method == "dilation" else info.max)


def plateau_input(shape, dtype, method, rng):
    """mask = random integers 0 .. 7, seed = mask on 2 % of the voxels and the extreme value elsewhere: plateaus of equal
    values along which the seeds travel far, across blocks (the highest / lowest voxel of the mask is always a seed, so
    that something spreads in the smallest arrays too)"""
    mask = rng.integers(0, 8, size=shape).astype(dtype)
    seed = np.full(shape, extreme(dtype, method), dtype)
    pick = rng.random(shape) < 0.02
    pick.flat[mask.argmax() if method == "dilation" else mask.argmin()] = True
    seed[pick] = mask[pick]
    return seed, mask


def hdome_input(shape, dtype, method, rng):
    """smooth mask (Gaussian-filtered noise, sigma 3, stretched over the dtype's middle range), seed = mask -/+ h"""
    dtype = np.dtype(dtype)
    g = sndi.gaussian_filter(rng.standard_normal(shape), 3.0, mode="nearest")
    g = (g - g.min()) / max(g.max() - g.min(), 1e-30)
    if dtype.kind == "f":
        mask = (g * 100.0).astype(dtype)
        h = dtype.type(7.5)
    else:
        span = 200 if dtype.itemsize == 1 else 20000
        h = dtype.type(span // 12)
        base = 2 * int(h) if dtype.kind == "u" else -span // 2         # seed = mask -/+ h stays inside the dtype
        mask = (base + np.round(g * span)).astype(dtype)
    seed = (mask - h if method == "dilation" else mask + h).astype(dtype)
    return seed, mask


def serpentine(shape, wall=0, corridor=200, start=150, dtype=np.uint8):
    """A one-voxel corridor snaking through the rows of the middle plane of a 3-D volume: every second row over its whole
    length, joined at alternating ends by one voxel of the row between, and one last voxel stepping out of the plane at
    the far end.  Returns (seed, mask, path): `path` lists the corridor's voxels in order -- consecutive entries are face
    neighbours and no other two are, so the geodesic distance from the first to the last voxel under the
    connectivity-1 element is len(path) - 1 steps.  mask = `corridor` on the path and `wall` elsewhere; seed = `start` on
    the first voxel and `wall` elsewhere: reconstruction by dilation sets exactly the path to `start`."""
    nz, ny, nx = shape
    if nz < 2 or ny < 2 or nx < 2:
        raise ValueError("the serpentine needs at least two voxels along every axis")
    z = nz // 2 if nz // 2 + 1 < nz else 0
    path = []
    forward = True
    rows = list(range(0, ny, 2))
    for k, y in enumerate(rows):
        xs = range(nx) if forward else range(nx - 1, -1, -1)
        path.extend((z, y, x) for x in xs)
        end = nx - 1 if forward else 0
        if k + 1 < len(rows):
            path.append((z, y + 1, end))
        else:
            path.append((z + 1, y, end))
        forward = not forward
    mask = np.full(shape, wall, dtype)
    seed = np.full(shape, wall, dtype)
    idx = tuple(np.array(path).T)
    mask[idx] = corridor
    seed[path[0]] = start
    return seed, mask, path
