"""Host references for cupyimg_amd.skimage.segmentation (boundaries, relabelling, joins) and skimage.util.map_array, written
from the behaviour of the reference (cupyimg/skimage/segmentation/boundaries.py, _join.py, cupyimg/skimage/util/_map_array.py)
with NumPy and SciPy: `dilation != erosion` with the masks, the subpixel loop with a `unique` per window, the first-match
search of map_array.  The closed forms the kernels evaluate (csrc/segment.hip) are here too, as NumPy, so that
tests/test_segment_yardstick.py can hold them against the transcriptions without a device."""
import itertools

import numpy as np
from scipy import ndimage as sndi


def _as_labels(label_img):
    label_img = np.asarray(label_img)
    return label_img.astype(np.uint8) if label_img.dtype == np.bool_ else label_img


# ------------------------------------------------------------------ transcriptions
def _grey(image, footprint, op):
    """scipy.ndimage.grey_dilation / grey_erosion(image, footprint=footprint) with the default mode="reflect" for a 3^ndim
    footprint, in the image's own integers: SciPy filters through doubles, which do not hold int64 labels near 2^63"""
    padded = np.pad(image, 1, mode="symmetric")
    out = None
    for off in itertools.product((0, 1, 2), repeat=image.ndim):
        if footprint[off]:
            q = padded[tuple(slice(o, o + s) for o, s in zip(off, image.shape))]
            out = q.copy() if out is None else op(out, q)
    return out


def grey_dilation(image, footprint):
    return _grey(image, footprint, np.maximum)


def grey_erosion(image, footprint):
    return _grey(image, footprint, np.minimum)


def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
    label_img = _as_labels(label_img)
    if mode == "subpixel":
        return find_boundaries_subpixel(label_img)
    ndim = label_img.ndim
    selem = sndi.generate_binary_structure(ndim, connectivity)
    boundaries = grey_dilation(label_img, selem) != grey_erosion(label_img, selem)
    if mode == "inner":
        boundaries &= label_img != background
    elif mode == "outer":
        max_label = np.iinfo(label_img.dtype).max
        background_image = label_img == background
        full = sndi.generate_binary_structure(ndim, ndim)
        inverted_background = np.array(label_img, copy=True)
        inverted_background[background_image] = max_label
        adjacent_objects = (grey_dilation(label_img, full) != grey_erosion(inverted_background, full)) & ~background_image
        boundaries &= background_image | adjacent_objects
    return boundaries


def find_boundaries_subpixel(label_img):
    label_img = _as_labels(label_img)
    ndim = label_img.ndim
    max_label = np.iinfo(label_img.dtype).max
    expanded = np.zeros([2 * s - 1 for s in label_img.shape], label_img.dtype)
    pixels = (slice(None, None, 2),) * ndim
    expanded[pixels] = label_img
    edges = np.ones(expanded.shape, dtype=bool)
    edges[pixels] = False
    expanded[edges] = max_label
    padded = np.pad(expanded, 1, mode="constant", constant_values=0)
    boundaries = np.zeros_like(edges)
    for index in np.ndindex(expanded.shape):
        if edges[index]:
            window = padded[tuple(slice(i, i + 3) for i in index)]
            if len(np.unique(window)) > 2:
                boundaries[index] = True
    return boundaries


def mark_boundaries_mean(shape, boundaries, color, outline_color=None):
    """channel mean of mark_boundaries over a zero image: the two masked assignments in the reference's order"""
    marked = np.zeros(tuple(shape) + (3,))
    if outline_color is not None:
        marked[sndi.grey_dilation(boundaries.astype(np.uint8), size=(3, 3)).astype(bool)] = outline_color
    marked[boundaries] = color
    return marked.mean(axis=-1)


def map_array(input_arr, input_vals, output_vals, out_dtype=None):
    """the value of the first key equal to the voxel, 0 without one; keys and values cast as the reference casts them"""
    input_arr = np.asarray(input_arr)
    keys = np.asarray(input_vals).astype(input_arr.dtype)
    vals = np.asarray(output_vals)
    if out_dtype is not None:
        vals = vals.astype(out_dtype)
    first = {}
    for j in range(len(keys) - 1, -1, -1):
        first[keys[j].item()] = j
    out = np.zeros(input_arr.shape, vals.dtype)
    flat_in, flat_out = input_arr.reshape(-1), out.reshape(-1)
    for i in range(flat_in.size):
        j = first.get(flat_in[i].item())
        if j is not None:
            flat_out[i] = vals[j]
    return out


def relabel_sequential(label_field, offset=1, input_type=None):
    """(relabeled, in_vals, out_vals)"""
    label_field = np.asarray(label_field)
    if offset <= 0:
        raise ValueError("Offset must be strictly positive.")
    if label_field.min() < 0:
        raise ValueError("Cannot relabel array that contains negative values.")
    in_vals = np.unique(label_field)
    out_val_dtype = np.min_scalar_type(offset + len(in_vals))
    if int(in_vals[0]) == 0:
        out_vals = np.concatenate([np.zeros(1, out_val_dtype), out_val_dtype.type(offset) + np.arange(len(in_vals) - 1, dtype=out_val_dtype)])
    else:
        out_vals = out_val_dtype.type(offset) + np.arange(len(in_vals), dtype=out_val_dtype)
    input_type = label_field.dtype if input_type is None else np.dtype(input_type)
    if input_type.kind not in "iu":
        raise TypeError("label_field must have an integer dtype")
    out_max = int(out_vals[-1])
    required_type = np.min_scalar_type(out_max)
    if input_type.itemsize < required_type.itemsize:
        output_type = required_type
    elif out_max <= np.iinfo(input_type).max:
        output_type = input_type
    else:
        output_type = required_type
    out_vals = out_vals.astype(output_type)
    lookup = dict(zip(in_vals.tolist(), out_vals.tolist()))
    relabeled = np.array([lookup[v] for v in label_field.reshape(-1).tolist()], dtype=output_type).reshape(label_field.shape)
    return relabeled, in_vals, out_vals


def join_segmentations(s1, s2, int64=False):
    """int64=False: the reference's arithmetic, in the relabelled dtype (it wraps); int64=True: the key in int64 and the
    result's dtype from relabel_sequential's rule applied to result_type(s1, s2)"""
    s1, s2 = np.asarray(s1), np.asarray(s2)
    if s1.shape != s2.shape:
        raise ValueError("Cannot join segmentations of different shape.")
    r1 = relabel_sequential(s1)[0]
    r2 = relabel_sequential(s2)[0]
    if int64:
        j = (int(r2.max()) + 1) * r1.astype(np.int64) + r2.astype(np.int64)
        return relabel_sequential(j, input_type=np.result_type(s1.dtype, s2.dtype))[0]
    with np.errstate(over="ignore"):
        j = (r2.max() + 1) * r1 + r2
    return relabel_sequential(j)[0]


def dense_map(in_vals, out_vals):
    in_vals, out_vals = np.asarray(in_vals), np.asarray(out_vals)
    out = np.zeros(int(in_vals.max()) + 1, out_vals.dtype)
    out[in_vals] = out_vals
    return out


# ------------------------------------------------------------------ the closed forms of csrc/segment.hip
def _shifted(padded, offsets, shape):
    return padded[tuple(slice(1 + o, 1 + o + s) for o, s in zip(offsets, shape))]


def closed_form_boundaries(label_img, connectivity=1, mode="thick", background=0):
    """thick(p): a neighbour at city-block distance <= connectivity differs; inner: thick and not background; outer: thick and
    (background or max over the 3^ndim window of L != min over it of g(L)), g(v) = MAX where v == background; the windows
    clamped to the array"""
    L = _as_labels(label_img)
    info = np.iinfo(L.dtype)
    has_bg = info.min <= background <= info.max
    is_bg = (L == background) if has_bg else np.zeros(L.shape, bool)
    G = np.where(is_bg, L.dtype.type(info.max), L)
    pl, pg = np.pad(L, 1, mode="edge"), np.pad(G, 1, mode="edge")
    thick = np.zeros(L.shape, bool)
    mx, mn = L.copy(), G.copy()
    for off in itertools.product((-1, 0, 1), repeat=L.ndim):
        q = _shifted(pl, off, L.shape)
        if 0 < sum(abs(o) for o in off) <= connectivity:
            thick |= q != L
        mx = np.maximum(mx, q)
        mn = np.minimum(mn, _shifted(pg, off, L.shape))
    if mode == "thick":
        return thick
    if mode == "inner":
        return thick & ~is_bg
    return thick & (is_bg | (mx != mn))


def closed_form_subpixel(label_img):
    """an element with an odd coordinate is true when {MAX} + {0 at the first or last coordinate of an axis} + {the labels of
    the pixels its window covers} has more than two distinct values"""
    L = _as_labels(label_img)
    max_label = np.iinfo(L.dtype).max
    shape = tuple(2 * s - 1 for s in L.shape)
    out = np.zeros(shape, bool)
    for c in np.ndindex(shape):
        if not any(v & 1 for v in c):
            continue
        seen = {max_label}
        if any(v == 0 or v == n - 1 for v, n in zip(c, shape)):
            seen.add(0)
        axes = [(v // 2,) if not v & 1 else ((v - 1) // 2, (v + 1) // 2) for v in c]
        for p in itertools.product(*axes):
            seen.add(int(L[p]))
        out[c] = len(seen) > 2
    return out
