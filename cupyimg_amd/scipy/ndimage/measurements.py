"""scipy.ndimage measurements on device arrays: label and the labelled reductions.

Same signatures and results as cupyimg/scipy/ndimage/measurements.py (label :29, sum :316, mean :388, variance :428,
standard_deviation :470, minimum :689, maximum :739, minimum_position :842, maximum_position :895, extrema :950,
center_of_mass :1003, histogram :1066).  All voxel work runs in csrc/label.hip and csrc/measure.hip; this module
massages arguments.  `median` and `labeled_comprehension` are not provided (a per-label median needs a segmented
select; labeled_comprehension takes a Python callable).

Return kinds follow the reference: values are device arrays (0-d for a scalar or absent `index`), positions and centres
of mass are host tuples (a list of tuples for a sequence `index`).
"""
import ctypes

import numpy as np

from ... import core
from . import _support as S

__all__ = [
    "label", "sum", "sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum",
    "minimum_position", "maximum_position", "extrema", "center_of_mass", "histogram", "find_objects",
]

_MAX_VOXELS = 2 ** 31
_MAX_LABEL = 2 ** 31 - 1
# the region tables (csrc/regionprops.hip) have one row per label up to max_label; a table larger than this is refused
# (a label image whose largest label is far above its number of regions wants relabelling, not gigabytes of empty rows)
_TABLE_BYTES_CAP = 2 ** 31


def _generate_binary_structure(rank, connectivity):
    if connectivity < 1:
        connectivity = 1
    if rank < 1:
        return np.array(True, dtype=bool)
    return np.abs(np.indices([3] * rank) - 1).sum(axis=0) <= connectivity


def _label(input, structure, output, greyscale_mode=False, background=0):
    """Label `input` (device, any non-complex dtype) into the int32 device array `output`; returns num_features."""
    input = core.ascontiguousarray(input)
    if input.size >= _MAX_VOXELS:
        raise ValueError("label: arrays of 2**31 voxels or more are not supported (int32 labels); got {} voxels"
                         .format(input.size))
    st = np.ascontiguousarray(structure, dtype=np.uint8)
    num = ctypes.c_int64()
    a, o = input._desc(), output._desc()
    S.check(S.lib().mi_label(ctypes.byref(a), ctypes.byref(o), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                             int(bool(greyscale_mode)), int(background), ctypes.byref(num), None))
    return int(num.value)


def label(input, structure=None, output=None, *, greyscale_mode=False):
    """Label features of an array (scipy.ndimage.label; measurements.py:29-93).

    Returns ``(labels, num_features)``, or ``num_features`` alone when `output` is an array.  Synchronises the device
    once (the feature count)."""
    input = S.as_device(input)            # complex input: TypeError
    if input.dtype == np.float16:
        input = input.astype(np.float32)  # exact; only "non-zero" and equality matter
    if structure is None:
        structure = _generate_binary_structure(input.ndim, 1)
    structure = np.asarray(S.as_host(structure), dtype=bool)
    if structure.ndim != input.ndim:
        raise RuntimeError("structure and input must have equal rank")
    for i in structure.shape:
        if i != 3:
            raise ValueError("structure dimensions must be equal to 3")
    if isinstance(output, core.ndarray):
        if output.shape != input.shape:
            raise ValueError("output shape not correct")
        output._touch()
        caller_provided_output = True
    else:
        caller_provided_output = False
        output = core.empty(input.shape, np.int32 if output is None else np.dtype(output))
    if input.size == 0:
        maxlabel = 0
    elif input.ndim == 0:
        maxlabel = 0 if input.reshape(1).get()[0] == 0 else 1
        output.fill(maxlabel)
    else:
        y = output if output.dtype == np.int32 and output._is_c_contiguous() else core.empty(input.shape, np.int32)
        maxlabel = _label(input, structure, y, greyscale_mode=greyscale_mode)
        if y is not output:
            _check_bit_depth(output.dtype, maxlabel)
            output[...] = y            # the conversion pass (mi_copy)
    if output.dtype != np.int32:
        _check_bit_depth(output.dtype, maxlabel)
    if caller_provided_output:
        return maxlabel
    return output, maxlabel


def _check_bit_depth(dtype, maxlabel):
    dtype = np.dtype(dtype)
    if dtype.kind in "iu" and maxlabel > np.iinfo(dtype).max or dtype.kind == "b" and maxlabel > 1:
        raise RuntimeError("insufficient bit-depth in requested output type")


# ------------------------------------------------------------------ labelled reductions
_OPS = {"sum": 0, "mean": 1, "variance": 2, "std": 3, "extrema": 4, "com": 5, "hist": 6}
_NONZERO = 0x100        # MI_REDUCE_NONZERO: with no index the region is labels != 0
_PRESENCE = 0x200       # MI_REDUCE_PRESENCE: extrema report only whether a voxel carries each value (no position pass)
_LUT_SLACK = 1 << 16


def _prepare(input, labels, index):
    """(input, labels, index_dev, imin, imax, sorted_flag, K, scalar, restore, flags, absent) for mi_labeled_reduce.
    `restore` maps results over the unique sorted index back to the caller's order (None when the lookup-table path
    is used).  `flags`: _NONZERO for uint64 labels with no index.  `absent` (or None): the caller's index entries that
    name no label whatever the labels hold; they are left out of the reduction and filled in by _reduce."""
    input = S.as_device(input)
    if input.dtype == np.float16:
        input = input.astype(np.float32)
    input = core.ascontiguousarray(input)
    if labels is None:
        if index is not None:
            raise ValueError("index given without labels")
        return input, None, None, 0, 0, 0, 1, True, None, 0, None
    labels = S.as_device(labels)
    if labels.dtype.kind not in "biu":
        raise TypeError("labels must be of integer or bool dtype")
    if labels.shape != input.shape:
        labels = _broadcast(labels, input.shape)
    u64 = labels.dtype == np.uint64
    if index is None:
        # SciPy keeps labels > 0: for uint64 labels that is labels != 0, also for those that wrap negative as int64
        return input, _as_int_labels(labels), None, 0, 0, 0, 1, True, None, _NONZERO if u64 else 0, None
    scalar = False
    absent = None
    if isinstance(index, core.ndarray):
        idx_dev = core.ascontiguousarray(index.reshape(-1) if index.ndim != 1 else index, dtype=np.int64)
        if idx_dev.size == 0:
            return input, _as_int_labels(labels), idx_dev, 0, 0, 0, 0, False, None, 0, None
        lo, hi = S.min_max(idx_dev)         # doubles: exact below 2**53 only
        if max(abs(lo), abs(hi)) >= 2.0 ** 53 or (u64 and index.dtype.kind == "i" and lo < 0):
            idx_host, idx_dev = idx_dev.get(), None
            if u64 and index.dtype.kind == "i" and (idx_host < 0).any():
                absent = idx_host < 0
        else:
            imin, imax = int(lo), int(hi)
            idx_host = None
    else:
        arr = np.asarray(index)
        scalar = arr.ndim == 0
        if arr.size == 0:
            return input, _as_int_labels(labels), None, 0, 0, 0, 0, False, None, 0, None
        idx_host, unmatched = _host_index(index, arr, u64)
        if unmatched.any():
            absent = unmatched
        idx_dev = None
    labels = _as_int_labels(labels)
    if absent is not None:
        idx_host = idx_host[~absent]
        if idx_host.size == 0:
            return input, labels, None, 0, 0, 0, 0, scalar, None, 0, absent
    if idx_host is not None:
        imin, imax = int(idx_host.min()), int(idx_host.max())
    K = idx_dev.size if idx_dev is not None else idx_host.size
    if imax - imin < 4 * K + _LUT_SLACK:
        if idx_dev is None:
            idx_dev = core.asarray(idx_host)
        return input, labels, idx_dev, imin, imax, 0, K, scalar, None, 0, absent
    # wide range: binary search over the sorted unique values; results are put back in the caller's order
    if idx_host is None:
        idx_host = idx_dev.get()
    uniq, inv = np.unique(idx_host, return_inverse=True)
    return input, labels, core.asarray(uniq), int(uniq[0]), int(uniq[-1]), 1, uniq.size, scalar, inv, 0, absent


def _as_int_labels(labels):
    """int32 / int64 labels for the device (uint64 values of 2**63 and up wrap negative, equality is kept)"""
    ldt = np.int64 if labels.dtype.itemsize > 4 or labels.dtype == np.uint32 else np.int32
    return core.ascontiguousarray(labels, dtype=ldt)


def _host_index(index, arr, u64):
    """(int64 index values, entries that name no label).  Labels and index meet as int64, uint64 values of 2**63 and
    up wrapped negative: a negative value then names no uint64 label, and a value of 2**63 or more no other label.
    A list that mixes such large Python integers with small ones (NumPy makes it float64) is converted exactly."""
    flat = arr.reshape(-1)
    if arr.dtype.kind in "fO" and all(isinstance(v, (int, np.integer)) for v in np.asarray(index, dtype=object).flat):
        vals = [int(v) for v in np.asarray(index, dtype=object).flat]
        bad = np.array([v < 0 if u64 else v >= 1 << 63 for v in vals]) | \
            np.array([not -(1 << 63) <= v < 1 << 64 for v in vals])
        wrapped = np.array([v % (1 << 64) if -(1 << 63) <= v < 1 << 64 else 0 for v in vals], np.uint64)
        return wrapped.view(np.int64).copy(), bad
    idx = np.ascontiguousarray(flat, dtype=np.int64)
    if arr.dtype.kind == "i" and u64:
        return idx, flat < 0
    if arr.dtype.kind == "u" and not u64:
        return idx, flat >= np.uint64(1 << 63)
    return idx, np.zeros(idx.size, bool)


def _broadcast(labels, shape):
    try:
        bshape = np.broadcast_shapes(labels.shape, shape)
    except ValueError:
        raise ValueError("labels and input must have broadcastable shapes")
    if bshape != tuple(shape):
        raise ValueError("labels and input must have broadcastable shapes")
    nd = len(shape)
    lshape = (1,) * (nd - labels.ndim) + labels.shape
    lstrides = (0,) * (nd - labels.ndim) + labels.strides
    strides = tuple(0 if ls == 1 and s != 1 else st for ls, s, st in zip(lshape, shape, lstrides))
    return labels._view(tuple(shape), strides, labels.ptr)


def _reduce(op, input, labels, index, out_dtype=np.float64, positions=False, hist=None, presence=False):
    inp, lab, idx, imin, imax, srt, K, scalar, restore, flags, absent = _prepare(input, labels, index)
    if op == _OPS["extrema"]:
        out_dtype, width = inp.dtype, 2
    elif op == _OPS["com"]:
        width = inp.ndim
    elif op == _OPS["hist"]:
        out_dtype, width = np.int64, hist[1] + 1
    else:
        width = 1
    out = core.empty((max(K, 1), width), out_dtype)
    pos = core.empty((max(K, 1), 2), np.int64) if positions or presence else None
    if presence and not positions:
        flags |= _PRESENCE
    if K == 0:
        out, pos = out[0:0], (pos[0:0] if pos is not None else None)
    else:
        edges_arr = None
        bins = 0
        if hist is not None:
            edges_arr, bins = hist
        a = inp._desc()
        la = lab._desc() if lab is not None else None
        ia = idx._desc() if idx is not None else None
        oa = out._desc()
        pa = pos._desc() if pos is not None else None
        S.check(S.lib().mi_labeled_reduce(
            op | flags, ctypes.byref(a), ctypes.byref(la) if la is not None else None,
            ctypes.byref(ia) if ia is not None else None, imin, imax, srt,
            edges_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if edges_arr is not None else None,
            bins, ctypes.byref(oa), ctypes.byref(pa) if pa is not None else None, None))
    if absent is not None:
        out, pos = _fill_absent(op, out, pos, restore, absent)
        restore = None
    return out, pos, scalar, restore, inp.shape


def _fill_absent(op, out, pos, restore, absent):
    """results in the caller's index order with the rows of `absent` entries as for a value no voxel carries"""
    fill = np.nan if op in (_OPS["mean"], _OPS["variance"], _OPS["std"], _OPS["com"]) else 0

    def expand(a, value):
        h = a.get() if a.shape[0] else np.zeros(a.shape, a.dtype)
        if restore is not None:
            h = h[restore]
        full = np.empty((absent.size,) + h.shape[1:], h.dtype)
        full[~absent] = h
        full[absent] = value
        return core.asarray(full)
    return expand(out, fill), (expand(pos, -1) if pos is not None else None)


def _values(out, scalar, restore, index):
    """Device result of shape (K, 1) -> 0-d (scalar / no index) or 1-D in the caller's order."""
    flat = out.reshape(out.shape[0])
    if restore is not None:
        flat = core.asarray(flat.get()[restore])
    if index is None or scalar:
        return flat.reshape(()) if flat.size == 1 else flat
    shape = np.shape(index) if not isinstance(index, core.ndarray) else index.shape
    return flat.reshape(shape) if len(shape) != 1 else flat


def _stat(op, input, labels, index):
    out, _, scalar, restore, _ = _reduce(_OPS[op], input, labels, index)
    return _values(out, scalar, restore, index)


def sum_labels(input, labels=None, index=None):
    """Sum of the values per label (scipy.ndimage.sum_labels; measurements.py:316-385), float64."""
    return _stat("sum", input, labels, index)


sum = sum_labels


def mean(input, labels=None, index=None):
    """Mean per label (measurements.py:388-425); NaN for an index value no voxel carries."""
    return _stat("mean", input, labels, index)


def variance(input, labels=None, index=None):
    """Variance per label, two passes (measurements.py:428-467)."""
    return _stat("variance", input, labels, index)


def standard_deviation(input, labels=None, index=None):
    """Standard deviation per label (measurements.py:470-507)."""
    return _stat("std", input, labels, index)


def _extrema(input, labels, index, positions):
    input = S.as_device(input)
    scalar_form = index is None or labels is None or np.ndim(index) == 0 and not isinstance(index, core.ndarray)
    # a scalar form needs to know whether the region is empty: the positions when they are asked for anyway, else the
    # presence flags of the extrema pass (no position pass, whose atomics grow with the ties of the extreme)
    out, pos, scalar, restore, shape = _reduce(_OPS["extrema"], input, labels, index, positions=positions,
                                               presence=scalar_form)
    if scalar and out.shape[0] == 1:
        # no index or a scalar one: SciPy reduces the region's values with vals.min() / vals.max(), which raise on an
        # empty region and give NaN for the minimum when the region holds a NaN (its maximum is then NaN); with a
        # sequence index NaN is skipped unless the region holds nothing else, as the kernel does
        if int(pos.get()[0, 0]) < 0:
            raise ValueError("zero-size array to reduction operation: no voxel carries the index value")
        if input.dtype.kind == "f":
            host = out.get()
            if np.isnan(host[0, 1]) and not np.isnan(host[0, 0]):
                host[0, 0] = np.nan
                out = core.asarray(host)
    if input.dtype == np.float16:
        out = out.astype(np.float16)        # reduced in float32: exact, and SciPy answers in the input dtype
    return out, pos, scalar, restore, shape


def _column(out, col, scalar, restore, index):
    K = out.shape[0]
    v = out[:, col] if K else out.reshape(0)
    return _values(core.ascontiguousarray(v).reshape(K, 1) if K else out.reshape(0, 1), scalar, restore, index)


def _positions(pos, col, scalar, restore, index, shape):
    p = np.maximum(pos.get()[:, col], 0) if pos.shape[0] else np.zeros(0, np.int64)      # absent (-1): (0, ..)
    if restore is not None:
        p = p[restore]
    coords = [tuple(int(c) for c in np.unravel_index(int(v), shape)) for v in p] if len(shape) else [() for _ in p]
    if index is None or scalar:
        return coords[0]
    return coords


def minimum(input, labels=None, index=None):
    """Minimum per label (measurements.py:689-736); 0 for an index value no voxel carries.  With a sequence index NaN
    is skipped unless a region holds nothing else; with no index or a scalar one a NaN in the region is the minimum,
    as in SciPy.  Input dtype."""
    out, _, scalar, restore, _ = _extrema(input, labels, index, False)
    return _column(out, 0, scalar, restore, index)


def maximum(input, labels=None, index=None):
    """Maximum per label (measurements.py:739-786); NaN where a region holds a NaN."""
    out, _, scalar, restore, _ = _extrema(input, labels, index, False)
    return _column(out, 1, scalar, restore, index)


def minimum_position(input, labels=None, index=None):
    """Position of the first minimum per label, as host tuples (measurements.py:842-892)."""
    _, pos, scalar, restore, shape = _extrema(input, labels, index, True)
    return _positions(pos, 0, scalar, restore, index, shape)


def maximum_position(input, labels=None, index=None):
    """Position of the first maximum per label (of the last NaN where the maximum is NaN), host tuples
    (measurements.py:895-947)."""
    _, pos, scalar, restore, shape = _extrema(input, labels, index, True)
    return _positions(pos, 1, scalar, restore, index, shape)


def extrema(input, labels=None, index=None):
    """(minimums, maximums, min_positions, max_positions) per label (measurements.py:950-1000), one pass of each kind.
    With no index or a scalar one, a region no voxel carries raises ValueError, as SciPy's vals.min() does (also for
    minimum, maximum and the position functions)."""
    out, pos, scalar, restore, shape = _extrema(input, labels, index, True)
    return (_column(out, 0, scalar, restore, index), _column(out, 1, scalar, restore, index),
            _positions(pos, 0, scalar, restore, index, shape), _positions(pos, 1, scalar, restore, index, shape))


def center_of_mass(input, labels=None, index=None):
    """Centre of mass per label as host tuples of floats (measurements.py:1003-1063); value and value x coordinate of
    every axis are summed in one pass."""
    out, _, scalar, restore, shape = _reduce(_OPS["com"], input, labels, index)
    res = out.get() if out.shape[0] else np.zeros((0, len(shape)))
    if restore is not None:
        res = res[restore]
    rows = [tuple(float(c) for c in r) for r in res]
    if index is None or scalar:
        return rows[0]
    return rows


def histogram(input, min, max, bins, labels=None, index=None):
    """Histogram per label (measurements.py:1066-1110; scipy: numpy.histogram(values, linspace(min, max, bins + 1))):
    bin k counts edges[k] <= v < edges[k + 1] against those float64 edges, the last bin closed.  Counts are int64
    device arrays; with a sequence `index` a 1-D object ndarray (as SciPy's labeled_comprehension) of one array per
    index value, None for a value no voxel carries.  Raises ValueError, as SciPy does, when the edges decrease and some
    region holds a voxel, for an empty sequence `index`, and for index values that do not survive a round trip through
    the labels' dtype."""
    inp = S.as_device(input)
    bins = int(bins)
    edges = np.ascontiguousarray(np.linspace(min, max, bins + 1), dtype=np.float64)
    labelled = labels is not None and index is not None
    if labelled and (index.size if isinstance(index, core.ndarray) else np.size(index)) == 0:
        raise ValueError("histogram: empty index")          # SciPy: a reduction over no regions
    if labelled:
        # scipy's labeled_comprehension: the index values must survive a round trip through the labels' dtype
        ih = np.atleast_1d(index.get() if isinstance(index, core.ndarray) else index)
        ldt = np.dtype(labels.dtype)
        with np.errstate(all="ignore"):
            lossy = bool(np.any(ih.astype(ldt).astype(ih.dtype) != ih))
        if lossy:
            raise ValueError("Cannot convert index values from <{}> to <{}> (labels' type) without loss of precision"
                             .format(ih.dtype, ldt))
        if ldt == np.uint64 and ih.dtype.kind == "i":
            # SciPy compares labels with index.astype(labels.dtype): here -1 names the label 2**64 - 1
            index = ih.astype(np.uint64) if np.ndim(index) else ih.astype(np.uint64)[0]
    out, _, scalar, restore, _ = _reduce(_OPS["hist"], inp, labels, index, hist=(edges, bins))
    K = out.shape[0]
    # column `bins` counts the region's voxels outside the edges: a row summing to 0 is a region no voxel carries
    present = out.get().sum(axis=1) > 0 if K else np.zeros(0, bool)
    if np.any(edges[:-1] > edges[1:]) and (not labelled or present.any()):
        # numpy.histogram's check, which SciPy reaches only for a region some voxel carries
        raise ValueError("`bins` must increase monotonically, when an array")
    if restore is not None:
        host = out.get()[restore]
        present = present[restore]
        rows = [core.asarray(r[:bins]) for r in host]
    else:
        rows = [out[k, 0:bins] for k in range(K)]
    if labels is not None and index is not None:
        rows = [r if p else None for r, p in zip(rows, present)]      # SciPy's labeled_comprehension default
    if index is None or scalar:
        return rows[0]
    res = np.empty(len(rows), dtype=object)          # as SciPy: an object array of count arrays (None: absent)
    for k, r in enumerate(rows):
        res[k] = r
    return res


# ------------------------------------------------------------------ region tables (csrc/regionprops.hip)
def _dtype_of(a):
    return a.dtype if isinstance(a, core.ndarray) else np.asarray(a).dtype


def _check_table_rows(max_label, row_bytes, what):
    if max_label > _MAX_LABEL:
        raise ValueError("{}: max_label {} is above 2**31 - 1".format(what, max_label))
    if max_label * row_bytes > _TABLE_BYTES_CAP:
        raise ValueError("{}: a table of {} rows of {} bytes is above the cap of {} bytes (one row per label up to the "
                         "largest one: relabel the image sequentially)".format(what, max_label, row_bytes, _TABLE_BYTES_CAP))


def _max_label(labels, what):
    """(smallest, largest) label of a non-empty device array as Python ints: the existing min / max reduction, one small
    read-back.  uint64 labels of 2**63 and up have no int64 the kernels could compare: ValueError."""
    lo, hi = S.min_max(labels)
    if labels.dtype == np.uint64 and hi >= 2.0 ** 63:
        raise ValueError("{}: uint64 labels of 2**63 or more are not supported".format(what))
    return int(lo), int(hi)


def _region_extents(labels, max_label):
    """int64 device table (max_label, 1 + 3 ndim) of the C-contiguous int32 / int64 device `labels` (ndim >= 1): voxel count |
    smallest index per axis | largest index + 1 per axis | sum of the indices per axis.  Nothing synchronises."""
    ext = core.empty((max_label, 1 + 3 * labels.ndim), np.int64)
    la, ea = labels._desc(), ext._desc()
    S.check(S.lib().mi_rp_extent(ctypes.byref(la), ctypes.byref(ea), None), ValueError)
    return ext


def find_objects(input, max_label=0):
    """Bounding boxes of the labelled regions (scipy.ndimage.find_objects): a list of `max_label` tuples of slices, None
    for a label no voxel carries.  One sweep of rp_extent_kernel over the labels and one read-back of its table.

    max_label < 1 means the array's maximum (one more small read-back).  Any integer or bool dtype; floats raise TypeError
    and an empty input ValueError, as SciPy.  Deviations, both ValueError: uint64 labels of 2**63 or more, and a max_label
    above 2**31 - 1 or one whose table (max_label x (1 + 3 ndim) x 8 bytes) is above 2 GiB."""
    dt = _dtype_of(input)
    if dt.kind not in "biu":
        raise TypeError("find_objects: labels must be of integer or bool dtype, got {}".format(dt))
    if (input.size if isinstance(input, core.ndarray) else np.size(input)) == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    max_label = int(max_label)
    ndim = input.ndim if isinstance(input, core.ndarray) else np.ndim(input)
    if max_label >= 1:
        _check_table_rows(max_label, 8 * (1 + 3 * max(ndim, 1)), "find_objects")
    input = S.as_device(input)
    if max_label < 1:
        max_label = _max_label(input, "find_objects")[1]
        if max_label < 1:
            return []
        _check_table_rows(max_label, 8 * (1 + 3 * max(ndim, 1)), "find_objects")
    elif input.dtype == np.uint64:
        _max_label(input, "find_objects")
    labels = _as_int_labels(input)
    if ndim == 0:
        v = int(labels.reshape(1).get()[0])
        return [() if k + 1 == v else None for k in range(max_label)]
    ext = _region_extents(labels, max_label).get()
    return _slices_of(ext, ndim)


def _slices_of(ext, ndim):
    """SciPy's list of slice tuples from the host copy of an extent table"""
    out = []
    for row in ext:
        if row[0] == 0:
            out.append(None)
        else:
            out.append(tuple(slice(int(row[1 + d]), int(row[1 + ndim + d]), None) for d in range(ndim)))
    return out
