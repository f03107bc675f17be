"""map_array and ArrayMap (cupyimg/skimage/util/_map_array.py).

The reference searches all `nvals` keys linearly for every voxel.  Here a voxel either gathers through a dense table of key
positions over [smallest key, largest key] (built by one fill and one atomicMin launch; kept in LDS while it is small), or
does a leftmost binary search in the keys sorted once by the stable device argsort.  Both give what the reference's loop
gives, duplicate keys (the first wins) and missing keys (0) included."""
import ctypes

import numpy as np

from ... import core
from ...scipy.ndimage import _support as S

__all__ = ["map_array", "ArrayMap"]

# Route rules, from profiles/segment.txt (the "map_array 4096x4096 int32" lines: 16.8 M voxels, both routes alternated).
# The table costs 4 bytes per value of the key range whatever the number of keys, the search log2(nvals) dependent reads per
# voxel.  The table was the faster route at every point measured, up to the widest range measured, 2^24 values (whole calls,
# table against search, the sort of the keys included): 100 keys spread over 2^24 values 105 us against 221 us, 10^4 keys 168
# against 490, 10^6 keys 535 against 1474; dense keys 96 / 220, 127 / 487, 381 / 1475.  Wider ranges are unmeasured and take
# the search.
TABLE_MAX_RANGE = 1 << 24
# A workgroup copies the table to LDS first while it fits the 64 KiB a launch gets without an attribute (16384 values: the
# kernel's limit); that was faster than gathering from global memory at both ranges measured that fit (the three launches
# alone): 100 values 43 us against 51 us, 10^4 values 76 against 85.
LDS_MAX_RANGE = 1 << 14
_EXACT_DOUBLE = 2 ** 53             # S.min_max reports the extrema as doubles

ROUTES = ("auto", "table_lds", "table", "search")
_route = "auto"


def set_route(route):
    """Force a route for every later map_array call of this process ("table_lds", "table", "search"), or give the choice
    back to the rules above ("auto").  For tests and timing: a forced table route raises when the key range does not fit."""
    global _route
    if route not in ROUTES:
        raise ValueError("route must be one of {}".format(ROUTES))
    _route = route


def _ordered(value, dtype):
    """an integer of `dtype` as the order-preserving unsigned 64-bit key of csrc/segment.hip"""
    return int(value) + 2 ** 63 if dtype.kind == "i" else int(value)


def _key_range(keys):
    """(smallest, largest) key as Python ints, or None when a double does not hold them exactly"""
    lo, hi = S.min_max(keys)
    if abs(lo) >= _EXACT_DOUBLE or abs(hi) >= _EXACT_DOUBLE:
        return None
    return int(lo), int(hi)


def map_array(input_arr, input_vals, output_vals, out=None):
    """out[i] = output_vals[j] for the first j with input_vals[j] == input_arr[i], 0 where there is none.  `input_arr` is an
    integer device array (or anything `asarray` takes); `out`, when given, is a C-contiguous device array of its shape."""
    if not isinstance(input_arr, core.ndarray):
        input_arr = core.asarray(input_arr) if hasattr(input_arr, "__cuda_array_interface__") else np.asarray(input_arr)
    if input_arr.dtype.kind not in "iu":
        raise TypeError("The dtype of an array to be remapped should be integer.")
    input_arr = core.asarray(input_arr)
    input_vals = core.asarray(input_vals)
    output_vals = core.asarray(output_vals)
    orig_shape = input_arr.shape
    if out is None:
        out = core.ndarray(orig_shape, output_vals.dtype)
    elif not isinstance(out, core.ndarray):
        raise TypeError("out must be a device array")
    elif out.shape != orig_shape:
        raise ValueError("If out array is provided, it should have the same shape as the input array. Input array has "
                         "shape {}, provided output array has shape {}.".format(orig_shape, out.shape))
    elif not out._is_c_contiguous():
        raise ValueError("If out array is provided, it should be either contiguous or 1-dimensional. Got array with shape "
                         "{} and strides {}.".format(out.shape, out.strides))
    if input_vals.ndim != 1 or output_vals.ndim != 1 or input_vals.size != output_vals.size:
        raise ValueError("input_vals and output_vals are 1-D arrays of one length")
    if out.dtype == np.float16:
        raise TypeError("float16 arrays are storage only: convert with astype(float32) around this call")
    if not input_arr.size:
        return out
    out._touch()
    nvals = input_vals.size
    lib = S.lib()
    if nvals == 0:
        S.check(lib.mi_memset(out.ptr, 0, out.nbytes, None))
        return out
    flat_in = core.ascontiguousarray(input_arr).reshape(-1)
    flat_out = out.reshape(-1)
    keys = core.ascontiguousarray(input_vals.astype(input_arr.dtype, copy=False))
    vals = core.ascontiguousarray(output_vals.astype(out.dtype, copy=False))
    route = _route
    span = None
    if route != "search":
        rng = _key_range(keys)
        if rng is not None:
            span = rng[1] - rng[0] + 1
        if route == "auto":
            if span is None or span > TABLE_MAX_RANGE:
                route = "search"
            else:
                route = "table_lds" if span <= LDS_MAX_RANGE else "table"
        elif span is None or span > 2 ** 31 or (route == "table_lds" and span > 16384):
            raise ValueError("map_array: the key range does not fit the forced route {!r}".format(route))
    ind, kd, vd, od = flat_in._desc(), keys._desc(), vals._desc(), flat_out._desc()
    if route == "search":
        perm, srt = core._argsort(keys, False, True, True)
        sd, pd = srt._desc(), perm._desc()
        S.check(lib.mi_map_array_search(ctypes.byref(ind), ctypes.byref(sd), ctypes.byref(pd), ctypes.byref(vd), ctypes.byref(od), None))
    else:
        S.check(lib.mi_map_array_table(ctypes.byref(ind), ctypes.byref(kd), ctypes.byref(vd), ctypes.byref(od),
                                       _ordered(rng[0], keys.dtype), span, int(route == "table_lds"), None))
    return out


class ArrayMap:
    """Mapping by indexing without the dense array: `m[index]` is `map_array(index, in_values, out_values)`.  in_values and
    out_values are device arrays (or anything `asarray` takes)."""

    def __init__(self, in_values, out_values):
        self.in_values = core.asarray(in_values)
        self.out_values = core.asarray(out_values)
        self._max_str_lines = 4
        self._max_label = int(S.min_max(self.in_values)[1]) if self.in_values.size else -1

    def __len__(self):
        """One more than the largest value being remapped."""
        return self._max_label + 1

    def _dense(self, dtype=None):
        """the device array that behaves like the map when indexed: map_array over 0 .. max"""
        index = core.asarray(np.arange(len(self), dtype=np.int64))
        out = self[index] if len(self) else core.ndarray((0,), self.out_values.dtype)
        return out if dtype is None else out.astype(dtype, copy=False)

    def __array__(self, dtype=None, copy=None):
        return self._dense(dtype).get()

    @property
    def dtype(self):
        return self.out_values.dtype

    def __repr__(self):
        return "ArrayMap({!r}, {!r})".format(self.in_values.get(), self.out_values.get())

    def __str__(self):
        ins, outs = self.in_values.get(), self.out_values.get()
        if len(ins) <= self._max_str_lines + 1:
            rows = ["  {} → {}".format(ins[i], outs[i]) for i in range(len(ins))]
        else:
            half = self._max_str_lines // 2
            rows = (["  {} → {}".format(ins[i], outs[i]) for i in range(half)] + ["  ..."]
                    + ["  {} → {}".format(ins[i], outs[i]) for i in range(-half, 0)])
        return "\n".join(["ArrayMap:"] + rows)

    def __call__(self, arr):
        return self.__getitem__(arr)

    def __getitem__(self, index):
        scalar = np.isscalar(index)
        if scalar:
            index = core.asarray(np.asarray([index]))
        elif isinstance(index, slice):
            start = index.start or 0
            stop = index.stop if index.stop is not None else len(self)
            index = core.asarray(np.arange(start, stop, index.step, dtype=np.int64))
        else:
            index = core.asarray(index)
        if index.dtype == np.bool_:
            index = core.flatnonzero(index)
        if index.dtype.kind not in "iu":
            raise TypeError("The dtype of an array to be remapped should be integer.")
        out = map_array(index, self.in_values.astype(index.dtype, copy=False), self.out_values)
        if scalar:
            return out.get()[0]
        return out

    def __setitem__(self, indices, values):
        raise NotImplementedError("ArrayMap is read-only here: the device array layer has no index assignment")
