"""scipy.ndimage filters on device arrays.

Same signatures, defaults and error behaviour as
cupyimg/scipy/ndimage/filters.py (correlate :65, convolve :137, correlate1d
:213, convolve1d :286, uniform_filter1d :549, uniform_filter :602,
gaussian_filter1d :668, gaussian_filter :725, minimum/maximum_filter(1d)
:1291-1475), re-written around the C-ABI of libmi355img:

  * the three separable passes of uniform_filter / gaussian_filter on
    3-D float32 volumes run as ONE fused HIP launch (mi_separable3d_f32);
    everything else runs one generic HIP kernel per pass, ping-ponging
    between the output and one scratch volume (no zero-fills, no copy-backs);
  * small parameter arrays (weights, footprints) stay on the host.

Where the reference deviates from SciPy the implementation follows SciPy
(SURVEY.md section 8c): float64 weights, sum-then-divide box means (exact for
integer images), min/max `cval` converted to the input dtype.
"""
import collections
import ctypes
import warnings

import numpy as np

from ... import core
from . import _support as S

__all__ = [
    "correlate1d", "convolve1d", "gaussian_filter1d", "gaussian_filter", "correlate", "convolve",
    "uniform_filter1d", "uniform_filter", "minimum_filter1d", "maximum_filter1d", "minimum_filter",
    "maximum_filter", "prewitt", "sobel", "generic_laplace", "laplace", "gaussian_laplace",
    "generic_gradient_magnitude", "gaussian_gradient_magnitude", "rank_filter", "median_filter",
    "percentile_filter",
]


# ----------------------------------------------------------------------------
# correlate / convolve
# ----------------------------------------------------------------------------
def _check_real(a):
    if a.dtype.kind == "c":
        raise TypeError("Complex type not supported")


def _launch_correlate1d(src, dst, axis, weights, origin, mode, cval, acc):
    w, wp = S.c_doubles(weights)
    a, b = src._desc(), dst._desc()
    S.check(S.lib().mi_correlate1d(ctypes.byref(a), ctypes.byref(b), axis, wp, int(w.size), int(origin),
                                   S.mode_code(mode), float(cval), acc, None))


def correlate1d(input, weights, axis=-1, output=None, mode="reflect", cval=0, origin=0, *,
                backend="ndimage", dtype_mode="float"):
    """One-dimensional correlate along ``axis`` (filters.py:213-283)."""
    if backend != "ndimage":
        raise ValueError("only backend='ndimage' is available")
    input = S.as_device(input)
    weights = S.as_host(weights)
    _check_real(weights)
    if weights.ndim != 1 or weights.size < 1:
        raise RuntimeError("incorrect filter size")
    S.check_mode(mode)
    axis = S.normalize_axis(axis, input.ndim)
    origin = S.check_origin(origin, weights.size)
    S.check_cval(mode, cval, S.is_integer_output(output, input))
    acc = S.acc_flag(dtype_mode)
    output = S.get_output(output, input)
    if input.ndim == 0 or input.size == 0:
        return output
    return S.run_kernel(input, output,
                        lambda s, d: _launch_correlate1d(s, d, axis, weights, origin, mode, cval, acc))


def convolve1d(input, weights, axis=-1, output=None, mode="reflect", cval=0, origin=0, *,
               crop=True, backend="ndimage", dtype_mode="float"):
    """One-dimensional convolution (filters.py:286-438): correlate with the
    reversed kernel and the origin mirrored (-1 more for even lengths)."""
    if not crop:
        raise ValueError("crop=False requires backend='fast_upfirdn', which is not available")
    weights = S.as_host(weights)
    if weights.ndim != 1 or weights.size < 1:
        raise RuntimeError("incorrect filter size")
    origin = S.check_origin(origin, weights.size)
    weights = weights[::-1]
    origin = -origin
    if not len(weights) & 1:
        origin -= 1
    return correlate1d(input, weights, axis, output, mode, cval, origin, backend=backend,
                       dtype_mode=dtype_mode)


def _correlate_or_convolve(input, weights, output, mode, cval, origin, convolution, dtype_mode):
    """filters.py:441-495"""
    input = S.as_device(input)
    weights = S.as_host(weights)
    _check_real(weights)
    S.check_mode(mode)
    wdims = [x for x in weights.shape if x != 0]
    if len(wdims) != input.ndim:
        raise RuntimeError("filter weights array has incorrect shape")
    origins = S.fix_sequence_arg(origin, len(wdims), "origin", int)
    for o, wd in zip(origins, wdims):
        S.check_origin(o, wd)
    if weights.size == 0:
        return core.zeros_like(input)
    S.check_cval(mode, cval, S.is_integer_output(output, input))
    if convolution:
        weights = weights[tuple([slice(None, None, -1)] * weights.ndim)]
        origins = [-o - (1 if ws % 2 == 0 else 0) for o, ws in zip(origins, weights.shape)]
        for o, wd in zip(origins, weights.shape):
            S.check_origin(o, wd)
    if dtype_mode == "numpy":
        # scipy.signal's callers: the result has NumPy's promoted dtype, not a float (filters.py:470-487)
        if output is not None:
            raise ValueError("dtype_mode == 'numpy' does not support the output argument")
        dtype = np.promote_types(input.dtype, weights.dtype)
        if input.dtype != dtype:
            input = input.astype(dtype)
        output = dtype
        acc = 0
    else:
        acc = S.acc_flag(dtype_mode)
    output = S.get_output(output, input)
    if input.size == 0:
        return output
    w, wp = S.c_doubles(weights)
    wshape = S.c_int64s(weights.shape)
    org = S.c_ints(origins)

    def launch(src, dst):
        a, b = src._desc(), dst._desc()
        S.check(S.lib().mi_correlate_nd(ctypes.byref(a), ctypes.byref(b), wp, wshape, org,
                                        S.mode_code(mode), float(cval), acc, None))

    if (input.ndim == 3 and output.dtype == input.dtype and input.dtype in (np.float32, np.uint8, np.int8, np.uint16, np.int16)
            and input.shape[2] % 4 and max(weights.shape) <= 9 and S.current_planes() is None):       # (the stencil kernel takes rows of 4 k elements)
        # rows that are not a multiple of 16 bytes: the LDS-tiled stencil kernel on explicitly extended rows (r4b;
        # 181 x 217 x 181 float32, 3 x 3 x 3 weights: 219 -> see DESIGN.md)
        if (input.dtype == np.float32 and weights.shape in ((3, 3, 3), (5, 5, 5), (7, 7, 7)) and input._is_c_contiguous()
                and output._is_c_contiguous() and not core.shares_memory(output, input)):
            # r6: the scatter kernel takes rows of any length -- asked first; a refusal queues nothing
            a, b = input._desc(), output._desc()
            try:
                S.check(S.lib().mi_correlate3_dense(ctypes.byref(a), ctypes.byref(b), wp, wshape, org, S.mode_code(mode), float(cval), acc, None))
                return output
            except S.Unsupported:
                pass
        left = weights.shape[2] // 2 + int(origins[2])
        res = _run_on_extended_rows(input, output, left, weights.shape[2] - 1 - left, mode, cval,
                                    lambda e, o: (launch(e, o), o)[1])        # (the launch raises or succeeds: nothing to remember)
        if res is not None:
            return res
    return S.run_kernel(input, output, launch)


def correlate(input, weights, output=None, mode="reflect", cval=0.0, origin=0, *,
              use_weights_mask=False, dtype_mode="ndimage"):
    """Multi-dimensional correlate (filters.py:65-134)."""
    return _correlate_or_convolve(input, weights, output, mode, cval, origin, False, dtype_mode)


def convolve(input, weights, output=None, mode="reflect", cval=0.0, origin=0, *,
             use_weights_mask=False, dtype_mode="ndimage"):
    """Multi-dimensional convolution (filters.py:137-210)."""
    return _correlate_or_convolve(input, weights, output, mode, cval, origin, True, dtype_mode)


# ----------------------------------------------------------------------------
# fused separable path
# ----------------------------------------------------------------------------
def _try_fused_3d(input, output, weights, origins, modes, cval, is_box):
    """All 1-D passes of a 3-D float32 filter in one launch.  Returns the
    output, or None when the fused kernel does not cover the request (the
    caller then runs generic *device* passes).  Inside `S.output_planes(..)`
    only the given output planes are computed, and a request the fused kernel
    cannot take raises instead of falling back."""
    planes = S.current_planes()
    if input.ndim == 2 and output.ndim == 2 and planes is None:
        # an image is a one-plane volume: same kernels, no z taps
        as3 = lambda a: a._as3()   # noqa: E731
        res = _fused_3d(as3(input), as3(output), [None] + list(weights), [0] + list(origins),
                        ["reflect"] + list(modes), cval, is_box, None)
        return None if res is None else output
    res = _fused_3d(input, output, weights, origins, modes, cval, is_box, planes)
    if res is None and planes is not None:
        raise S.Unsupported("plane-restricted filtering needs the fused 3-D float32 kernel "
                            "(contiguous, non-aliasing float32 volumes, odd kernels of at most 9 taps)")
    return res


_NULL_DP = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
_WEIGHT_CACHE = {}
_INTS_CACHE = {}


def _marshal_weights(weights):
    """(arrays kept alive, double *[3], lengths) for three optional host weight vectors; memoised on the values --
    the same few kernels are requested over and over, and marshalling them was a quarter of a small call."""
    key = tuple(None if w is None else np.asarray(w, dtype=np.float64).tobytes() for w in weights)
    hit = _WEIGHT_CACHE.get(key)
    if hit is None:
        keep = [None if w is None else np.ascontiguousarray(w, dtype=np.float64).copy() for w in weights]
        ptrs = (ctypes.POINTER(ctypes.c_double) * 3)(*[
            _NULL_DP if w is None else w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for w in keep])
        hit = (keep, ptrs, S.c_ints([0 if w is None else len(w) for w in keep]))
        if len(_WEIGHT_CACHE) > 256:
            _WEIGHT_CACHE.clear()
        _WEIGHT_CACHE[key] = hit
    return hit


def _cached_ints(values):
    hit = _INTS_CACHE.get(values)
    if hit is None:
        if len(_INTS_CACHE) > 1024:
            _INTS_CACHE.clear()
        hit = _INTS_CACHE[values] = S.c_ints(values)
    return hit


def _fused_3d(input, output, weights, origins, modes, cval, is_box, planes):
    if input.ndim == 3 and input.dtype == np.float64 and output.dtype == np.float64 and planes is None:
        return _fused_3d_f64(input, output, weights, origins, modes, cval)
    if input.ndim != 3 or input.dtype != np.float32 or output.dtype != np.float32:
        return None
    if not any(w is not None for w in weights):
        return None
    for w, o in zip(weights, origins):
        if w is not None and (len(w) > 33 or len(w) % 2 == 0):
            return None
    if weights[2] is not None and origins[2] != 0:
        return None
    if input.size == 0:
        return None
    ragged = input.shape[2] % 4 != 0
    if input.shape[2] < 8 or (ragged and input.shape[2] < 16 and planes is not None):
        return None
    if planes is not None and not (input._is_c_contiguous() and output._is_c_contiguous()
                                   and not core.shares_memory(output, input)):
        return None
    src = core.ascontiguousarray(input)
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    if src.ptr % 16 or dst.ptr % 16:
        if ragged and planes is None and input.size >= (1 << 15):
            return _fused_3d_padded_rows(input, output, weights, origins, modes, cval, is_box)
        return None
    keep, ptrs, wlen = _marshal_weights(weights)
    org = _cached_ints(tuple(origins))
    mds = _cached_ints(tuple(S.mode_code(m) for m in modes))
    a, b = src._desc(), dst._desc()
    try:
        if planes is None:
            S.check(S.lib().mi_separable3d_f32(ctypes.byref(a), ctypes.byref(b), ptrs, wlen, org, mds,
                                               float(cval), int(is_box), None))
        else:
            flat = S.c_int64s([v for r in planes for v in r])
            S.check(S.lib().mi_separable3d_f32_planes(ctypes.byref(a), ctypes.byref(b), ptrs, wlen, org, mds,
                                                      float(cval), flat, len(planes), None))
    except S.Unsupported:
        # r5: rows that are not a multiple of 16 bytes go to the library first (the 3 / 5 / 7-tap kernel takes them as they
        # are); what it refuses runs on explicitly extended rows
        if ragged and planes is None and input.size >= (1 << 15):
            return _fused_3d_padded_rows(input, output, weights, origins, modes, cval, is_box)
        return None
    if not direct:
        output[...] = dst
    return output


# requests the fused path behind _run_on_extended_rows refused: (tag, dtypes, shape, parameters, knob generation), oldest first
_EXT_REFUSED = collections.OrderedDict()
_EXT_REFUSED_MAX = 1024


def _refusal_key(key, input, output, left, right, mode_x):
    """What a refusal of the fused path depends on.  r5 advisor findings: the library's debug knobs are part of it (their
    generation counter, mi_debug_generation: a refusal recorded while a test had a kernel switched off must not outlive the
    switch), and a NaN anywhere in the parameters must compare equal to itself."""
    def norm(v):
        if isinstance(v, float) and v != v:
            return "nan"
        if isinstance(v, (tuple, list)):
            return tuple(norm(x) for x in v)
        return v
    return (norm(key), input.dtype.char, output.dtype.char, tuple(input.shape), left, right, mode_x,
            int(S.lib().mi_debug_generation()))


def _reset_ext_refused():
    _EXT_REFUSED.clear()


def _run_on_extended_rows(input, output, left, right, mode_x, cval, run, exact_cval=True, key=None):
    """Rows whose length is not a multiple of 16 bytes (181 x 217 x 181, 91 x 109 x 91, ...: most volumes that were not
    acquired as powers of two) cannot take the fused kernels directly -- their 16-byte row accesses need aligned rows.
    r4b: extend every row explicitly along the last axis (what its boundary mode prescribes, at least the filter's reach
    (`left`, `right`) on either side, to a multiple of 16 bytes: mi_extend_rows), call `run(ext_in, ext_out)` -- the fused
    path on the extended array, whose x boundary handling no kept output depends on any more; returns None when it does
    not take the request -- and copy the columns back (mi_crop_rows).  Three efficient launches at ~3 x the fused
    kernel's traffic instead of generic per-axis passes (181 x 217 x 181 float32, uniform_filter(5): 125 -> 48 us).
    `key`: what the fused path's answer depends on besides the data (r4 advisor finding: a request it refuses -- large
    windows, ranks it does not handle -- paid two allocations and a full-volume copy before falling back to the generic
    passes, on every call): a refusal is remembered and the next call with the same key returns at once."""
    raw_key = key
    if key is not None and _EXT_REFUSED:                  # (nothing recorded: nothing to look up -- the key is made when a refusal is stored)
        key = _refusal_key(key, input, output, left, right, mode_x)
        if key in _EXT_REFUSED:
            _EXT_REFUSED.move_to_end(key)
            return None
    if left < 0 or right < 0 or input.size < (1 << 15) or input.dtype.itemsize not in (1, 2, 4, 8) or output.dtype.itemsize not in (1, 2, 4, 8):
        return None
    if exact_cval and mode_x in ("constant", "grid-constant"):
        # the fill value is written into the extended rows in the ARRAY's dtype; the bit-exact kernels (like SciPy) use cval
        # as a double: only values the dtype holds exactly may take this route (the float32 separable kernels round it
        # to float32 themselves: exact_cval = False)
        cv = float(cval)
        if input.dtype.kind in "iub":
            info = np.iinfo(input.dtype) if input.dtype.kind in "iu" else None
            if not (np.isfinite(cv) and cv == int(cv) and (info is None and cv in (0.0, 1.0) or info is not None and info.min <= cv <= info.max)):
                return None
        elif input.dtype == np.float32:
            if not (np.isnan(cv) or float(np.float32(cv)) == cv):
                return None
        elif input.dtype != np.float64:
            return None
    v = 16 // min(input.dtype.itemsize, output.dtype.itemsize)      # rows of both arrays become multiples of 16 bytes
    nx = input.shape[-1]
    pl = -(-left // v) * v
    total = -(-(pl + -(-nx // v) * v + right) // v) * v          # the kept columns, rounded up to 16 bytes, lie inside a row
    shape = tuple(input.shape[:-1]) + (total,)
    if int(np.prod(shape)) * input.dtype.itemsize >= (1 << 31):
        return None
    src = core.ascontiguousarray(input)
    ext = core.empty(shape, input.dtype)
    tmp = core.empty(shape, output.dtype)
    a, b = src._desc(), ext._desc()
    S.check(S.lib().mi_extend_rows(ctypes.byref(a), ctypes.byref(b), pl, S.mode_code(mode_x), float(cval), None))
    if run(ext, tmp) is None:
        if raw_key is not None:
            key = _refusal_key(raw_key, input, output, left, right, mode_x)
            _EXT_REFUSED[key] = True
            while len(_EXT_REFUSED) > _EXT_REFUSED_MAX:
                _EXT_REFUSED.popitem(last=False)          # least recently used first
        return None
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    a, b = tmp._desc(), dst._desc()
    S.check(S.lib().mi_crop_rows(ctypes.byref(a), ctypes.byref(b), pl, None))
    if not direct:
        output[...] = dst
    return output


def _fused_3d_padded_rows(input, output, weights, origins, modes, cval, is_box):
    wx = weights[2]
    if wx is None:
        left = right = 0
    else:
        left = len(wx) // 2 + int(origins[2])
        right = len(wx) - 1 - left
    # the x mode no longer matters for the columns that are kept; `nearest` is the cheapest for the kernels
    return _run_on_extended_rows(input, output, left, right, modes[2], cval,
                                 lambda e, o: _fused_3d(e, o, weights, origins, [modes[0], modes[1], "nearest"], cval, is_box, None),
                                 exact_cval=False,
                                 key=("sep3d", tuple(None if w is None else len(w) for w in weights), tuple(int(o) for o in origins), tuple(modes[:2]), bool(is_box)))


def _fused_3d_f64(input, output, weights, origins, modes, cval):
    """float64 volumes / images: streaming passes with the x pass fused (mi_separable3d_f64)."""
    if not any(w is not None for w in weights) or input.size == 0:
        return None
    for w in weights:
        if w is not None and (len(w) > 33 or len(w) % 2 == 0):
            return None
    if (weights[2] is not None and origins[2] != 0) or input.shape[2] < 4:
        return None
    if input.shape[2] % 2:
        # r5: rows of an odd number of doubles (181 x 217 x 181 as nibabel's get_fdata() hands it out): extended to whole 16-byte
        # vectors, filtered by the streaming kernels, cropped -- instead of the generic passes
        wx = weights[2]
        left = 0 if wx is None else len(wx) // 2 + int(origins[2])
        right = 0 if wx is None else len(wx) - 1 - left
        return _run_on_extended_rows(input, output, left, right, modes[2], cval,
                                     lambda e, o: _fused_3d_f64(e, o, weights, origins, [modes[0], modes[1], "nearest"], cval),
                                     key=("sep3d64", tuple(None if w is None else len(w) for w in weights), tuple(int(o) for o in origins), tuple(modes[:2])))
    src = core.ascontiguousarray(input)
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    if src.ptr % 16 or dst.ptr % 16:
        return None
    keep, ptrs, wlen = _marshal_weights(weights)
    a, b = src._desc(), dst._desc()
    try:
        S.check(S.lib().mi_separable3d_f64(ctypes.byref(a), ctypes.byref(b), ptrs, wlen, _cached_ints(tuple(origins)),
                                           _cached_ints(tuple(S.mode_code(m) for m in modes)), float(cval), None))
    except S.Unsupported:
        return None
    if not direct:
        output[...] = dst
    return output


# ----------------------------------------------------------------------------
# uniform
# ----------------------------------------------------------------------------
def _launch_uniform1d(src, dst, axis, size, origin, mode, cval):
    a, b = src._desc(), dst._desc()
    S.check(S.lib().mi_uniform_filter1d(ctypes.byref(a), ctypes.byref(b), axis, int(size), int(origin),
                                        S.mode_code(mode), float(cval), None))


def uniform_filter1d(input, size, axis=-1, output=None, mode="reflect", cval=0.0, origin=0, *,
                     dtype_mode="ndimage"):
    """One-dimensional uniform filter (filters.py:549-599)."""
    input = S.as_device(input)
    if size < 1:
        raise RuntimeError("incorrect filter size")
    S.check_mode(mode)
    output = S.get_output(output, input)
    size = int(size)
    origin = S.check_origin(origin, size)
    axis = S.normalize_axis(axis, input.ndim)
    S.check_cval(mode, cval, output.dtype.kind in "iu")
    if input.ndim == 0 or input.size == 0:
        return output
    if dtype_mode == "float":
        w = np.full((size,), 1.0 / size)
        return S.run_kernel(input, output,
                            lambda s, d: _launch_correlate1d(s, d, axis, w, origin, mode, cval, 1))
    S.acc_flag(dtype_mode)
    return S.run_kernel(input, output,
                        lambda s, d: _launch_uniform1d(s, d, axis, size, origin, mode, cval))


def _try_uniform_integer(input, output, sizes, origins, modes, cval):
    """uint8 / uint16 / int16 image or volume, same dtype out: the box passes in integer arithmetic -- y and x in one
    launch (mi_uniform2d_*), a z window of a volume as one more launch before it (mi_uniform_z_*; SciPy filters axis 0
    first and keeps the intermediate in the integer dtype).  None when the request is not covered."""
    if S.current_planes() is not None or input.size == 0:
        return None
    nd = input.ndim
    sz = [int(v) for v in sizes]
    og = [int(v) for v in origins]
    md_all = list(modes)
    if any(v < 1 or v > 9 or v % 2 == 0 for v in sz) or og[-1] != 0 or all(v == 1 for v in sz):
        return None
    if any(s_ == 1 and o_ != 0 for s_, o_ in zip(sz, og)):
        return None
    md = md_all[-2:]
    info = np.iinfo(input.dtype)
    if any(m in ("constant", "grid-constant") for m in md_all):
        if not (np.isfinite(cval) and info.min <= cval <= info.max and float(cval) == int(cval)):
            return None
    cv = int(cval) if np.isfinite(cval) and info.min <= cval <= info.max else 0
    is8 = input.dtype == np.uint8
    lib = S.lib()
    src = core.ascontiguousarray(input)
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    plane_pass = not (sz[-2] == 1 and sz[-1] == 1)
    try:
        if nd == 3 and sz[0] > 1:
            mid = core.empty(src.shape, src.dtype) if plane_pass else dst
            a, b = src._desc(), mid._desc()
            S.check((lib.mi_uniform_z_u8 if is8 else lib.mi_uniform_z_16)(ctypes.byref(a), ctypes.byref(b), sz[0], og[0],
                                                                          S.mode_code(md_all[0]), cv, None))
            src = mid
        if plane_pass:
            a, b = src._desc(), dst._desc()
            S.check((lib.mi_uniform2d_u8 if is8 else lib.mi_uniform2d_16)(ctypes.byref(a), ctypes.byref(b), _cached_ints(tuple(sz[-2:])),
                                                                          og[-2], _cached_ints(tuple(S.mode_code(m) for m in md)), cv, None))
    except S.Unsupported:
        return None
    if not direct:
        output[...] = dst
    return output


def uniform_filter(input, size=3, output=None, mode="reflect", cval=0.0, origin=0, *,
                   dtype_mode="ndimage"):
    """Multi-dimensional uniform filter (filters.py:602-665).

    Precision: on 2-D / 3-D float32 inputs the fused kernel, where it takes the call, accumulates in float32 whatever
    `dtype_mode` says (calls it declines run generic per-axis passes that accumulate in float64); it is tested per
    voxel to |y - y64| <= c . 2^-24 . B (B: the same filter of |input| with |weights| and |cval|; c: the sum over the
    filtered axes of taps + 2), and to the suite's 1e-6 max-norm on non-negative data."""
    input = S.as_device(input)
    output = S.get_output(output, input)
    sizes = S.normalize_sequence(size, input.ndim)
    origins = S.normalize_sequence(origin, input.ndim)
    modes = S.normalize_sequence(mode, input.ndim)
    for m in modes:
        S.check_mode(m)
    axes = [(ax, int(sizes[ax]), int(origins[ax]), modes[ax]) for ax in range(input.ndim)
            if sizes[ax] > 1]
    for _, sz, og, _m in axes:
        S.check_origin(og, sz)
    if any(m == "constant" for _, _, _, m in axes):
        S.check_cval("constant", cval, output.dtype.kind in "iu")
    S.acc_flag(dtype_mode)
    if not axes:
        output[...] = input
        return output
    if input.size == 0:
        return output

    # fused single-launch path (3-D float32)
    if input.ndim in (2, 3):
        nd = input.ndim
        w3, o3, m3 = [None] * nd, [0] * nd, ["reflect"] * nd
        for ax, sz, og, m in axes:
            w3[ax], o3[ax], m3[ax] = np.full((sz,), 1.0 / sz), og, m
        res = _try_fused_3d(input, output, w3, o3, m3, cval, True)
        if res is not None:
            return res

    if (dtype_mode != "float" and input.dtype in (np.uint8, np.uint16, np.int16) and output.dtype == input.dtype
            and input.ndim in (2, 3)):
        res = _try_uniform_integer(input, output, sizes, origins, modes, cval)
        if res is not None:
            return res
        if (input.shape[-1] * input.dtype.itemsize) % 16 and S.current_planes() is None and int(origins[-1]) == 0 and int(sizes[-1]) % 2:
            # rows that are not a multiple of 16 bytes: the integer box kernels on explicitly extended rows (r4b)
            reach = int(sizes[-1]) // 2
            modes_x = list(modes[:-1]) + ["nearest"]
            res = _run_on_extended_rows(input, output, reach, reach, modes[-1], cval,
                                        lambda e, o: _try_uniform_integer(e, o, sizes, origins, modes_x, cval),
                                        key=("box-int", tuple(int(v) for v in sizes), tuple(int(v) for v in origins), tuple(modes_x), float(cval)))
            if res is not None:
                return res

    if dtype_mode == "float":
        passes = [(lambda s, d, ax=ax, sz=sz, og=og, m=m:
                   _launch_correlate1d(s, d, ax, np.full((sz,), 1.0 / sz), og, m, cval, 1))
                  for ax, sz, og, m in axes]
    else:
        passes = [(lambda s, d, ax=ax, sz=sz, og=og, m=m: _launch_uniform1d(s, d, ax, sz, og, m, cval))
                  for ax, sz, og, m in axes]
    return S.run_passes(input, output, passes)


# ----------------------------------------------------------------------------
# gaussian
# ----------------------------------------------------------------------------
def _gaussian_kernel1d(sigma, order, radius):
    """1-D Gaussian (derivative) kernel, float64, on the host
    (filters.py:795-825).  phi(x) = exp(-x^2 / 2 sigma^2) / sum; the n-th
    derivative is q_n(x) phi(x) with q_0 = 1 and q_{k+1} = q_k' - x q_k / sigma^2,
    carried here as polynomial coefficients."""
    if order < 0:
        raise ValueError("order must be non-negative")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi /= phi.sum()
    if order == 0:
        return phi
    poly = np.polynomial.polynomial
    q = np.array([1.0])
    slope = np.array([0.0, -1.0 / (sigma * sigma)])
    for _ in range(order):
        q = poly.polyadd(poly.polyder(q), poly.polymul(q, slope))
    return poly.polyval(x.astype(np.float64), q) * phi


_GAUSS_CACHE = {}


def _gaussian_weights(sigma, order, truncate):
    key = (float(sigma), int(order), float(truncate))
    w = _GAUSS_CACHE.get(key)
    if w is None:
        sd = float(sigma)
        lw = int(truncate * sd + 0.5)
        # correlate, not convolve: revert the kernel (filters.py:716-718)
        w = _gaussian_kernel1d(sigma, order, lw)[::-1].copy()
        w.setflags(write=False)         # shared between calls
        if len(_GAUSS_CACHE) > 256:
            _GAUSS_CACHE.clear()
        _GAUSS_CACHE[key] = w
    return w


def gaussian_filter1d(input, sigma, axis=-1, order=0, output=None, mode="reflect", cval=0.0,
                      truncate=4.0, *, dtype_mode="ndimage"):
    """One-dimensional Gaussian filter (filters.py:668-722)."""
    weights = _gaussian_weights(sigma, order, truncate)
    return correlate1d(input, weights, axis, output, mode, cval, 0, dtype_mode=dtype_mode)


def gaussian_filter(input, sigma, order=0, output=None, mode="reflect", cval=0.0, truncate=4.0, *,
                    dtype_mode="ndimage"):
    """Multi-dimensional Gaussian filter (filters.py:725-792).

    Precision: on 2-D / 3-D float32 inputs the fused kernel, where it takes the call, accumulates in float32 whatever
    `dtype_mode` says (calls it declines run generic per-axis passes that accumulate in float64); it is tested per
    voxel to |y - y64| <= c . 2^-24 . B (B: the same filter of |input| with |weights| and |cval|; c: the sum over the
    filtered axes of taps + 2), and to the suite's 1e-6 max-norm on non-negative data."""
    input = S.as_device(input)
    output = S.get_output(output, input)
    orders = S.normalize_sequence(order, input.ndim)
    sigmas = S.normalize_sequence(sigma, input.ndim)
    modes = S.normalize_sequence(mode, input.ndim)
    for m in modes:
        S.check_mode(m)
    axes = [(ax, sigmas[ax], orders[ax], modes[ax]) for ax in range(input.ndim) if sigmas[ax] > 1e-15]
    acc = S.acc_flag(dtype_mode)
    if not axes:
        output[...] = input
        return output
    weights = {ax: _gaussian_weights(sg, od, truncate) for ax, sg, od, _ in axes}
    if any(m == "constant" for _, _, _, m in axes):
        S.check_cval("constant", cval, output.dtype.kind in "iu")
    if input.size == 0:
        return output

    if input.ndim in (2, 3):
        nd = input.ndim
        w3, o3, m3 = [None] * nd, [0] * nd, ["reflect"] * nd
        for ax, _sg, _od, m in axes:
            w3[ax], m3[ax] = weights[ax], m
        res = _try_fused_3d(input, output, w3, o3, m3, cval, False)
        if res is not None:
            return res

    passes = [(lambda s, d, ax=ax, m=m: _launch_correlate1d(s, d, ax, weights[ax], 0, m, cval, acc))
              for ax, _sg, _od, m in axes]
    return S.run_passes(input, output, passes)


# ----------------------------------------------------------------------------
# min / max
# ----------------------------------------------------------------------------
def _check_size_footprint_structure(ndim, size, footprint, structure, stacklevel=3):
    """_filters_core.py:14-48, with footprint/structure kept on the host."""
    if structure is None and footprint is None:
        if size is None:
            raise RuntimeError("no footprint or filter size provided")
        sizes = S.fix_sequence_arg(size, ndim, "size", int)
        return sizes, None, None
    if size is not None:
        warnings.warn("ignoring size because {} is set".format(
            "structure" if footprint is None else "footprint"), UserWarning, stacklevel=stacklevel + 1)
    if footprint is not None:
        footprint = np.ascontiguousarray(S.as_host(footprint), dtype=bool)
        if not footprint.any():
            raise ValueError("all-zero footprint is not supported")
    if structure is None:
        if footprint.all():
            if footprint.ndim != ndim:
                raise RuntimeError("size must have length equal to input rank")
            return list(footprint.shape), None, None
        return None, footprint, None
    structure = np.ascontiguousarray(S.as_host(structure))
    if footprint is None:
        footprint = np.ones(structure.shape, bool)
    return None, footprint, structure


def _launch_minmax1d(src, dst, axis, size, origin, mode, cval, is_max):
    a, b = src._desc(), dst._desc()
    S.check(S.lib().mi_minmax1d(ctypes.byref(a), ctypes.byref(b), axis, int(size), int(origin),
                                S.mode_code(mode), float(cval), int(is_max), None))


def _minmax_planes(input, output, sizes, origins, modes, cval, is_max, planes):
    """Plane-restricted separable min / max (multi-GPU slabs): uint8 cubic 3 / 5 / 7 and float32 cubic 3 .. 9 volumes
    through mi_minmax3d_u8_planes / mi_minmax3d_f32_planes; anything else raises Unsupported (the caller falls back to
    the plain schedule on the whole extended slab)."""
    if (input.ndim != 3 or input.dtype not in (np.uint8, np.float32) or output.dtype != input.dtype or
            not input._is_c_contiguous() or not output._is_c_contiguous() or core.shares_memory(output, input)):
        raise S.Unsupported("plane-restricted min/max filters need contiguous, distinct uint8 / float32 volumes")
    flat = [int(v) for pr in planes for v in pr]
    pl = S.c_int64s(flat)
    a, b = input._desc(), output._desc()
    args = (ctypes.byref(a), ctypes.byref(b), _cached_ints(tuple(int(v) for v in sizes)), _cached_ints(tuple(int(v) for v in origins)),
            _cached_ints(tuple(S.mode_code(m) for m in modes)))
    if input.dtype == np.uint8:
        if any(m in ("constant", "grid-constant") for m in modes) and not (np.isfinite(cval) and 0 <= cval <= 255 and float(cval) == int(cval)):
            raise S.Unsupported("cval outside uint8")
        cv = int(cval) if np.isfinite(cval) and 0 <= cval <= 255 else 0
        S.check(S.lib().mi_minmax3d_u8_planes(*args, cv, int(is_max), pl, len(planes), None))
    else:
        S.check(S.lib().mi_minmax3d_f32_planes(*args, float(cval), int(is_max), pl, len(planes), None))
    return output


def _try_fused_minmax_u8(input, output, sizes, origins, modes, cval, is_max):
    if S.current_planes() is not None:
        return _minmax_planes(input, output, sizes, origins, modes, cval, is_max, S.current_planes())
    if (input.ndim not in (2, 3) or input.dtype not in (np.uint8, np.uint16, np.int16) or output.dtype != input.dtype
            or input.size == 0):
        return None
    info = np.iinfo(input.dtype)
    out3 = output
    if input.ndim == 2:
        # an image is a one-plane volume: x and y windows in one streaming launch
        as3 = lambda a: a._as3()   # noqa: E731
        input, out3 = as3(input), as3(output)
        sizes, origins, modes = [1] + list(sizes), [0] + list(origins), ["reflect"] + list(modes)
    src = core.ascontiguousarray(input)
    direct = out3._is_c_contiguous() and not core.shares_memory(out3, src)
    dst = out3 if direct else core.empty(out3.shape, out3.dtype)
    a, b = src._desc(), dst._desc()
    # SciPy compares cval as a double and casts after every pass; the byte
    # kernel is only equivalent when cval is itself a uint8 value
    if any(m in ("constant", "grid-constant") for m in modes):
        if not (np.isfinite(cval) and info.min <= cval <= info.max and float(cval) == int(cval)):
            return None
    if any(int(o) != 0 for o in origins) or any(int(sz) % 2 == 0 for sz in sizes):
        return None
    entry = S.lib().mi_minmax3d_u8 if input.dtype == np.uint8 else S.lib().mi_minmax3d_16
    try:
        cv = int(cval) if np.isfinite(cval) and info.min <= cval <= info.max else 0
        S.check(entry(ctypes.byref(a), ctypes.byref(b), _cached_ints(tuple(int(v) for v in sizes)),
                      _cached_ints(tuple(int(v) for v in origins)), _cached_ints(tuple(S.mode_code(m) for m in modes)),
                      cv, int(is_max), None))
    except S.Unsupported:
        return None
    if not direct:
        out3[...] = dst
    return output


def _try_stream_minmax_f32(input, output, sizes, origins, modes, cval, is_max):
    """Separable flat min / max on float32 volumes and images: streaming
    passes (mi_minmax3d_f32) instead of one generic launch per axis."""
    if S.current_planes() is not None:
        raise S.Unsupported("min/max filters cannot be restricted to a range of output planes")
    if input.dtype not in (np.float32, np.float64) or output.dtype != input.dtype or input.size == 0:
        return None
    if any(int(sz) % 2 == 0 or int(sz) > 9 for sz in sizes) or int(origins[-1]) != 0:
        return None
    entry = S.lib().mi_minmax3d_f32 if input.dtype == np.float32 else S.lib().mi_minmax3d_f64
    if input.ndim == 2:
        as3 = lambda a: a._as3()   # noqa: E731
        in3, out3 = as3(input), as3(output)
        sizes, origins, modes = [1] + list(sizes), [0] + list(origins), ["reflect"] + list(modes)
    else:
        in3, out3 = input, output
    src = core.ascontiguousarray(in3)
    direct = out3._is_c_contiguous() and not core.shares_memory(out3, src)
    dst = out3 if direct else core.empty(out3.shape, out3.dtype)
    a, b = src._desc(), dst._desc()
    try:
        S.check(entry(ctypes.byref(a), ctypes.byref(b), _cached_ints(tuple(int(v) for v in sizes)),
                      _cached_ints(tuple(int(v) for v in origins)), _cached_ints(tuple(S.mode_code(m) for m in modes)),
                      float(cval), int(is_max), None))
    except S.Unsupported:
        return None
    if not direct:
        out3[...] = dst
    return output


_RUNS_CACHE = {}


def _footprint_runs(fp):
    """Half widths of the rows of a 2-D footprint whose rows are centred runs (disk, diamond, cross, square, octagon),
    or None: row r covers columns -hw[r] .. +hw[r] about the centre column, -1 = empty row.  Memoised on the mask."""
    key = (fp.shape, fp.tobytes())
    if key not in _RUNS_CACHE:
        if len(_RUNS_CACHE) > 256:
            _RUNS_CACHE.clear()
        _RUNS_CACHE[key] = _footprint_runs_uncached(fp)
    return _RUNS_CACHE[key]


def _footprint_runs_uncached(fp):
    h, w = fp.shape
    if h % 2 == 0 or w % 2 == 0 or h > 9 or w > 9:
        return None
    c = w // 2
    runs = []
    for row in fp:
        nz = np.flatnonzero(row)
        if nz.size == 0:
            runs.append(-1)
            continue
        lo, hi = int(nz[0]), int(nz[-1])
        if hi - lo + 1 != nz.size or c - lo != hi - c:
            return None
        runs.append(hi - c)
    return runs


def _footprint_runs3d(fp):
    """half widths (-1 / 0 / 1) of the nine x rows of a 3 x 3 x (1 or 3) footprint, or None"""
    if fp.ndim != 3 or fp.shape[0] != 3 or fp.shape[1] != 3 or fp.shape[2] not in (1, 3):
        return None
    runs = _footprint_runs(fp.reshape(9, fp.shape[2]))
    return runs


def _try_runs3d_minmax_u8(input, output, fp, mode, cval, is_max):
    """uint8 / bool volumes, 3 x 3 x 3 footprints of centred runs (6- / 18- / 26-connected structures): one streaming
    launch."""
    if input.ndim != 3 or input.dtype not in (np.uint8, np.bool_) or output.dtype != input.dtype or input.size == 0:
        return None
    runs = _footprint_runs3d(fp)
    if runs is None:
        return None
    if mode in ("constant", "grid-constant") and not (np.isfinite(cval) and 0 <= cval <= 255 and float(cval) == int(cval)):
        return None
    src = core.ascontiguousarray(input)
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    a, b = src._desc(), dst._desc()
    try:
        cv = int(cval) if np.isfinite(cval) and 0 <= cval <= 255 else 0
        S.check(S.lib().mi_minmax_runs3d_u8(ctypes.byref(a), ctypes.byref(b), _cached_ints(tuple(runs)),
                                            _cached_ints((S.mode_code(mode),) * 3), cv, int(is_max), None))
    except S.Unsupported:
        return None
    if not direct:
        output[...] = dst
    return output


def _try_runs_minmax_u8(input, output, fp, mode, cval, is_max):
    """uint8 / uint16 / int16 images (volumes with a one-plane footprint): footprints made of centred runs in one
    streaming launch."""
    if S.current_planes() is not None or input.ndim not in (2, 3) or fp.ndim != input.ndim or input.size == 0:
        return None
    if fp.ndim == 3 and fp.shape[0] != 1:
        return _try_runs3d_minmax_u8(input, output, fp, mode, cval, is_max)
    if fp.ndim == 3:
        fp = fp[0]
    runs = _footprint_runs(fp)
    if runs is None:
        return None
    is_float = input.dtype == np.float32
    if not is_float:
        info = np.iinfo(input.dtype)
        if mode in ("constant", "grid-constant") and not (np.isfinite(cval) and info.min <= cval <= info.max
                                                          and float(cval) == int(cval)):
            return None
    if is_float:
        entry = S.lib().mi_minmax_runs_f32
    else:
        entry = S.lib().mi_minmax_runs_u8 if input.dtype == np.uint8 else S.lib().mi_minmax_runs_16
    src = core.ascontiguousarray(input)
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    a, b = src._desc(), dst._desc()
    try:
        if is_float:
            cv = float(cval)
        else:
            cv = int(cval) if np.isfinite(cval) and info.min <= cval <= info.max else 0
        S.check(entry(ctypes.byref(a), ctypes.byref(b), len(runs), _cached_ints(tuple(runs)),
                      _cached_ints((S.mode_code(mode),) * 2), cv, int(is_max), None))
    except S.Unsupported:
        return None
    if not direct:
        output[...] = dst
    return output


def _min_or_max_filter(input, size, ftprnt, structure, output, mode, cval, origin, func):
    """filters.py:1373-1419"""
    input = S.as_device(input)
    is_max = func == "max"
    sizes, ftprnt, structure = _check_size_footprint_structure(input.ndim, size, ftprnt, structure)
    if cval is np.nan or (isinstance(cval, float) and np.isnan(cval)):
        raise NotImplementedError("NaN cval is unsupported")

    if sizes is not None:
        # separable: a series of 1-D passes (filters.py:1385-1396)
        output = S.get_output(output, input)
        modes = S.fix_sequence_arg(mode, input.ndim, "mode", S.check_mode)
        origins = S.fix_sequence_arg(origin, input.ndim, "origin", int)
        axes = [(ax, sizes[ax], origins[ax], modes[ax]) for ax in range(input.ndim) if sizes[ax] > 1]
        for _, sz, og, _m in axes:
            S.check_origin(og, sz)
        if not axes:
            output[...] = input
            return output
        if input.size == 0:
            return output
        if input.ndim in (2, 3):
            res = _try_fused_minmax_u8(input, output, sizes, origins, modes, cval, is_max)
            if res is not None:
                return res
        if input.ndim in (2, 3):
            res = _try_stream_minmax_f32(input, output, sizes, origins, modes, cval, is_max)
            if res is not None:
                return res
        if (input.ndim in (2, 3) and S.current_planes() is None and output.dtype == input.dtype and int(origins[-1]) == 0
                and input.dtype in (np.uint8, np.uint16, np.int16, np.float32, np.float64)
                and (input.shape[-1] * input.dtype.itemsize) % 16 and all(int(sz) % 2 == 1 for sz in sizes)):
            # rows that are not a multiple of 16 bytes: the fused kernels on explicitly extended rows (r4b; r5: float64 too)
            fused = _try_stream_minmax_f32 if input.dtype in (np.float32, np.float64) else _try_fused_minmax_u8
            reach = int(sizes[-1]) // 2
            modes_x = list(modes[:-1]) + ["nearest"]
            res = _run_on_extended_rows(input, output, reach, reach, modes[-1], cval,
                                        lambda e, o: fused(e, o, sizes, origins, modes_x, cval, is_max),
                                        key=("minmax", tuple(int(v) for v in sizes), tuple(int(v) for v in origins), tuple(modes_x), float(cval), bool(is_max)))
            if res is not None:
                return res
        passes = [(lambda s, d, ax=ax, sz=sz, og=og, m=m: _launch_minmax1d(s, d, ax, sz, og, m, cval, is_max))
                  for ax, sz, og, m in axes]
        return S.run_passes(input, output, passes)

    S.check_mode(mode)
    fdims = [x for x in ftprnt.shape if x != 0]
    if len(fdims) != input.ndim:
        raise RuntimeError("footprint array has incorrect shape")
    origins = S.fix_sequence_arg(origin, len(fdims), "origin", int)
    for o, wd in zip(origins, fdims):
        S.check_origin(o, wd)
    if structure is not None and structure.ndim != input.ndim:
        raise RuntimeError("structure array has incorrect shape")
    if ftprnt.size == 0:
        return core.zeros_like(input)
    output = S.get_output(output, input)
    if input.size == 0:
        return output
    fp = np.ascontiguousarray(ftprnt, dtype=np.uint8)
    if (structure is None and input.dtype in (np.uint8, np.uint16, np.int16, np.float32) and output.dtype == input.dtype
            and not any(origins)):
        res = _try_runs_minmax_u8(input, output, fp, mode, cval, is_max)
        if res is not None:
            return res
    fpp = fp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    if structure is not None:
        st, stp = S.c_doubles(structure)
    else:
        st, stp = None, ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
    fshape = S.c_int64s(fp.shape)
    org = S.c_ints(origins)

    def launch(src, dst):
        a, b = src._desc(), dst._desc()
        S.check(S.lib().mi_minmax_nd(ctypes.byref(a), ctypes.byref(b), fpp, stp, fshape, org,
                                     S.mode_code(mode), float(cval), int(is_max), None))

    return S.run_kernel(input, output, launch)


def minimum_filter(input, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """Multi-dimensional minimum filter (filters.py:1291-1329)."""
    return _min_or_max_filter(input, size, footprint, None, output, mode, cval, origin, "min")


def maximum_filter(input, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """Multi-dimensional maximum filter (filters.py:1332-1370)."""
    return _min_or_max_filter(input, size, footprint, None, output, mode, cval, origin, "max")


def _min_or_max_1d(input, size, axis, output, mode, cval, origin, func):
    """filters.py:1478-1507"""
    input = S.as_device(input)
    size = int(size)
    if size < 1:
        raise RuntimeError("incorrect filter size")
    S.check_mode(mode)
    axis = S.normalize_axis(axis, input.ndim)
    origin = S.check_origin(origin, size)
    output = S.get_output(output, input)
    if input.ndim == 0 or input.size == 0:
        return output
    return S.run_kernel(input, output,
                        lambda s, d: _launch_minmax1d(s, d, axis, size, origin, mode, cval, func == "max"))


def minimum_filter1d(input, size, axis=-1, output=None, mode="reflect", cval=0.0, origin=0):
    """Minimum filter along a single axis (filters.py:1422-1447)."""
    return _min_or_max_1d(input, size, axis, output, mode, cval, origin, "min")


def maximum_filter1d(input, size, axis=-1, output=None, mode="reflect", cval=0.0, origin=0):
    """Maximum filter along a single axis (filters.py:1450-1475)."""
    return _min_or_max_1d(input, size, axis, output, mode, cval, origin, "max")


# ----------------------------------------------------------------------------
# derivative filters: compositions of the 1-D passes (filters.py:828-1252)
# ----------------------------------------------------------------------------
def _derivative_then_smooth(input, axis, output, mode, cval, smooth, dtype_mode="ndimage"):
    S.acc_flag(dtype_mode)
    input = S.as_device(input)
    axis = S.normalize_axis(axis, input.ndim)
    output = S.get_output(output, input)
    modes = S.normalize_sequence(mode, input.ndim)
    if input.ndim in (2, 3) and input.dtype in (np.float32, np.float64) and output.dtype == input.dtype and input.size:
        # a separable product of 3-tap kernels: one fused launch for float32 / float64 images and volumes
        for m in modes:
            S.check_mode(m)
        w = [np.asarray([-1.0, 0.0, 1.0]) if ii == axis else np.asarray(smooth, dtype=np.float64) for ii in range(input.ndim)]
        res = _try_fused_3d(input, output, w, [0] * input.ndim, list(modes), cval, False)
        if res is not None:
            return res
    correlate1d(input, [-1, 0, 1], axis, output, modes[axis], cval, 0, dtype_mode=dtype_mode)
    for ii in range(input.ndim):
        if ii != axis:
            correlate1d(output, smooth, ii, output, modes[ii], cval, 0, dtype_mode=dtype_mode)
    return output


def prewitt(input, axis=-1, output=None, mode="reflect", cval=0.0, *, dtype_mode="ndimage"):
    """Prewitt filter (filters.py:828-886): derivative along `axis`, [1, 1, 1] along the others; `dtype_mode` is
    handed to every 1-D pass as in the reference (filters.py:835, 876-884).

    Precision: on 2-D / 3-D float32 inputs the fused kernel, where it takes the call, accumulates in float32 whatever
    `dtype_mode` says (calls it declines run generic per-axis passes that accumulate in float64); it is tested per
    voxel to |y - y64| <= c . 2^-24 . B (B: the same filter of |input| with |weights| and |cval|; c: the sum over the
    filtered axes of taps + 2), which is the only bound a derivative of offset data can meet in float32."""
    return _derivative_then_smooth(input, axis, output, mode, cval, [1, 1, 1], dtype_mode)


def sobel(input, axis=-1, output=None, mode="reflect", cval=0.0, *, dtype_mode="ndimage"):
    """Sobel filter (filters.py:889-940): derivative along `axis`, [1, 2, 1] along the others; `dtype_mode` as in
    `prewitt` (filters.py:896).

    Precision: on 2-D / 3-D float32 inputs the fused kernel, where it takes the call, accumulates in float32 whatever
    `dtype_mode` says (calls it declines run generic per-axis passes that accumulate in float64); it is tested per
    voxel to |y - y64| <= c . 2^-24 . B (B: the same filter of |input| with |weights| and |cval|; c: the sum over the
    filtered axes of taps + 2), which is the only bound a derivative of offset data can meet in float32."""
    return _derivative_then_smooth(input, axis, output, mode, cval, [1, 2, 1], dtype_mode)


def generic_laplace(input, derivative2, output=None, mode="reflect", cval=0.0, extra_arguments=(),
                    extra_keywords=None):
    """Sum over the axes of a caller-supplied second derivative (filters.py:902-1011)."""
    if extra_keywords is None:
        extra_keywords = {}
    input = S.as_device(input)
    output = S.get_output(output, input)
    if input.ndim == 0:
        output[...] = input
        return output
    modes = S.normalize_sequence(mode, input.ndim)
    derivative2(input, 0, output, modes[0], cval, *extra_arguments, **extra_keywords)
    for ii in range(1, input.ndim):
        tmp = derivative2(input, ii, output.dtype, modes[ii], cval, *extra_arguments, **extra_keywords)
        S.elementwise("add", output, tmp, output)
    return output


def laplace(input, output=None, mode="reflect", cval=0.0, *, dtype_mode="ndimage"):
    """Laplace filter from [1, -2, 1] second differences (filters.py:1041-1075; `dtype_mode` reaches the 1-D passes
    through the derivative callback, filters.py:1067-1073)."""
    S.acc_flag(dtype_mode)

    def derivative2(input, axis, output, mode, cval):
        return correlate1d(input, [1, -2, 1], axis, output, mode, cval, 0, dtype_mode=dtype_mode)
    input = S.as_device(input)
    if input.ndim in (2, 3) and input.dtype == np.float32 and isinstance(mode, str) and (
            output is None or (isinstance(output, core.ndarray) and output.dtype == np.float32)):
        # the sum of the second differences is one (2 ndim + 1)-point stencil: a single tiled launch for float32
        cross = np.zeros((3,) * input.ndim)
        centre = (1,) * input.ndim
        cross[centre] = -2.0 * input.ndim
        for ax in range(input.ndim):
            for d in (0, 2):
                idx = list(centre)
                idx[ax] = d
                cross[tuple(idx)] = 1.0
        return correlate(input, cross, output, mode, cval)
    return generic_laplace(input, derivative2, output, mode, cval)


def gaussian_laplace(input, sigma, output=None, mode="reflect", cval=0.0, **kwargs):
    """Laplace filter from Gaussian second derivatives (filters.py:1046-1087)."""
    input = S.as_device(input)

    def derivative2(input, axis, output, mode, cval, sigma, **kwargs):
        order = [0] * input.ndim
        order[axis] = 2
        return gaussian_filter(input, sigma, order, output, mode, cval, **kwargs)
    return generic_laplace(input, derivative2, output, mode, cval, extra_arguments=(sigma,), extra_keywords=kwargs)


def generic_gradient_magnitude(input, derivative, output=None, mode="reflect", cval=0.0, extra_arguments=(),
                               extra_keywords=None):
    """sqrt of the summed squares of a caller-supplied first derivative (filters.py:1090-1150)."""
    if extra_keywords is None:
        extra_keywords = {}
    input = S.as_device(input)
    output = S.get_output(output, input)
    if input.ndim == 0:
        output[...] = input
        return output
    modes = S.normalize_sequence(mode, input.ndim)
    derivative(input, 0, output, modes[0], cval, *extra_arguments, **extra_keywords)
    S.elementwise("multiply", output, output, output)
    for ii in range(1, input.ndim):
        tmp = derivative(input, ii, output.dtype, modes[ii], cval, *extra_arguments, **extra_keywords)
        S.elementwise("multiply", tmp, tmp, tmp)
        S.elementwise("add", output, tmp, output)
    S.elementwise("sqrt", output, None, output)
    return output


def gaussian_gradient_magnitude(input, sigma, output=None, mode="reflect", cval=0.0, **kwargs):
    """Gradient magnitude from Gaussian first derivatives (filters.py:1153-1197)."""
    input = S.as_device(input)

    def derivative(input, axis, output, mode, cval, sigma, **kwargs):
        order = [0] * input.ndim
        order[axis] = 1
        return gaussian_filter(input, sigma, order, output, mode, cval, **kwargs)
    return generic_gradient_magnitude(input, derivative, output, mode, cval, extra_arguments=(sigma,),
                                      extra_keywords=kwargs)


# ----------------------------------------------------------------------------
# rank / median / percentile (filters.py:1560-1848)
# ----------------------------------------------------------------------------
def _try_median3x3(input, output, mode, cval):
    """3 x 3 median of float32 / uint8 images (volumes: footprint (1, 3, 3)) as one streaming launch."""
    src = core.ascontiguousarray(input)
    direct = output._is_c_contiguous() and not core.shares_memory(output, src)
    dst = output if direct else core.empty(output.shape, output.dtype)
    a, b = src._desc(), dst._desc()
    try:
        S.check(S.lib().mi_median3x3(ctypes.byref(a), ctypes.byref(b), _cached_ints((S.mode_code(mode),) * 2), float(cval), None))
    except S.Unsupported:
        return None
    if not direct:
        output[...] = dst
    return output


def _rank_filter(input, rank, size, footprint, output, mode, cval, origin, operation):
    if size is not None and footprint is not None:
        warnings.warn("ignoring size because footprint is set", UserWarning, stacklevel=3)
    input = S.as_device(input)
    _check_real(input)
    if footprint is None:
        if size is None:
            raise RuntimeError("no footprint or filter size provided")
        sizes = S.normalize_sequence(size, input.ndim)
        footprint = np.ones([int(v) for v in sizes], dtype=bool)
    else:
        footprint = S.as_host(footprint).astype(bool)
    origins = S.fix_sequence_arg(origin, input.ndim, "origin", int)
    fshape = [ii for ii in footprint.shape if ii > 0]
    if len(fshape) != input.ndim:
        raise RuntimeError("filter footprint array has incorrect shape.")
    for o, lenf in zip(origins, fshape):
        S.check_origin(o, lenf)
    filter_size = int(np.count_nonzero(footprint))
    if operation == "median":
        rank = filter_size // 2
    elif operation == "percentile":
        percentile = rank
        if percentile < 0.0:
            percentile += 100.0
        if percentile < 0 or percentile > 100:
            raise RuntimeError("invalid percentile")
        rank = filter_size - 1 if percentile == 100.0 else int(float(filter_size) * percentile / 100.0)
    rank = int(rank)
    if rank < 0:
        rank += filter_size
    if rank < 0 or rank >= filter_size:
        raise RuntimeError("rank not within filter footprint size")
    if rank == 0:
        return minimum_filter(input, None, footprint, output, mode, cval, origins)
    if rank == filter_size - 1:
        return maximum_filter(input, None, footprint, output, mode, cval, origins)
    if not isinstance(mode, str):
        raise RuntimeError("A sequence of modes is not supported by non-separable rank filters")
    S.check_mode(mode)
    output = S.get_output(output, input)
    if input.size == 0:
        return output
    fp = np.ascontiguousarray(footprint, dtype=np.uint8)
    # the streaming 3 x 3 median never sees the footprint: only the FULL in-plane 3 x 3 window qualifies (a (3, 3, 3)
    # footprint with nine ones in another plane has the same count and trailing shape)
    if (rank == 4 and filter_size == 9 and fp.shape in ((3, 3), (1, 3, 3)) and bool(fp.all()) and fp.ndim == input.ndim
            and not any(origins) and input.dtype in (np.float32, np.float64, np.uint8, np.uint16, np.int16) and output.dtype == input.dtype
            and S.current_planes() is None):
        res = _try_median3x3(input, output, mode, cval)
        if res is not None:
            return res
        if input.dtype.itemsize in (1, 2, 4) and (input.shape[-1] * input.dtype.itemsize) % 16 and mode != "constant":
            # rows that are not a multiple of 16 bytes (r4b).  Not for `constant`: the kernel takes ONE mode for both axes, and
            # on the extended rows the x mode must be one that never supplies a value of its own
            res = _run_on_extended_rows(input, output, 1, 1, mode, cval, lambda e, o: _try_median3x3(e, o, mode, cval),
                                        key=("median3x3", float(cval)))
            if res is not None:
                return res
    fpp = fp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    fsh = S.c_int64s(fp.shape)
    org = S.c_ints(origins)

    def launch(src, dst):
        a, b = src._desc(), dst._desc()
        try:
            S.check(S.lib().mi_rank_filter(ctypes.byref(a), ctypes.byref(b), fpp, fsh, org, rank, S.mode_code(mode),
                                           float(cval), None))
        except S.Unsupported as exc:
            raise NotImplementedError(str(exc))
    return S.run_kernel(input, output, launch)


def rank_filter(input, rank, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """Multidimensional rank filter (filters.py:1704-1748)."""
    return _rank_filter(input, int(rank), size, footprint, output, mode, cval, origin, "rank")


def median_filter(input, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """Multidimensional median filter (filters.py:1751-1792)."""
    return _rank_filter(input, 0, size, footprint, output, mode, cval, origin, "median")


def percentile_filter(input, percentile, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """Multidimensional percentile filter (filters.py:1795-1848)."""
    return _rank_filter(input, percentile, size, footprint, output, mode, cval, origin, "percentile")
