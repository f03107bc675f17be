"""Minimal device ndarray on top of the libmi355img runtime.

The reference takes ``cupy.ndarray`` everywhere (README.md:50-58); this is the
counterpart owned by the engine itself: a pointer into pooled HBM plus
shape / byte strides / dtype.  It supports what the filtering path needs
(creation, host transfer, views by basic slicing and transposition, dtype
casts, ``out[...] = in``) and deliberately nothing more -- it is plumbing, not
an array library.  No CuPy, no PyTorch.
"""
import ctypes
import threading

import numpy as np

from . import _lib
from ._lib import MiArray

_DTYPE_CODES = {
    np.dtype(np.bool_): 0, np.dtype(np.int8): 1, np.dtype(np.uint8): 2,
    np.dtype(np.int16): 3, np.dtype(np.uint16): 4, np.dtype(np.int32): 5,
    np.dtype(np.uint32): 6, np.dtype(np.int64): 7, np.dtype(np.uint64): 8,
    np.dtype(np.float32): 9, np.dtype(np.float64): 10,
    np.dtype(np.float16): 11,      # storage only (mi_copy converts); see scipy.ndimage._support.float16_aware
}


def dtype_code(dtype):
    dtype = np.dtype(dtype)
    try:
        return _DTYPE_CODES[dtype]
    except KeyError:
        raise TypeError("dtype {} is not supported by cupyimg_amd".format(dtype))


class _Memory:
    """Owner of one pooled device allocation."""

    __slots__ = ("ptr", "nbytes", "device", "__weakref__")

    def __init__(self, nbytes):
        lib = _lib.load()
        p = ctypes.c_void_p()
        dev = ctypes.c_int()
        _lib.check(lib.mi_get_device(ctypes.byref(dev)))
        _lib.check(lib.mi_malloc(ctypes.byref(p), max(int(nbytes), 1)))
        self.ptr = p.value
        self.nbytes = int(nbytes)
        self.device = dev.value

    def __del__(self):
        try:
            if self.ptr:
                _lib.load().mi_free(self.ptr)
        except Exception:  # interpreter shutdown
            pass
        self.ptr = None


class _ForeignMemory:
    """Memory owned by someone else (e.g. a torch tensor); kept alive via `owner`."""

    __slots__ = ("ptr", "nbytes", "device", "owner")

    def __init__(self, ptr, nbytes, owner, device=0):
        self.ptr = int(ptr)
        self.nbytes = int(nbytes)
        self.owner = owner
        self.device = device


class _Flags:
    __slots__ = ("c_contiguous",)

    def __init__(self, c):
        self.c_contiguous = c

    def __repr__(self):
        return "  C_CONTIGUOUS : {}".format(self.c_contiguous)


def _c_strides(shape, itemsize):
    strides = []
    st = itemsize
    for s in reversed(shape):
        strides.append(st)
        st *= max(int(s), 1)
    return tuple(reversed(strides))


class ndarray:
    """Device array: pointer + shape + byte strides + dtype."""

    __slots__ = ("_mem", "ptr", "shape", "strides", "dtype", "base", "_dc", "_v3", "_hc")

    def __init__(self, shape, dtype=np.float32, _mem=None, _ptr=None, _strides=None, _base=None):
        if np.isscalar(shape):
            shape = (int(shape),)
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) > _lib.MI_MAX_NDIM:
            raise ValueError("at most {} dimensions are supported".format(_lib.MI_MAX_NDIM))
        self.dtype = np.dtype(dtype)
        dtype_code(self.dtype)
        if _mem is None:
            _mem = _Memory(self.size * self.dtype.itemsize)
            _ptr = _mem.ptr
        self._mem = _mem
        self.ptr = int(_ptr)
        self.strides = tuple(_strides) if _strides is not None else _c_strides(self.shape, self.dtype.itemsize)
        self.base = _base
        self._dc = None         # cached C-ABI descriptor: (shape, strides, ptr, MiArray)
        self._v3 = None         # cached one-plane-volume view of an image
        self._hc = None         # host copy of a small constant array (structuring elements), see host_hint()

    # ------------------------------------------------------------- properties
    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    @property
    def itemsize(self):
        return self.dtype.itemsize

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def device(self):
        return self._mem.device

    @property
    def flags(self):
        return _Flags(self._is_c_contiguous())

    @property
    def real(self):
        return self

    @property
    def T(self):
        return self.transpose()

    def _is_c_contiguous(self):
        expect = self.dtype.itemsize
        for s, st in zip(reversed(self.shape), reversed(self.strides)):
            if s == 0:
                return True
            if s != 1 and st != expect:
                return False
            expect *= s
        return True

    def __len__(self):
        if not self.shape:
            raise TypeError("len() of unsized object")
        return self.shape[0]

    def __repr__(self):
        return "cupyimg_amd.ndarray(shape={}, dtype={}, device={})".format(self.shape, self.dtype, self.device)

    def __array__(self, *args, **kwargs):
        raise TypeError("implicit conversion to a NumPy array is not allowed; use .get()")

    @property
    def __cuda_array_interface__(self):
        """Version 3.  By default the library's default stream is synchronised
        before the pointer is handed out and `stream` is None ("no
        synchronisation required"): torch.as_tensor ignores the `stream` entry
        (measured: it read the array before the filter had run), so naming the
        stream alone is not safe.  With ``core.EXPORT_SYNC = False`` the entry
        names the library's default stream instead and a protocol-abiding
        consumer (CuPy) orders its own stream behind it without a host sync."""
        if EXPORT_SYNC:
            _lib.check(_lib.load().mi_stream_sync(None))
        return {
            "shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False),
            "strides": None if self._is_c_contiguous() else self.strides, "version": 3,
            "stream": None if EXPORT_SYNC else default_stream_handle(),
        }

    # ------------------------------------------------------------- C-ABI view
    def _desc(self):
        # the descriptor is read-only for the library, so one per array object is enough (a filter call on a small
        # image is bound by this Python layer: building two descriptors cost 3 of its ~20 us)
        c = self._dc
        if c is not None and c[0] is self.shape and c[1] is self.strides and c[2] == self.ptr:
            return c[3]
        d = MiArray()
        d.data = self.ptr
        d.dtype = dtype_code(self.dtype)
        d.ndim = self.ndim
        for i, (s, st) in enumerate(zip(self.shape, self.strides)):
            d.shape[i] = s
            d.strides[i] = st
        self._dc = (self.shape, self.strides, self.ptr, d)
        return d

    def _as3(self):
        """An image as a one-plane volume (what the fused 3-D kernels take); cached."""
        v = self._v3
        if v is None or v.ptr != self.ptr or v.shape[1:] != self.shape:
            # no strong reference back to `self` (array -> _v3 -> base -> array would keep the device buffer alive
            # until the cyclic collector runs): the view shares `_mem`, which is what owns the allocation
            v = ndarray((1,) + self.shape, self.dtype, _mem=self._mem, _ptr=self.ptr,
                        _strides=(self.strides[0] * self.shape[0],) + self.strides, _base=self.base)
            self._v3 = v
        return v

    # ------------------------------------------------------------- transfers
    def get(self):
        """Copy to a new NumPy array (synchronises the default stream)."""
        src = self if self._is_c_contiguous() else self.copy()
        out = np.empty(self.shape, self.dtype)
        if out.nbytes:
            _lib.check(_lib.load().mi_memcpy_d2h(out.ctypes.data, src.ptr, out.nbytes, None))
        return out

    def set(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype).reshape(np.shape(arr))     # (ascontiguousarray makes 0-d one-dimensional)
        if arr.shape != self.shape:
            raise ValueError("shape mismatch")
        self._touch()
        if self._is_c_contiguous():
            if arr.nbytes:
                lib = _lib.load()
                _lib.check(lib.mi_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes, None))
                # the source is pageable host memory: wait so it may be reused
                _lib.check(lib.mi_stream_sync(None))
        else:
            self[...] = asarray(arr)

    # ------------------------------------------------------------- copies / casts
    def copy(self):
        out = ndarray(self.shape, self.dtype)
        _copy(self, out)
        return out

    def astype(self, dtype, copy=True):
        dtype = np.dtype(dtype)
        if dtype == self.dtype and not copy:
            return self
        out = ndarray(self.shape, dtype)
        _copy(self, out)
        return out

    def _touch(self):
        """The array is about to be written: drop the remembered host copy (with_host_hint) of this array and of the
        array it is a view of."""
        self._hc = None
        b = self.base
        if b is not None:
            b._hc = None

    def fill(self, value):
        self._touch()
        if self.dtype == np.float16 or (self.dtype.kind in "iu" and self.dtype.itemsize == 8 and _is_wide_integer(value)):
            # mi_fill takes the value as a double: 64-bit integers beyond 2**53 would come out rounded (and 2**63 - 1
            # overflow the cast), and float16 is not a type it computes in.  The value is converted on the host, as NumPy
            # converts it, and copied from one device element to every element (a source with zero strides).
            one = ndarray((1,), self.dtype)
            one.set(np.asarray(value, dtype=self.dtype).reshape(1))
            _copy(one._view(self.shape, (0,) * self.ndim, one.ptr), self)
            return
        d = self._desc()
        _lib.check(_lib.load().mi_fill(ctypes.byref(d), float(value), None))

    # ------------------------------------------------------------- views
    def _view(self, shape, strides, ptr):
        return ndarray(shape, self.dtype, _mem=self._mem, _ptr=ptr, _strides=strides,
                       _base=self if self.base is None else self.base)

    def transpose(self, *axes):
        if not axes or axes == (None,):
            axes = tuple(reversed(range(self.ndim)))
        elif len(axes) == 1 and hasattr(axes[0], "__iter__"):
            axes = tuple(axes[0])
        if sorted(a % self.ndim for a in axes) != list(range(self.ndim)):
            raise ValueError("axes don't match array")
        axes = [a % self.ndim for a in axes]
        return self._view([self.shape[a] for a in axes], [self.strides[a] for a in axes], self.ptr)

    def reshape(self, *shape):
        if len(shape) == 1 and hasattr(shape[0], "__iter__"):
            shape = tuple(shape[0])
        shape = list(shape)
        if shape.count(-1) > 1:
            raise ValueError("can only specify one unknown dimension")
        if -1 in shape:
            known = 1
            for s in shape:
                if s != -1:
                    known *= s
            shape[shape.index(-1)] = self.size // known if known else 0
        n = 1
        for s in shape:
            n *= s
        if n != self.size:
            raise ValueError("cannot reshape array of size {} into shape {}".format(self.size, tuple(shape)))
        src = self if self._is_c_contiguous() else self.copy()
        return src._view(shape, _c_strides(shape, self.dtype.itemsize), src.ptr)

    def ravel(self):
        return self.reshape(-1)

    def __getitem__(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        if any(k is Ellipsis for k in key):
            i = [k is Ellipsis for k in key].index(True)
            nfill = self.ndim - sum(1 for k in key if k is not None and k is not Ellipsis)
            key = key[:i] + (slice(None),) * nfill + key[i + 1:]
        shape, strides, ptr, dim = [], [], self.ptr, 0
        for k in key:
            if k is None:
                shape.append(1)
                strides.append(0)
                continue
            if dim >= self.ndim:
                raise IndexError("too many indices for array")
            n, st = self.shape[dim], self.strides[dim]
            if isinstance(k, slice):
                start, stop, step = k.indices(n)
                length = len(range(start, stop, step))
                ptr += start * st
                shape.append(length)
                strides.append(st * step)
            else:
                k = int(k)
                if k < -n or k >= n:
                    raise IndexError("index out of bounds")
                ptr += (k % n) * st
            dim += 1
        shape += list(self.shape[dim:])
        strides += list(self.strides[dim:])
        return self._view(shape, strides, ptr)

    def __setitem__(self, key, value):
        self._touch()
        dst = self[key]
        if isinstance(value, ndarray):
            src = value
        elif np.isscalar(value) or (isinstance(value, np.ndarray) and value.ndim == 0):
            dst.fill(value)
            return
        else:
            src = asarray(np.asarray(value))
        if src.shape != dst.shape:
            # shapes that agree once unit axes are dropped; nothing else (a (6, 4) source is not a (4, 6) one)
            if [s for s in src.shape if s != 1] == [s for s in dst.shape if s != 1]:
                src = src.reshape(dst.shape)
            else:
                raise ValueError("could not broadcast input array from shape {} into shape {}".format(
                    src.shape, dst.shape))
        _copy(src, dst)


    # ------------------------------------------------------------- ordering (csrc/threshold.hip: mi_compare)
    def __gt__(self, other):
        return _compare(self, other, 0)

    def __ge__(self, other):
        return _compare(self, other, 1)

    def __lt__(self, other):
        return _compare(self, other, 2)

    def __le__(self, other):
        return _compare(self, other, 3)


_CMP_INT, _CMP_F32, _CMP_F64 = 0, 1, 2


def _compare(a, other, op):
    """a > / >= / < / <= other as a C-contiguous bool device array from one launch, compared as NumPy 2 compares
    `a.get()` with `other`: in the common dtype of the two (a Python int or float is a weak scalar: a uint8 image against a
    Python float compares in float64, a float32 image against one in float32), integers of any two dtypes exactly, NaN
    false.  `other`: a Python or NumPy scalar, or a device array of a's shape; anything else is left to Python (TypeError).
    float16 operands are widened to float32 (exact; no kernel computes in float16) and strided ones compacted first."""
    scalar = None
    if isinstance(other, ndarray):
        if other.shape != a.shape:
            raise ValueError("operands could not be broadcast together with shapes {} {} (comparisons take a scalar or an "
                             "array of the same shape)".format(a.shape, other.shape))
        common = np.result_type(a.dtype, other.dtype)
        kinds = a.dtype.kind + other.dtype.kind
    else:
        if isinstance(other, np.ndarray) and other.ndim == 0:
            other = other[()]
        if not isinstance(other, (bool, int, float, np.bool_, np.integer, np.floating)):
            return NotImplemented
        common = np.result_type(a.dtype, other)
        kinds = a.dtype.kind + ("b" if isinstance(other, (bool, np.bool_)) else "i" if isinstance(other, (int, np.integer)) else "f")
        scalar = other
    hi, lo, value = 0, 0, 0.0
    if all(k in "biu" for k in kinds):
        ctype = _CMP_INT                        # exact across signedness, as NumPy's mixed integer loops are
        if scalar is not None:
            v = int(scalar)
            if v < -2 ** 63:
                hi, lo = 0, 0                   # below every int64
            elif v > 2 ** 64 - 1:
                hi, lo = 2, 0                   # above every uint64
            else:
                hi, lo = int(v >= 0), v & (2 ** 64 - 1)
    else:
        ctype = _CMP_F64 if common == np.float64 else _CMP_F32
        if scalar is not None:
            value = float(common.type(scalar))  # the scalar in the common dtype, as NumPy converts it
    lhs = ascontiguousarray(a.astype(np.float32) if a.dtype == np.float16 else a)
    rhs = None
    if scalar is None:
        rhs = ascontiguousarray(other.astype(np.float32) if other.dtype == np.float16 else other)
    out = ndarray(a.shape, np.bool_)
    da, do = lhs._desc(), out._desc()
    db = rhs._desc() if rhs is not None else None
    _lib.check(_lib.load().mi_compare(op, ctypes.byref(da), ctypes.byref(db) if db is not None else None, ctype, value, hi, lo,
                                      ctypes.byref(do), None), ValueError)
    return out


def _is_wide_integer(value):
    """an integer value a double does not hold exactly"""
    if isinstance(value, np.ndarray):
        value = value[()] if value.ndim == 0 else None
    return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_)) and abs(int(value)) > 2 ** 53


def _copy(src, dst, round_half_even=False):
    dst._touch()
    if src._mem is dst._mem or not (isinstance(src._mem, _Memory) and isinstance(dst._mem, _Memory)):
        # possibly one allocation (views of one array, or foreign memory whose owner is unknown): NumPy assigns as if
        # from a copy, the kernels read while they write (`a[1:] = a[:-1]` would be a race)
        if src.ptr == dst.ptr and src.shape == dst.shape and src.strides == dst.strides and src.dtype == dst.dtype:
            return                                  # the same view: nothing to do
        if shares_memory(src, dst):
            src = src.copy()
    a, b = src._desc(), dst._desc()
    _lib.check(_lib.load().mi_copy(ctypes.byref(a), ctypes.byref(b), int(round_half_even), None))


# --------------------------------------------------------------------- creation
def empty(shape, dtype=np.float32):
    return ndarray(shape, dtype)


def zeros(shape, dtype=np.float32):
    a = ndarray(shape, dtype)
    if a.nbytes:
        _lib.check(_lib.load().mi_memset(a.ptr, 0, a.nbytes, None))
    return a


def full(shape, value, dtype=None):
    if dtype is None:
        dtype = np.asarray(value).dtype
    a = ndarray(shape, dtype)
    a.fill(value)
    return a


def ones(shape, dtype=np.float32):
    return full(shape, 1, dtype)


def empty_like(a, dtype=None):
    return ndarray(a.shape, a.dtype if dtype is None else dtype)


def zeros_like(a, dtype=None):
    return zeros(a.shape, a.dtype if dtype is None else dtype)


def asarray(obj, dtype=None):
    """Device array from a device array (no copy), a NumPy array / sequence
    (host to device copy) or anything exposing ``__cuda_array_interface__``
    (zero copy, e.g. a torch ROCm tensor)."""
    if isinstance(obj, ndarray):
        if dtype is not None and np.dtype(dtype) != obj.dtype:
            return obj.astype(dtype)
        return obj
    if not isinstance(obj, np.ndarray) and hasattr(obj, "__cuda_array_interface__"):
        return from_cuda_array_interface(obj)
    arr = np.asarray(obj, dtype=dtype)
    if arr.dtype.kind in "cOSU":
        raise TypeError("dtype {} is not supported by cupyimg_amd".format(arr.dtype))
    arr = np.ascontiguousarray(arr)
    out = ndarray(arr.shape, arr.dtype)
    out.set(arr)
    return out


array = asarray


EXPORT_SYNC = True      # see ndarray.__cuda_array_interface__


def default_stream_handle():
    """The library's default stream (a non-blocking hipStream_t) as an integer."""
    h = ctypes.c_void_p()
    _lib.check(_lib.load().mi_default_stream(ctypes.byref(h)))
    return int(h.value or 0)


def wait_for_stream(producer):
    """Work queued on the library's default stream from now on waits for what is
    queued on `producer` (a foreign stream handle as an integer, or 1 / 2 for the
    legacy / per-thread default stream)."""
    _lib.check(_lib.load().mi_stream_wait_stream(None, ctypes.c_void_p(int(producer))))


def stream_waits_for_us(consumer):
    """The foreign stream `consumer` (integer handle, or 1 / 2) waits for the work
    queued on the library's default stream so far -- call it before another
    runtime reads an array this library wrote in place (a torch tensor passed as
    `output=`); arrays exported through __cuda_array_interface__ carry the
    stream themselves."""
    _lib.check(_lib.load().mi_stream_wait_stream(ctypes.c_void_p(int(consumer)), None))


def from_cuda_array_interface(obj):
    """Zero-copy view of a foreign device array.  Stream ordering: when the
    producer names a stream (protocol version 3) the library's default stream
    waits for the work queued there.  Without one -- torch exports version 2,
    which has no `stream` entry -- it waits for the legacy default stream,
    which is where torch's default stream runs; a producer working on a
    non-blocking side stream has to name it or synchronise itself."""
    cai = obj.__cuda_array_interface__
    producer = cai.get("stream")
    if producer is not None and int(producer) == 0:
        raise ValueError("__cuda_array_interface__: stream 0 is not allowed by the protocol")
    wait_for_stream(1 if producer is None else int(producer))
    dtype = np.dtype(cai["typestr"])
    shape = tuple(cai["shape"])
    strides = cai.get("strides") or _c_strides(shape, dtype.itemsize)
    ptr = cai["data"][0]
    n = 1
    for s in shape:
        n *= s
    mem = _ForeignMemory(ptr, n * dtype.itemsize, obj)
    return ndarray(shape, dtype, _mem=mem, _ptr=ptr, _strides=strides)


def asnumpy(a):
    if isinstance(a, ndarray):
        return a.get()
    return np.asarray(a)


def ascontiguousarray(a, dtype=None):
    a = asarray(a)
    if dtype is not None and np.dtype(dtype) != a.dtype:
        return a.astype(dtype)
    return a if a._is_c_contiguous() else a.copy()


def with_host_hint(a, host):
    """Remember the host array a small device array was uploaded from (structuring elements: the morphology calls
    need them on the host again, and fetching one back costs a stream synchronisation plus a copy, ~50 us per call).
    Every write path of this package drops the hint -- `__setitem__`, `fill`, `set`, copies into the array, and its
    use as an `output=` (scipy.ndimage._support.get_output), also through a view (`ndarray._touch`); only the
    footprint constructors of skimage.morphology set it."""
    a._hc = np.array(host, copy=True)
    a._hc.setflags(write=False)
    return a


def host_copy(a):
    """NumPy copy of a device array: the remembered upload source if there is one, else a device-to-host copy."""
    hc = a._hc
    if hc is not None and hc.shape == a.shape and hc.dtype == a.dtype:
        return hc.copy()
    return a.get()


def _bounds(a):
    lo = hi = a.ptr
    for s, st in zip(a.shape, a.strides):
        if s == 0:
            return a.ptr, a.ptr
        if st >= 0:
            hi += (s - 1) * st
        else:
            lo += (s - 1) * st
    return lo, hi + a.dtype.itemsize


def shares_memory(a, b):
    """MAY_SHARE_BOUNDS test, as the reference uses it (_filters_core.py:148)."""
    if not isinstance(a, ndarray) or not isinstance(b, ndarray):
        return False
    if a.size == 0 or b.size == 0:
        return False
    alo, ahi = _bounds(a)
    blo, bhi = _bounds(b)
    return alo < bhi and blo < ahi


# --------------------------------------------------------------------- runtime
def synchronize():
    _lib.check(_lib.load().mi_stream_sync(None))


def device_count():
    n = ctypes.c_int(0)
    rc = _lib.load().mi_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def is_available():
    try:
        return device_count() > 0
    except Exception:
        return False


def set_device(dev):
    _lib.check(_lib.load().mi_set_device(int(dev)))


def get_device():
    d = ctypes.c_int()
    _lib.check(_lib.load().mi_get_device(ctypes.byref(d)))
    return d.value


def device_name(dev=None):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().mi_device_name(get_device() if dev is None else dev, buf, 256))
    return buf.value.decode()


def pool_stats():
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(_lib.load().mi_pool_stats(ctypes.byref(a), ctypes.byref(b)))
    return {"in_use": a.value, "cached": b.value}


def free_all_blocks():
    _lib.check(_lib.load().mi_pool_trim())


def arrays_differ(a, b):
    """True when two device arrays of equal dtype / shape differ anywhere
    (device-side comparison, one int32 read back).  The comparison is of bytes, not of values: NaNs with equal bits are
    equal, +0.0 and -0.0 differ."""
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("arrays_differ needs equal shapes and dtypes")
    a, b = ascontiguousarray(a), ascontiguousarray(b)
    flag = zeros((1,), np.int32)
    da, db = a._desc(), b._desc()
    _lib.check(_lib.load().mi_any_diff(ctypes.byref(da), ctypes.byref(db), ctypes.c_void_p(flag.ptr), None))
    return bool(flag.get()[0])


# --------------------------------------------------------------------- selection, gather, sorting (csrc/select.hip)
_SELECT_MAX = 2 ** 31 - 1


def _select_input(a):
    """C-contiguous device array within the family's limits (a strided view is compacted first, as the reductions do)"""
    a = asarray(a)
    if a.dtype == np.float16:
        raise TypeError("float16 arrays are storage only: convert with astype(float32) around this call")
    if a.size > _SELECT_MAX:
        raise ValueError("selection and sorting take at most 2**31 - 1 elements")
    return ascontiguousarray(a)


def _select_check(rc):
    try:
        _lib.check(rc, ValueError)
    except _lib.Unsupported as exc:
        raise ValueError(str(exc))


def _select_count(a):
    """(K, work): the count call of a compaction; `work` keeps the scanned per-tile counts for the write call"""
    lib = _lib.load()
    nbytes = ctypes.c_int64()
    _select_check(lib.mi_select_work_bytes(a.size, ctypes.byref(nbytes)))
    work = ndarray((nbytes.value,), np.uint8)
    total = ctypes.c_int64()
    ad, wd = a._desc(), work._desc()
    _select_check(lib.mi_select_count(ctypes.byref(ad), ctypes.byref(wd), ctypes.byref(total), None))
    return total.value, work


def _select_write(a, work, out, layout):
    ad, wd, od = a._desc(), work._desc(), out._desc()
    _select_check(_lib.load().mi_select_write(ctypes.byref(ad), ctypes.byref(wd), ctypes.byref(od), layout, None))
    return out


def count_nonzero(a):
    """Number of nonzero elements as a Python int (NaN counts, -0.0 does not): the count launch, the scan, one 8-byte read."""
    a = _select_input(a)
    return _select_count(a)[0] if a.size else 0


def flatnonzero(a):
    """Flat indices of the nonzero elements, int64, in raster order (numpy.flatnonzero)."""
    a = _select_input(a)
    if not a.size:
        return ndarray((0,), np.int64)
    k, work = _select_count(a)
    return _select_write(a, work, ndarray((k,), np.int64), 0)


def argwhere(a):
    """(K, ndim) int64 indices of the nonzero elements in raster order (numpy.argwhere), unravelled in the write kernel."""
    a = _select_input(a)
    if not a.size or not a.ndim:
        k = count_nonzero(a) if a.size else 0
        return ndarray((k, a.ndim), np.int64)
    k, work = _select_count(a)
    return _select_write(a, work, ndarray((k, a.ndim), np.int64), 1)


def nonzero(a):
    """Tuple of ndim int64 arrays, the indices of the nonzero elements along each axis (numpy.nonzero); the arrays are the
    rows of one (ndim, K) block."""
    a = _select_input(a)
    if not a.ndim:
        raise ValueError("nonzero of a 0-d array is not defined; use flatnonzero")
    if not a.size:
        return tuple(ndarray((0,), np.int64) for _ in range(a.ndim))
    k, work = _select_count(a)
    block = _select_write(a, work, ndarray((a.ndim, k), np.int64), 2)
    return tuple(block[d] for d in range(a.ndim))


def _take_rows(a, indices, inner):
    """out[k, :] = a.reshape(-1, inner)[indices[k], :]; IndexError when an index is out of range (checked on the device)"""
    a = _select_input(a)
    indices = ascontiguousarray(asarray(indices))
    if indices.dtype != np.int64:
        if indices.dtype.kind not in "iu":
            raise IndexError("indices must be integers")
        indices = indices.astype(np.int64)
    out = ndarray(tuple(indices.shape) + (inner,), a.dtype)
    if not indices.size:
        return out
    if not a.size:
        raise IndexError("cannot take from an empty array")
    flag = zeros((1,), np.int32)
    ad, idd, od = a._desc(), indices._desc(), out._desc()
    _select_check(_lib.load().mi_take(ctypes.byref(ad), ctypes.byref(idd), ctypes.byref(od), inner, ctypes.c_void_p(flag.ptr), None))
    if flag.get()[0]:
        raise IndexError("index out of range for an array of {} elements".format(a.size // inner))
    return out


def take(a, indices):
    """a.ravel()[indices] for an int64 device index array (numpy.take without an axis; negative indices count from the end).
    Whether every index is in range is checked on the device into a flag the host reads: an index out of range raises
    IndexError, and no out-of-bounds read is ever issued."""
    out = _take_rows(a, indices, 1)
    return out.reshape(out.shape[:-1])


def _argsort(a, descending, want_idx, want_sorted):
    a = _select_input(a)
    if a.ndim != 1:
        raise ValueError("argsort and sort take 1-D arrays")
    idx = ndarray(a.shape, np.int64) if want_idx else None
    srt = ndarray(a.shape, a.dtype) if want_sorted else None
    if a.size:
        ad = a._desc()
        idd = idx._desc() if want_idx else None
        sd = srt._desc() if want_sorted else None
        _select_check(_lib.load().mi_argsort(ctypes.byref(ad), ctypes.byref(idd) if want_idx else None,
                                             ctypes.byref(sd) if want_sorted else None, int(bool(descending)), None))
    return idx, srt


def argsort(a, descending=False):
    """Stable argsort of a 1-D array, int64: numpy.argsort(a, kind="stable") index for index; with `descending`
    numpy.argsort(-a, kind="stable") (integers negate with wrap-around, as NumPy's do; bool negates logically).  -0.0 sorts
    equal to +0.0; every NaN sorts last, the NaNs in their original order.  The input is not written."""
    return _argsort(a, descending, True, False)[0]


def sort(a):
    """Sorted copy of a 1-D array: a[argsort(a)] (numpy.sort(a, kind="stable"))."""
    return _argsort(a, False, False, True)[1]


def unique(a, return_index=False, return_inverse=False, return_counts=False):
    """numpy.unique of an integer or bool array of any shape, flattened: the sorted distinct values, and on request the
    index of each value's first occurrence, the inverse (of the input's shape, as NumPy 2 gives it) and the counts, all
    intp.  A stable sort, head flags where a sorted key differs from its predecessor (csrc/segment.hip), then the count /
    scan / scatter compaction of csrc/select.hip over the flags.  Float arrays raise TypeError: NumPy does not define
    which of -0.0 / +0.0 represents the pair."""
    if not isinstance(a, ndarray):
        a = asarray(a) if hasattr(a, "__cuda_array_interface__") else np.asarray(a)
    if a.dtype.kind not in "iub":
        raise TypeError("unique takes integer and bool arrays, not {}".format(a.dtype))
    a = asarray(a)
    flat = _select_input(a).reshape(-1)
    n = flat.size
    lib = _lib.load()
    if n == 0:
        values = ndarray((0,), a.dtype)
        index = counts = pos = perm = None
    else:
        perm, srt = _argsort(flat, False, True, True)
        heads = ndarray((n,), np.bool_)
        sd, hd = srt._desc(), heads._desc()
        _select_check(lib.mi_unique_heads(ctypes.byref(sd), ctypes.byref(hd), None))
        k, work = _select_count(heads)
        pos = _select_write(heads, work, ndarray((k,), np.int64), 0)
        values = take(srt, pos)
    out = [values]
    if return_index:
        out.append(ndarray((0,), np.int64) if n == 0 else take(perm, pos))
    if return_inverse:
        inverse = ndarray(a.shape, np.int64)
        if n:
            flat_inv = inverse.reshape(-1)
            pd, qd, fd = pos._desc(), perm._desc(), flat_inv._desc()
            _select_check(lib.mi_unique_inverse(ctypes.byref(pd), ctypes.byref(qd), ctypes.byref(fd), None))
        out.append(inverse)
    if return_counts:
        counts = ndarray(values.shape, np.int64)
        if n:
            pd, cd = pos._desc(), counts._desc()
            _select_check(lib.mi_unique_counts(ctypes.byref(pd), n, ctypes.byref(cd), None))
        out.append(counts)
    return out[0] if len(out) == 1 else tuple(out)


class Stream:
    """A hipStream besides the library's default stream (used for the halo
    exchange so that it overlaps the interior filtering)."""

    def __init__(self):
        self._s = ctypes.c_void_p()
        _lib.check(_lib.load().mi_stream_create(ctypes.byref(self._s)))

    @property
    def handle(self):
        return self._s

    def wait_event(self, event):
        """Work submitted to this stream from now on waits for `event`."""
        _lib.check(_lib.load().mi_stream_wait_event(self._s, event._e))

    def synchronize(self):
        _lib.check(_lib.load().mi_stream_sync(self._s))

    def __del__(self):
        try:
            if self._s:
                _lib.load().mi_stream_destroy(self._s)
        except Exception:
            pass


def default_stream_wait_event(event):
    """Work submitted to the default stream from now on waits for `event`."""
    _lib.check(_lib.load().mi_stream_wait_event(None, event._e))


class Event:
    """hipEvent; recorded on the library's default stream unless a Stream is given."""

    def __init__(self):
        self._e = ctypes.c_void_p()
        _lib.check(_lib.load().mi_event_create(ctypes.byref(self._e)))

    def record(self, stream=None):
        _lib.check(_lib.load().mi_event_record(self._e, None if stream is None else stream.handle))

    def synchronize(self):
        _lib.check(_lib.load().mi_event_sync(self._e))

    def elapsed_ms(self, later):
        ms = ctypes.c_float()
        _lib.check(_lib.load().mi_event_elapsed_ms(self._e, later._e, ctypes.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if self._e:
                _lib.load().mi_event_destroy(self._e)
        except Exception:
            pass
