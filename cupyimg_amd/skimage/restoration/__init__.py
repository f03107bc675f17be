"""skimage.restoration subset: total-variation denoising by Chambolle's projection algorithm
(cupyimg/skimage/restoration/_denoise.py:6-175) as fused HIP kernels (csrc/tv_chambolle.hip)."""
import ctypes

import numpy as np

from ... import core, _lib
from ...scipy.ndimage import _support as S
from ..filters import _img_as_float
from ._deconvolution import richardson_lucy

__all__ = ["denoise_tv_chambolle", "richardson_lucy"]

# Iterations queued between two reads of the state block.  A read costs one stream synchronisation and a 64-byte copy (tens
# of microseconds); an iteration queued after the stop costs two launches that return at once (a few microseconds each).
# With 16 a run of the usual 30 .. 50 iterations synchronises two to four times and queues at most 15 idle iterations,
# which is less than one synchronisation; on large volumes, where an iteration takes longer than a synchronisation,
# neither matters.
_TV_BATCH = 16
_STATE_BYTES = 64                                   # MI_TV_STATE_BYTES
_WORK_BYTES = _STATE_BYTES + 16 * 65536             # MI_TV_WORK_BYTES
_tv_iterations = None


def last_tv_iterations():
    """The value of the reference's loop variable `i` (_denoise.py:40-86) when the loop of the most recent
    `denoise_tv_chambolle` call of this process ended: the iteration at which the stopping rule held, or `n_iter_max` when
    the loop ran out.  A list with one value per channel after a multichannel call; None before the first call.  A
    diagnostic for benchmarks and tests."""
    return _tv_iterations


def _tv_nd(image, weight, eps, n_iter_max):
    """image: C-contiguous float32 / float64 device array of at least one element -> (denoised array, i at exit)"""
    ndim = image.ndim
    lib = S.lib()
    p = [core.zeros((ndim, image.size), image.dtype), core.empty((ndim, image.size), image.dtype)]
    work = core.empty((_WORK_BYTES,), np.uint8)
    state = work[:_STATE_BYTES]
    S.check(lib.mi_memset(work.ptr, 0, _STATE_BYTES, None))
    idesc = image._desc()
    pdesc = [p[0]._desc(), p[1]._desc()]
    queued = 0
    stop = None
    while queued < n_iter_max and stop is None:
        for i in range(queued, min(n_iter_max, queued + _TV_BATCH)):
            S.check(lib.mi_tv_chambolle_step(ctypes.byref(idesc), ctypes.byref(pdesc[i & 1]), ctypes.byref(pdesc[(i + 1) & 1]),
                                             float(weight), float(eps), i, ctypes.c_void_p(work.ptr), None))
            queued += 1
        words = state.get().view(np.int32)
        if words[0]:
            stop = int(words[1])
    last = n_iter_max - 1 if stop is None else stop          # `out` is the one computed at the start of this iteration
    out = core.empty(image.shape, image.dtype)
    odesc = out._desc()
    S.check(lib.mi_tv_chambolle_output(ctypes.byref(idesc), ctypes.byref(pdesc[last & 1]), ctypes.byref(odesc), None))
    return out, (n_iter_max if stop is None else stop)


def denoise_tv_chambolle(image, weight=0.1, eps=2.0e-4, n_iter_max=200, multichannel=False):
    """Total-variation denoising of an n-dimensional image by Chambolle's projection algorithm (_denoise.py:90-175).

    The greater `weight`, the more denoising.  The loop stops at the first iteration i >= 1 at which the energy
    E = (sum d^2 + weight * sum |grad out|) / size changed by less than `eps * E_0`, or after `n_iter_max` iterations;
    the result is `out = image + d` as it stood at the start of that iteration.  With `multichannel` every
    `image[..., c]` is denoised on its own.

    One iteration is one launch of a fused kernel (2-D and 3-D arrays; other ranks: one thread per voxel) that reads the
    image and the dual field once and writes the dual field once, plus a one-workgroup launch that applies the stopping
    rule on the device; the host reads 64 bytes every 16 iterations.  All arithmetic is the reference's, in the image's
    dtype, operation by operation, so a fixed number of iterations gives the bits a NumPy transcription gives.  Two
    deviations: the two sums of E are accumulated in double in a fixed order (the reference: in the image dtype, in its
    reduction's order), so the iteration at which the loop stops can differ where |E_(i-1) - E_i| / (eps * E_0) is
    within summation error of 1; float16 images are computed in float32 and returned as float16.  float32 and float64
    keep their dtype, every other dtype goes through img_as_float to float64.  `n_iter_max` < 1 raises ValueError (the
    reference: an unbound name).

    Always a new array, never a view of `image`.  Besides the input a call holds 2 * ndim + 1 volumes of the image dtype
    (two copies of the dual field and the result), all from the pool, plus 1 MiB of partial sums; a non-contiguous
    or converted input adds its contiguous copy."""
    global _tv_iterations
    if not isinstance(image, core.ndarray):
        host = np.asarray(image)
        if host.dtype.kind == "c":
            raise TypeError("Complex type not supported")
        image = core.asarray(host)
    if n_iter_max < 1:
        raise ValueError("n_iter_max must be at least 1")
    dtype = image.dtype
    result_dtype = dtype if dtype.kind == "f" else np.dtype(np.float64)
    nd = image.ndim - 1 if multichannel else image.ndim
    if nd < 1 or nd > _lib.MI_MAX_NDIM:
        raise ValueError("denoise_tv_chambolle takes arrays of rank 1 to {}".format(_lib.MI_MAX_NDIM))
    if image.size == 0:
        _tv_iterations = [0] * image.shape[-1] if multichannel else 0
        return core.empty(image.shape, result_dtype)
    if dtype == np.float16:
        work = image.astype(np.float32)
    elif dtype.kind == "f":
        work = image
    else:
        work = _img_as_float(image)
    n_iter_max = int(n_iter_max)
    if multichannel:
        out = core.empty(work.shape, work.dtype)
        its = []
        for c in range(work.shape[-1]):
            res, i = _tv_nd(work[..., c].copy(), weight, eps, n_iter_max)
            out[..., c] = res
            its.append(i)
        _tv_iterations = its
    else:
        out, _tv_iterations = _tv_nd(core.ascontiguousarray(work), weight, eps, n_iter_max)
    return out.astype(result_dtype, copy=False)
