"""skimage.registration subset: dense optical flow by the TV-L1 algorithm (cupyimg/skimage/registration/_optical_flow.py:20-254,
_optical_flow_utils.py:37-156) with the solver's fixed-point iteration as two fused HIP launches (csrc/tvl1.hip)."""
import ctypes
from functools import partial

import numpy as np

from ... import core
from ...scipy import ndimage as ndi
from ...scipy.ndimage import _support as S
from ..filters import _img_as_float
from ..transform import pyramid_reduce

__all__ = ["optical_flow_tvl1"]

_WORK_BYTES = 16384                 # MI_TVL1_WORK_BYTES
_MAX_NDIM = 4                       # what the per-voxel kernels of csrc/tvl1.hip are built for
_stats = []


def last_tvl1_stats():
    """One dict per pyramid level of the most recent `optical_flow_tvl1` call of this process, coarsest level first (after
    a direct `_tvl1` call: one more entry at the end): "shape", "warps" (warps run, the one that met the stopping rule
    included), "iterations" (fixed-point iterations run) and "launches" (kernel launches queued inside the fixed-point
    loops: the data term and the regularisation, nothing else).  A diagnostic for benchmarks and tests."""
    return [dict(s) for s in _stats]


def _convert(image, dtype):
    """The reference's `_convert(image, dtype)` for a float target (util/dtype.py:201-379): floats are cast, bool becomes
    {0, 1}, unsigned integers are multiplied by 1 / max and signed ones become (x + 0.5) * (2 / (max - min)), both in the
    first of (dtype, float32, float64) that is at least as wide as the integer.  Where that type is float64 the unsigned
    rule is `img_as_float`'s arithmetic and is taken from there."""
    dtype = np.dtype(dtype)
    din = image.dtype
    if din == dtype:
        return image
    if din.kind in "fb":
        return image.astype(dtype)
    if din.kind not in "ui":
        raise ValueError("Can not convert from {} to {}.".format(din, dtype))
    comp = dtype if dtype.itemsize >= din.itemsize else np.dtype(np.float64)
    info = np.iinfo(din)
    if din.kind == "u" and comp == np.float64:
        out = _img_as_float(image)
    elif din.kind == "u":
        # one rounding: the product of two float32 values is exact in the double the kernel works in
        out = S.scale_shift(image.astype(comp), float(comp.type(1.0 / info.max)), 0.0)
    else:
        out = S.scale_shift(image.astype(comp), 1.0, 0.5)
        out = S.scale_shift(out, float(comp.type(2 / (int(info.max) - int(info.min)))), 0.0)
    return out.astype(dtype, copy=False)


def resize_flow(flow, shape):
    """The vector field resized to `shape` by nearest-neighbour zoom, its values scaled to the new resolution
    (_optical_flow_utils.py:37-67)."""
    scale = [n / o for n, o in zip(shape, flow.shape[1:])]
    zoomed = ndi.zoom(flow, [1] + scale, order=0, mode="nearest", prefilter=False)
    rflow = core.empty(zoomed.shape, zoomed.dtype)
    for c, s in enumerate(scale):
        rflow[c] = S.scale_shift(zoomed[c], float(flow.dtype.type(s)), 0.0)
    return rflow


def get_pyramid(I, downscale=2.0, nlevel=10, min_size=16):
    """The image pyramid, coarsest level first (_optical_flow_utils.py:70-101)."""
    pyramid = [I]
    size = min(I.shape)
    count = 1
    while (count < nlevel) and (size > downscale * min_size):
        J = pyramid_reduce(pyramid[-1], downscale, multichannel=False)
        pyramid.append(J)
        size = min(J.shape)
        count += 1
    return pyramid[::-1]


def coarse_to_fine(I0, I1, solver, downscale=2, nlevel=10, min_size=16, dtype=np.float32):
    """Run `solver(reference, moving, flow0)` on every level of the pyramids of two device arrays, coarsest first, each
    level starting from the resized flow of the one before (_optical_flow_utils.py:104-156)."""
    if I0.shape != I1.shape:
        raise ValueError("Input images should have the same shape")
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("Only the floating point data types float32 and float64 are valid for optical flow")
    dtype = np.dtype(dtype)
    pyramid = list(zip(get_pyramid(_convert(I0, dtype), downscale, nlevel, min_size),
                       get_pyramid(_convert(I1, dtype), downscale, nlevel, min_size)))
    flow = core.zeros((pyramid[0][0].ndim,) + tuple(pyramid[0][0].shape), dtype)
    flow = solver(pyramid[0][0], pyramid[0][1], flow)
    for J0, J1 in pyramid[1:]:
        flow = solver(J0, J1, resize_flow(flow, J0.shape))
    return flow


def _scratch(lib, flow):
    """the block the per-voxel route of mi_tvl1_reg needs for this flow field (None on the fused route)"""
    need = ctypes.c_int64(0)
    S.check(lib.mi_tvl1_scratch_size(ctypes.byref(flow._desc()), ctypes.byref(need)), ValueError)
    return core.empty((need.value,), flow.dtype) if need.value else None


def _fixed_point(lib, gdesc, ndesc, r0desc, aux, out, pin_desc, pout_desc, scratch, f0, dt, f1):
    """One fixed-point iteration: the data term in place on `aux`, the regularisation from (aux, proj_in) into (out,
    proj_out).  Returns the number of launches queued."""
    n = ctypes.c_int(0)
    adesc = aux._desc()
    S.check(lib.mi_tvl1_data(ctypes.byref(gdesc), ctypes.byref(ndesc), ctypes.byref(r0desc), ctypes.byref(adesc), float(f0), None))
    S.check(lib.mi_tvl1_reg(ctypes.byref(adesc), ctypes.byref(pin_desc), ctypes.byref(out._desc()), ctypes.byref(pout_desc),
                            ctypes.c_void_p(scratch.ptr) if scratch is not None else None, float(dt), float(f1), ctypes.byref(n), None))
    return 1 + n.value


def _prepare(warped, reference, flow):
    """grad, NI and rho_0 of one warp (mi_tvl1_prepare) from C-contiguous device arrays of one float dtype."""
    lib = S.lib()
    grad = core.empty(flow.shape, flow.dtype)
    NI = core.empty(warped.shape, warped.dtype)
    rho_0 = core.empty(warped.shape, warped.dtype)
    S.check(lib.mi_tvl1_prepare(ctypes.byref(warped._desc()), ctypes.byref(reference._desc()), ctypes.byref(flow._desc()),
                                ctypes.byref(grad._desc()), ctypes.byref(NI._desc()), ctypes.byref(rho_0._desc()), None), ValueError)
    return grad, NI, rho_0


def _iterate(rho_0, grad, NI, flow, proj, n, attachment=15, tightness=0.3):
    """`n` fixed-point iterations from (flow, proj), which stay untouched -> (flow, proj, launches): the loop body of `_tvl1`
    on its own, for tests and benchmarks."""
    lib = S.lib()
    nd = rho_0.ndim
    dt = 0.5 / nd
    f0, f1 = attachment * tightness, dt / tightness
    flows = [flow.copy(), core.empty(flow.shape, flow.dtype)]
    projs = [proj.copy(), core.empty(proj.shape, proj.dtype)]
    scratch = _scratch(lib, flow)
    gdesc, ndesc, r0desc = grad._desc(), NI._desc(), rho_0._desc()
    launches = 0
    for i in range(n):
        launches += _fixed_point(lib, gdesc, ndesc, r0desc, flows[i & 1], flows[(i + 1) & 1], projs[i & 1]._desc(),
                                 projs[(i + 1) & 1]._desc(), scratch, f0, dt, f1)
    return flows[n & 1], projs[n & 1], launches


def _tvl1(reference_image, moving_image, flow0, attachment, tightness, num_warp, num_iter, tol, prefilter):
    """The TV-L1 solver on one pyramid level (_optical_flow.py:20-158).  reference_image, moving_image: device arrays of one
    shape and dtype (float32 / float64), flow0: (ndim, *shape) of that dtype; like the reference's, the first data step
    works in place on `flow0`.  Returns the flow, a C-contiguous device array."""
    ref = core.ascontiguousarray(reference_image)
    mov = core.ascontiguousarray(moving_image)
    dtype = ref.dtype
    nd = ref.ndim
    shape = tuple(ref.shape)
    lib = S.lib()
    dt = 0.5 / nd
    f0 = attachment * tightness
    f1 = dt / tightness
    tol = tol * ref.size

    flow_current = flow_previous = core.ascontiguousarray(flow0)
    fshape = (nd,) + shape
    proj = [core.zeros((nd, nd) + shape, dtype), core.empty((nd, nd) + shape, dtype)]
    coords = core.empty(fshape, dtype)
    grad = core.empty(fshape, dtype)
    NI = core.empty(shape, dtype)
    rho_0 = core.empty(shape, dtype)
    work = core.empty((_WORK_BYTES,), np.uint8)
    scratch = _scratch(lib, flow_current)
    spare = []
    lo, hi = S.min_max(mov)                     # what `warp` clips to
    rdesc, pdesc = ref._desc(), [proj[0]._desc(), proj[1]._desc()]
    gdesc, ndesc, r0desc, cdesc = grad._desc(), NI._desc(), rho_0._desc(), coords._desc()
    stats = {"shape": shape, "warps": 0, "iterations": 0, "launches": 0}
    _stats.append(stats)
    pi = 0

    for w in range(num_warp):
        if prefilter:
            # a new array, as in the reference: flow_previous stays the flow from before the median
            filtered = spare.pop() if spare else core.empty(fshape, dtype)
            for c in range(nd):
                filtered[c] = ndi.median_filter(flow_current[c], size=3)
            flow_current = filtered

        fdesc = flow_current._desc()
        S.check(lib.mi_tvl1_coords(ctypes.byref(fdesc), ctypes.byref(cdesc), None))
        warped = S.clip(ndi.map_coordinates(mov, coords, order=1, mode="nearest"), lo, hi)
        S.check(lib.mi_tvl1_prepare(ctypes.byref(warped._desc()), ctypes.byref(rdesc), ctypes.byref(fdesc), ctypes.byref(gdesc),
                                    ctypes.byref(ndesc), ctypes.byref(r0desc), None))

        for _ in range(num_iter):
            # the data term in place: flow_current becomes the reference's flow_auxiliary (an alias, not a copy), and the
            # regularisation writes a new flow_current
            aux = flow_current
            out = spare.pop() if spare else core.empty(fshape, dtype)
            launches = _fixed_point(lib, gdesc, ndesc, r0desc, aux, out, pdesc[pi], pdesc[pi ^ 1], scratch, f0, dt, f1)
            pi ^= 1
            stats["iterations"] += 1
            stats["launches"] += launches
            if aux is not flow_previous and aux is not flow0:
                spare.append(aux)
            flow_current = out
        stats["warps"] += 1

        if w == num_warp - 1:
            break                                    # the reference forms the sum once more; nothing depends on it
        S.check(lib.mi_tvl1_diff_sum(ctypes.byref(flow_previous._desc()), ctypes.byref(flow_current._desc()),
                                     ctypes.c_void_p(work.ptr), None))
        if float(work[:8].get().view(np.float64)[0]) < tol:
            break
        if flow_previous is not flow0:
            spare.append(flow_previous)
        flow_previous = flow_current

    return flow_current


def optical_flow_tvl1(reference_image, moving_image, *, attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4,
                      prefilter=False, dtype=np.float32):
    """Coarse-to-fine TV-L1 optical flow (Zach, Pock and Bischof 2007; _optical_flow.py:161-254): the field `flow` of shape
    (ndim, *image.shape) and dtype `dtype` for which reference_image(q) ~ moving_image(q + flow(q)).

    attachment: the smaller, the smoother the result; tightness: small, to keep the attachment and regularisation parts in
    correspondence; num_warp: how many times the moving image is warped per pyramid level; num_iter: fixed-point iterations
    per warp; tol: a warp ends the level when sum (flow_previous - flow)^2 < tol * image.size; prefilter: a 3^ndim median
    of every flow component before each warp.  Grey-scale images of rank 2 to 4; integer images are scaled as the
    reference's `_convert` scales them; host arrays are uploaded; the inputs are never modified.

    Per pyramid level (halving until the smallest extent is at most 32) the solver warps with the order-1
    `map_coordinates` (mode "nearest", clipped to the moving image's range), forms gradient, NI and rho_0 in one launch,
    and runs every fixed-point iteration as two launches: the pointwise data term, and a kernel that keeps one flow
    component of a tile in LDS through both regularisation steps (ranks 2 and 3; rank 4: four launches with one thread
    per voxel).  The host reads one double per warp, never inside the `num_iter` loop.  All arithmetic is the
    reference's, in `dtype`, operation by operation, so a call gives the bits a NumPy transcription gives with this
    library's interpolation and filters plugged in.

    As in the reference, `flow_previous` is the same array as the one the first data step of a warp updates in place, so
    the stopping rule compares the final flow of a warp with the flow as it stood after the first data step of that
    warp; with `prefilter` the median makes a new array and `flow_previous` is the flow from before the median.  Both
    behaviours are reproduced.

    Deviations, all of which raise: `dtype` must be float32 or float64 (the reference also admits float16 and
    longdouble) -- ValueError; images of rank 1 or above 4, or with an axis shorter than 2 -- ValueError; `num_warp` or
    `num_iter` below 1 -- ValueError (the reference returns the initial flow); complex input -- TypeError; mismatched
    shapes -- ValueError as in the reference.  One deviation does not raise: the stopping sum is taken in double in a
    fixed order (the reference: in `dtype`, in its reduction's order), so a warp can stop differently only where the sum
    is within summation error of tol * size.

    Besides the two converted images and their pyramids a level holds 2 * ndim^2 + 5 * ndim + 4 arrays of the level's
    size: three flow buffers, two copies of proj, the gradient and the coordinates, and NI, rho_0, the warped image and
    its clipped copy (37 with ndim = 3; `prefilter` adds one median result at a time; the rank-4 route adds ndim^2 + ndim
    arrays of scratch)."""
    images = []
    for im in (reference_image, moving_image):
        if not isinstance(im, core.ndarray):
            host = np.asarray(im)
            if host.dtype.kind == "c":
                raise TypeError("Complex type not supported")
            im = core.asarray(host)
        images.append(im)
    ref, mov = images
    if ref.shape != mov.shape:
        raise ValueError("Input images should have the same shape")
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("Only the floating point data types float32 and float64 are valid for optical flow")
    if ref.ndim < 2 or ref.ndim > _MAX_NDIM:
        raise ValueError("optical_flow_tvl1 takes images of rank 2 to {}".format(_MAX_NDIM))
    if min(ref.shape) < 2:
        raise ValueError("optical_flow_tvl1 needs at least 2 samples along every axis")
    if int(num_warp) < 1 or int(num_iter) < 1:
        raise ValueError("num_warp and num_iter must be at least 1")
    del _stats[:]
    solver = partial(_tvl1, attachment=attachment, tightness=tightness, num_warp=int(num_warp), num_iter=int(num_iter), tol=tol,
                     prefilter=prefilter)
    return coarse_to_fine(ref, mov, solver, dtype=dtype)
