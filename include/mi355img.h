/*
 * mi355img.h -- C-ABI of libmi355img.so, the MI355X (gfx950) n-D image
 * filtering engine behind cupyimg_amd.
 *
 * The reference (mritools/cupyimg) has no FFI: its seam is Python-level.  Every
 * hot-path API function funnels into one of three launch sites, and each entry
 * point below replaces exactly one of them (reference file:line in the
 * comment above each declaration):
 *
 *   _filters_core._call_kernel(kernel, input, weights, output, structure)
 *       cupyimg/scipy/ndimage/_filters_core.py:112-156   (K1, K2 kernels)
 *   erode_kernel(input, structure[, mask], output)
 *       cupyimg/scipy/ndimage/morphology.py:292-322      (K4)
 *   kern(filtered, coordinates | matrix, output)
 *       cupyimg/scipy/ndimage/interpolation.py:393,545,560 (K5)
 *
 * plus the part of CuPy the reference leans on for memory/streams (L0 in
 * SURVEY.md), which this library owns itself: no CuPy, no PyTorch.
 *
 * Conventions
 *   - plain C linkage, POD arguments only; every function returns int:
 *       0 = ok, < 0 = MI_ERR_*, > 0 = hipError_t of the failing HIP call.
 *     mi_last_error() returns a thread-local human-readable message.
 *   - device arrays are described by mi_array (pointer + dtype + shape +
 *     byte strides).  Compute entry points require C-contiguous arrays
 *     (MI_ERR_NOT_CONTIGUOUS otherwise); mi_copy handles arbitrary strides
 *     and dtype conversion.
 *   - the caller owns all buffers; the library owns only its scratch pool,
 *     streams/events it created and RCCL communicators.
 *   - small host-side parameter arrays (weights, footprints, matrices) are
 *     copied during the call; they may be freed as soon as it returns.
 *   - all work is enqueued on `stream` (NULL = the library's per-device
 *     default stream) and is asynchronous with respect to the host.
 *   - thread-safe: no unsynchronised global state (the reference's tests call
 *     filters from 4 threads, tests/test_filters.py:354-412).
 */
#ifndef MI355IMG_H
#define MI355IMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_MAX_NDIM 8
#define MI_VERSION 100 /* 0.1.0 */

typedef enum mi_dtype {
    MI_BOOL = 0, MI_I8 = 1, MI_U8 = 2, MI_I16 = 3, MI_U16 = 4, MI_I32 = 5,
    MI_U32 = 6, MI_I64 = 7, MI_U64 = 8, MI_F32 = 9, MI_F64 = 10,
    MI_F16 = 11   /* storage only: mi_copy converts to / from it (the reference keeps float16 results in float16,
                     _filters_core.py:169-171, computing in float32 / float64); every compute entry point answers
                     MI_ERR_INVALID_ARG for it and the Python layer converts around the call */
} mi_dtype;

/* scipy.ndimage boundary modes (cupyimg/scipy/ndimage/_util.py:105-119).
 * For filters WRAP == GRID_WRAP and GRID_CONSTANT == CONSTANT
 * (_filters_core.py:224-225); interpolation distinguishes them. */
typedef enum mi_mode {
    MI_MODE_REFLECT = 0,      /* also 'grid-mirror' */
    MI_MODE_CONSTANT = 1,
    MI_MODE_NEAREST = 2,
    MI_MODE_MIRROR = 3,
    MI_MODE_WRAP = 4,
    MI_MODE_GRID_WRAP = 5,
    MI_MODE_GRID_CONSTANT = 6
} mi_mode;

enum {
    MI_OK = 0,
    MI_ERR_INVALID_ARG = -1,
    MI_ERR_UNSUPPORTED = -2,   /* valid request, no kernel for it (host falls back) */
    MI_ERR_NOMEM = -3,
    MI_ERR_NOT_CONTIGUOUS = -4,
    MI_ERR_RCCL = -5,
    MI_ERR_INTERNAL = -6
};

typedef struct mi_array {
    void *data;                    /* device pointer */
    int32_t dtype;                 /* mi_dtype */
    int32_t ndim;                  /* 0..MI_MAX_NDIM */
    int64_t shape[MI_MAX_NDIM];
    int64_t strides[MI_MAX_NDIM];  /* bytes */
} mi_array;

typedef void *mi_stream; /* hipStream_t */
typedef void *mi_event;  /* hipEvent_t  */
typedef void *mi_comm;   /* ncclComm_t  */

/* ------------------------------------------------------------------ */
/* runtime: replaces the CuPy runtime the reference imports             */
/* (cupyimg/__init__.py:23-28; cupy.zeros at _util.py:80)               */
/* ------------------------------------------------------------------ */
int mi_version(void);
const char *mi_last_error(void);
int mi_device_count(int *count);
int mi_set_device(int device);
int mi_get_device(int *device);
int mi_device_name(int device, char *buf, size_t buflen);
int mi_device_attr(int device, int *cu_count, int *clock_khz, size_t *total_mem);
int mi_mem_info(size_t *free_bytes, size_t *total_bytes);

/* pooled device memory (size-bucketed free lists, mutex guarded) */
int mi_malloc(void **ptr, size_t nbytes);
int mi_free(void *ptr);
int mi_pool_trim(void);
int mi_pool_stats(size_t *bytes_in_use, size_t *bytes_cached);

int mi_memcpy_h2d(void *dst, const void *src, size_t nbytes, mi_stream stream);
int mi_memcpy_d2h(void *dst, const void *src, size_t nbytes, mi_stream stream); /* syncs */
int mi_memcpy_d2d(void *dst, const void *src, size_t nbytes, mi_stream stream);
int mi_memcpy_peer(void *dst, int dst_dev, const void *src, int src_dev, size_t nbytes,
                   mi_stream stream);
int mi_memset(void *dst, int value, size_t nbytes, mi_stream stream);

int mi_stream_create(mi_stream *stream);
int mi_stream_destroy(mi_stream stream);
int mi_stream_sync(mi_stream stream);
int mi_default_stream(mi_stream *stream);
int mi_device_sync(void);
int mi_event_create(mi_event *event);
int mi_event_destroy(mi_event event);
int mi_event_record(mi_event event, mi_stream stream);
int mi_stream_wait_event(mi_stream stream, mi_event event); /* later work on stream waits for event */
/* Later work on `waiter` waits for everything queued on `producer` so far.  Either
 * argument: a hipStream_t (also one owned by another runtime: torch, CuPy), NULL = the
 * library's default stream, or the __cuda_array_interface__ stream codes 1 (legacy
 * default stream) / 2 (per-thread default stream).  This is how zero-copy imports and
 * exports are ordered against the other runtime's stream: the library's default stream
 * is non-blocking, it never synchronises with the null stream by itself. */
int mi_stream_wait_stream(mi_stream waiter, mi_stream producer);
int mi_event_sync(mi_event event);
int mi_event_elapsed_ms(mi_event start, mi_event stop, float *ms);

/* ------------------------------------------------------------------ */
/* array plumbing: `output[...] = input` and dtype casts               */
/* (_filters_core.py:94,107,154; cast<> at :166-187)                    */
/* ------------------------------------------------------------------ */
/* dst[...] = (dst dtype) src, arbitrary strides, same shape.  Float ->
 * integer conversion truncates toward zero; negative -> unsigned wraps.
 * round_half_even != 0 applies rint() first (interpolation integer outputs,
 * _interp_kernels.py:580-583). */
int mi_copy(const mi_array *src, const mi_array *dst, int round_half_even, mi_stream stream);
int mi_fill(const mi_array *dst, double value, mi_stream stream);
/* r4b: rows that are not a multiple of 16 bytes (181 x 217 x 181 ...): out[..., x] = in[..., map(x - left)] for
 * x in [0, out.shape[-1]) -- every row extended along the last axis by a filter boundary mode (MI_MODE_CONSTANT: cval) --
 * and its inverse out[..., x] = in[..., left + x].  1-, 2-, 4- and 8-byte dtypes (r5: 8), C-contiguous; the extended rows and `left`
 * are multiples of 16 bytes and the extended array is 16-byte aligned (what the fused kernels need: the Python layer runs
 * them on the extended volume and copies the columns back; the reference has no counterpart -- its kernels index
 * element by element, _filters_core.py:190-348). */
int mi_extend_rows(const mi_array *in, const mi_array *out, int left, int mode, double cval, mi_stream stream);
int mi_crop_rows(const mi_array *in, const mi_array *out, int left, mi_stream stream);
/* *flag_dev (device int32) |= any(a != b); a, b contiguous, same dtype/shape */
int mi_any_diff(const mi_array *a, const mi_array *b, int32_t *flag_dev, mi_stream stream);
/* out = a (op) b, elementwise, one dtype, C-contiguous; op: 0 add, 1 subtract,
 * 2 multiply, 3 sqrt(a) (b may be NULL).  Integers wrap like NumPy's same-dtype
 * ufuncs.  Used by the composite filters built on the path (generic_laplace
 * `output += tmp` filters.py:1005-1011, generic_gradient_magnitude :1134-1147,
 * top-hats / morphological gradient morphology.py:887-1226). */
int mi_elementwise(int op, const mi_array *a, const mi_array *b, const mi_array *out, mi_stream stream);
/* float32 / float64: op 0: out = a * p0 + p1; op 1: out = clip(a, p0, p1), entries equal
 * to `keep` left alone when keep_flag != 0 (skimage warp's output clipping,
 * skimage/transform/_warps.py:745-787; dtype range scaling of img_as_float).  op 0 also
 * takes an 8- / 16-bit integer or bool input with a float32 / float64 output: conversion
 * and scaling in one pass. */
int mi_scalar_op(int op, const mi_array *a, const mi_array *out, double p0, double p1, double keep,
                 int keep_flag, mi_stream stream);
/* minimum and maximum of a contiguous array (synchronises the stream) */
int mi_min_max(const mi_array *a, double *lo, double *hi, mi_stream stream);
/* Reductions in double over an arbitrarily strided array (synchronises the stream): op 0 sum(a),
 * op 1 sum((a - b)^2), op 2 sum(a^2).  Serves the cropped mean of the SSIM map
 * (skimage/metrics/_structural_similarity.py:229-233) and skimage/metrics/simple_metrics.py. */
int mi_sum(int op, const mi_array *a, const mi_array *b, double *result, mi_stream stream);
/* x*x, y*y, x*y of two float images in one pass: the second-moment inputs of SSIM
 * (skimage/metrics/_structural_similarity.py:189-214 forms them with three multiplies). */
int mi_ssim_products(const mi_array *x, const mi_array *y, const mi_array *xx, const mi_array *yy,
                     const mi_array *xy, mi_stream stream);
/* SSIM map from the five filtered moments in one pass, float32 / float64, contiguous:
 * S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), v* = cov_norm (u** - u* u*)
 * (skimage/metrics/_structural_similarity.py:206-227).  gA/gB/gC (all or none) receive the three
 * fields the gradient filters (A1/D, -S/B2, (ux(A2-A1) - uy(B2-B1)S)/D; :235-243). */
int mi_ssim_combine(const mi_array *ux, const mi_array *uy, const mi_array *uxx, const mi_array *uyy,
                    const mi_array *uxy, const mi_array *S, const mi_array *gA, const mi_array *gB,
                    const mi_array *gC, double cov_norm, double C1, double C2, mi_stream stream);
/* The SSIM map (optional: S may be NULL) and the SUM of the map cropped by `pad` samples on
 * every side (the mean of _structural_similarity.py:240-243) in the same pass; rank 1..3,
 * no gradient fields.  *sum_out is a host double (the call synchronises the stream). */
int mi_ssim_combine_mean(const mi_array *ux, const mi_array *uy, const mi_array *uxx,
                         const mi_array *uyy, const mi_array *uxy, const mi_array *S, int pad,
                         double cov_norm, double C1, double C2, double *sum_out,
                         mi_stream stream);

/* ------------------------------------------------------------------ */
/* K8: measurements (label and labelled reductions)                     */
/* ------------------------------------------------------------------ */
/* Connected components of a contiguous array of rank 1..8 and fewer than 2**31 voxels, numbered as
 * scipy.ndimage.label numbers them (cupyimg/scipy/ndimage/measurements.py:29-199): raster order of each feature's
 * first voxel.  A voxel is foreground when it differs from `background` (0 for scipy; skimage.measure.label's
 * `background`, skimage/measure/_label.py:108-114; a background the input dtype cannot hold equals no voxel); `structure` is 3**ndim bytes, assumed centrosymmetric.
 * greyscale != 0 connects only neighbours of equal value (measurements.py:145-199, skimage semantics).  `out` is int32,
 * contiguous, of the input's shape (it holds the union-find parents until the last pass); *num_features is written on
 * the host (the call synchronises the stream). */
int mi_label(const mi_array *in, const mi_array *out, const uint8_t *structure, int greyscale, int64_t background,
             int64_t *num_features, mi_stream stream);
/* Labelled reductions (measurements.py:316-1464): op 0 sum, 1 mean, 2 variance, 3 standard deviation (float64 out,
 * one value per index entry), 4 extrema (out: input dtype (K, 2) = minimum, maximum; out_pos, optional: int64 (K, 2)
 * linear indices of the first minimum and first maximum in C order, of the LAST NaN where the maximum is NaN),
 * 5 center of mass (float64 (K, ndim)), 6 histogram (int64 (K, bins + 1): bin k counts edges[k] <= v < edges[k + 1],
 * the last bin closed, as numpy.histogram against scipy's float64 linspace(min, max, bins + 1) `edges`; the extra last
 * column counts the region's voxels outside [edges[0], edges[bins]] and NaNs, so a region with no voxel sums to 0).
 * `labels` (int32 / int64, or NULL: one region of every voxel) has the input's shape; `index` (int64, K values in
 * [imin, imax], or NULL: the voxels with labels > 0 form one region) names the regions: a lookup table over
 * [imin, imax] unless sorted_index != 0 (index sorted and unique: binary search).  Extrema and their positions treat
 * -0.0 and +0.0 as equal.  An index value no voxel carries gives sum 0, NaN for the means and centres, 0 for extrema
 * and -1 for positions.  Flags or'ed into `op`: MI_REDUCE_NONZERO (no index: the voxels with labels != 0 form the
 * region, for uint64 labels passed as int64), MI_REDUCE_PRESENCE (op 4 with out_pos: out_pos gets 0 where a voxel
 * carries the index value and -1 where none does, without the position pass).  Sums are in float64 with atomic adds:
 * integer inputs are exact below 2**53, float results vary in their last bits with the atomics' arrival order (not
 * bit-reproducible from run to run).  float16 inputs are converted to float32 by the caller. */
#define MI_REDUCE_NONZERO 0x100
#define MI_REDUCE_PRESENCE 0x200
int mi_labeled_reduce(int op, const mi_array *in, const mi_array *labels, const mi_array *index, int64_t imin,
                      int64_t imax, int sorted_index, const double *edges, int bins,
                      const mi_array *out, const mi_array *out_pos, mi_stream stream);

/* ------------------------------------------------------------------ */
/* K1: correlate family                                                 */
/* ------------------------------------------------------------------ */
/* One separable pass: out[.., o, ..] = sum_k w[k] * ext(in)[.., o - (wlen/2 + origin) + k, ..]
 * Replaces the K1 launch reached from correlate1d/convolve1d/gaussian_filter1d
 * (filters.py:213-283 -> :441-495 -> _filters_core.py:112-156).
 * acc_f32 != 0 selects float32 accumulation (dtype_mode="float",
 * _util.py:28-40), only honoured when promote(in, f32) == f32. */
int mi_correlate1d(const mi_array *in, const mi_array *out, int axis, const double *weights,
                   int wlen, int origin, int mode, double cval, int acc_f32, mi_stream stream);

/* Box mean along one axis with SciPy's sum-then-divide arithmetic (exact for
 * integer data); replaces the K1 launch behind uniform_filter1d
 * (filters.py:549-599). */
int mi_uniform_filter1d(const mi_array *in, const mi_array *out, int axis, int size, int origin,
                        int mode, double cval, mi_stream stream);

/* Fused separable 3-D filter, float32 -> float32, all three 1-D passes in one
 * launch (8 B/voxel of HBM traffic).  Replaces the three K1 launches plus the
 * zero-fills and copy-backs of uniform_filter / gaussian_filter
 * (filters.py:602-665, :725-792; _filters_core.py:148-155).
 * weights[a] (host, wlen[a] doubles) may be NULL for an axis that is not
 * filtered.  is_box != 0: all given weights are 1/wlen (sum-then-scale path).
 * Returns MI_ERR_UNSUPPORTED when no fused kernel covers the request.
 * Precision: weights, cval, products and partial sums are float32 whatever the
 * caller's dtype_mode (the reference accumulates in float64 by default).  The
 * tested bound, per output voxel: |out - exact| <= c * 2^-24 * B, where B is the
 * same filter applied to |in| with |weights| and |cval|, and c = sum over the
 * filtered axes of (wlen + 2) (tests/test_gpu_value_ranges.py). */
int mi_separable3d_f32(const mi_array *in, const mi_array *out, const double *const weights[3],
                       const int wlen[3], const int origin[3], const int mode[3], double cval,
                       int is_box, mi_stream stream);

/* Same filter restricted to one or two ranges of OUTPUT planes (axis 0):
 * planes = {begin0, end0[, begin1, end1]}, ascending and disjoint.  Boundary
 * handling still refers to the whole array; planes outside the ranges are
 * neither read for their own sake nor written.  New (the reference is
 * single-GPU): lets a slab rank filter its interior while the halo planes are
 * still in flight and finish the planes next to the halos afterwards. */
int mi_separable3d_f32_planes(const mi_array *in, const mi_array *out, const double *const weights[3],
                              const int wlen[3], const int origin[3], const int mode[3], double cval,
                              const int64_t *planes, int nranges, mi_stream stream);

/* Would mi_separable3d_f32 (plane_ranges = 0) / mi_separable3d_f32_planes (plane_ranges != 0) take this request?
 * MI_OK / MI_ERR_UNSUPPORTED / an argument error, decided by a dry run of the same dispatch code; nothing is
 * queued.  A plane-range request is judged as a partial one whatever ranges a caller would pass, so every rank of a
 * slab chain gets the same answer (r4; lets callers pick a schedule identically on all ranks). */
int mi_separable3d_f32_supports(const mi_array *in, const mi_array *out, const double *const weights[3],
                                const int wlen[3], const int origin[3], const int mode[3], double cval,
                                int plane_ranges);

/* Dense n-D stencil (filters.py:65-210 -> :441-495): weights is a host array
 * of prod(wshape) doubles in C order, already flipped for convolution by the
 * caller; zero weights are skipped (_filters_core.py:242-246). */
int mi_correlate_nd(const mi_array *in, const mi_array *out, const double *weights,
                    const int64_t *wshape, const int *origins, int mode, double cval,
                    int acc_f32, mi_stream stream);
/* Precision of the dense float32 kernels: acc_f32 == 0 accumulates in float64 and
 * rounds once (bit-identical to SciPy); acc_f32 != 0 (stencil3s_kernel in float
 * mode) accumulates in float32, tested to |out - exact| <= (n + 2) * 2^-24 * B with
 * n the nonzero weights and B the correlate of |in| with |weights| and |cval|. */
/* The dense 3 x 3 x 3 / 5 x 5 x 5 (with acc_f32: 7 x 7 x 7) window without zero weights on a float32 volume through stencil3s_kernel only
 * -- rows of ANY length, x origin 0 -- or MI_ERR_UNSUPPORTED with nothing queued (mi_correlate_nd never refuses: it ends at the
 * generic gather kernel).  For callers that would otherwise extend ragged rows for the tiled kernel (filters.py:65-210). */
int mi_correlate3_dense(const mi_array *in, const mi_array *out, const double *weights,
                        const int64_t *wshape, const int *origins, int mode, double cval,
                        int acc_f32, mi_stream stream);

/* ------------------------------------------------------------------ */
/* K2: min / max family (grey morphology)                               */
/* ------------------------------------------------------------------ */
/* 1-D running min/max (filters.py:1478-1507), compared in double like SciPy's
 * line buffers. */
int mi_minmax1d(const mi_array *in, const mi_array *out, int axis, int size, int origin,
                int mode, double cval, int is_max, mi_stream stream);

/* Fused separable 3-D min/max for uint8 volumes (grey_erosion/grey_dilation
 * with `size`, morphology.py:769-884 -> filters.py:1385-1396): one launch,
 * 2 B/voxel.  MI_ERR_UNSUPPORTED when not applicable. */
int mi_minmax3d_u8(const mi_array *in, const mi_array *out, const int size[3],
                   const int origin[3], const int mode[3], int cval, int is_max,
                   mi_stream stream);

/* Same for float32 volumes (flat odd sizes <= 9 per axis, x origin 0): streaming
 * passes with the comparisons of the generic kernel, x window fused into the z
 * (or, for one-plane volumes = images, the y) pass.  cval is converted to
 * float32 first, as SciPy converts it to the input dtype. */
int mi_minmax3d_f32(const mi_array *in, const mi_array *out, const int size[3], const int origin[3],
                    const int mode[3], double cval, int is_max, mi_stream stream);
/* mi_minmax3d_u8 / mi_minmax3d_f32 restricted to one or two ranges of output planes [b0, e0), [b1, e1) along axis 0
 * (ascending, inside the volume) -- the multi-GPU slab schedule filters a rank's interior planes while the halo exchange
 * is in flight and the planes next to a neighbour afterwards (r3).  Only what the single-launch kernels take: uint8
 * cubic sizes 3 / 5 / 7 with origin 0; float32 cubic odd sizes 3 .. 9, index-mapping boundary modes;
 * MI_ERR_UNSUPPORTED otherwise (callers then use the plain schedule on the whole extended slab). */
int mi_minmax3d_u8_planes(const mi_array *in, const mi_array *out, const int size[3], const int origin[3],
                          const int mode[3], int cval, int is_max, const int64_t *planes, int nranges,
                          mi_stream stream);
int mi_minmax3d_f32_planes(const mi_array *in, const mi_array *out, const int size[3], const int origin[3],
                           const int mode[3], double cval, int is_max, const int64_t *planes, int nranges,
                           mi_stream stream);


/* uint16 / int16 images and volumes (2-D or 3-D arrays; size / origin / mode always have
 * three entries, the first one for the absent axis of an image): flat min / max with odd
 * sizes <= 9 and origin 0 as streaming passes on packed 16-bit pairs -- images and
 * slice-wise filters one launch (4 B/pixel), volumes two.  MI_ERR_UNSUPPORTED otherwise. */
int mi_minmax3d_16(const mi_array *in, const mi_array *out, const int size[3], const int origin[3],
                   const int mode[3], int cval, int is_max, mi_stream stream);

/* uniform_filter on a uint8 image (a uint8 volume: slice by slice) with a uint8 result
 * (filters.py:602-665 -> :549-599, every intermediate stored in the output dtype): one
 * streaming launch in integer arithmetic -- q = trunc(row sum / size[0]) as uint8, then
 * trunc(column sum of q / size[1]).  Odd sizes <= 9 (1 = axis not filtered), origin along y
 * only, mode[2] = y, x.  MI_ERR_UNSUPPORTED otherwise (-> mi_uniform_filter1d per axis). */
int mi_uniform2d_u8(const mi_array *in, const mi_array *out, const int size[2], int origin_y,
                    const int mode[2], int cval, mi_stream stream);
/* the same for uint16 / int16 images (32-bit sums) */
int mi_uniform2d_16(const mi_array *in, const mi_array *out, const int size[2], int origin_y,
                    const int mode[2], int cval, mi_stream stream);
/* The z pass of uniform_filter on a uint8 / 16-bit VOLUME, intermediate in the same dtype
 * (SciPy filters axis 0 first): trunc(sum of size_z planes / size_z), odd size 3 .. 9;
 * mi_uniform2d_* on the result completes the filter. */
int mi_uniform_z_u8(const mi_array *in, const mi_array *out, int size_z, int origin_z, int mode_z,
                    int cval, mi_stream stream);
int mi_uniform_z_16(const mi_array *in, const mi_array *out, int size_z, int origin_z, int mode_z,
                    int cval, mi_stream stream);

/* Flat footprint min / max on uint8 images (volumes: slice by slice) for footprints whose
 * rows are centred runs -- disk, diamond / cross, octagon, square, i.e. what skimage's
 * morphology passes (skimage/morphology/grey.py -> morphology.py:769-884 ->
 * filters.py:1398-1419): footprint row r (0 .. nrows-1, nrows odd <= 9) covers the columns
 * -half_width[r] .. +half_width[r] (<= 4; -1 = empty row), origin 0.  One streaming
 * launch, bit-exact.  mode[2]: y and x.  MI_ERR_UNSUPPORTED otherwise (-> mi_minmax_nd). */
int mi_minmax_runs_u8(const mi_array *in, const mi_array *out, int nrows, const int *half_width,
                      const int mode[2], int cval, int is_max, mi_stream stream);
/* 3 x 3 x 3 footprints of centred x runs on uint8 / bool volumes -- the 6- / 18- / 26-connected
 * structures of generate_binary_structure(3, k), morphology.py:174-201 -- as one streaming
 * launch: half_width[3 * (dz + 1) + (dy + 1)] in {-1 (no sample), 0 (centre voxel), 1 (three
 * voxels)}, mode[3] = z, y, x.  Grey erosion / dilation with such a footprint
 * (morphology.py:769-884 -> filters.py:1398-1419).  MI_ERR_UNSUPPORTED otherwise. */
int mi_minmax_runs3d_u8(const mi_array *in, const mi_array *out, const int half_width[9],
                        const int mode[3], int cval, int is_max, mi_stream stream);
/* the same for float32 images (compare-select like the generic kernel; cval converted to
 * float32 first) */
int mi_minmax_runs_f32(const mi_array *in, const mi_array *out, int nrows, const int *half_width,
                       const int mode[2], double cval, int is_max, mi_stream stream);
/* the same for uint16 / int16 images */
int mi_minmax_runs_16(const mi_array *in, const mi_array *out, int nrows, const int *half_width,
                      const int mode[2], int cval, int is_max, mi_stream stream);

/* float64 images and volumes (skimage's working dtype): the separable filter and the
 * flat min / max as streaming passes, x fused into the streamed pass when the tap
 * counts agree -- an image or a slice-wise filter is one launch (16 B/pixel), a volume
 * two.  weights[a] NULL = axis not filtered; odd tap counts <= 33 (min / max: odd
 * sizes <= 9), x origin 0, even x extent.  MI_ERR_UNSUPPORTED otherwise (the caller
 * runs mi_correlate1d / mi_minmax1d per axis). */
int mi_separable3d_f64(const mi_array *in, const mi_array *out, const double *const weights[3],
                       const int wlen[3], const int origin[3], const int mode[3], double cval,
                       mi_stream stream);
int mi_minmax3d_f64(const mi_array *in, const mi_array *out, const int size[3], const int origin[3],
                    const int mode[3], double cval, int is_max, mi_stream stream);

/* n-D footprint (+ optional non-flat structure) min/max
 * (filters.py:1398-1419, kernel :1510-1557).  footprint: host uint8
 * prod(fshape); structure: host doubles or NULL. */
int mi_minmax_nd(const mi_array *in, const mi_array *out, const uint8_t *footprint,
                 const double *structure, const int64_t *fshape, const int *origins, int mode,
                 double cval, int is_max, mi_stream stream);

/* rank-th smallest sample under the footprint (rank_filter / median_filter /
 * percentile_filter, filters.py:1560-1848).  Arrays of rank <= 3 with footprints of at
 * most 128 set elements take register kernels (sorting networks / partial selection);
 * anything else -- rank 4..8, larger footprints -- a scratch-column shell sort (r3; the
 * reference's shell-sort path, filters.py:1753-1768, has no limit either; scratch from the
 * pool, at most 256 MiB).  cval is converted to the input dtype like SciPy does.
 * NaN contract (r5 advisor finding): float32 windows are sorted on order-preserving integer keys -- NaNs with a clear
 * sign bit sort above +inf, with a set sign bit below -inf, and -0 below +0 (what numpy.sort does for the positive
 * NaNs NumPy produces); float64 windows use compare-select / v_min_f64 / v_max_f64, which pass over NaNs: a float64
 * volume that holds NaNs has NO guaranteed rank-filter result (SciPy's own depends on its partial sort), finite data
 * and infinities are exact for both dtypes. */
int mi_rank_filter(const mi_array *in, const mi_array *out, const uint8_t *footprint,
                   const int64_t *fshape, const int *origins, int rank, int mode, double cval,
                   mi_stream stream);

/* 3 x 3 median over the last two axes of a 2-D / 3-D float32, float64, uint8, uint16 or int16 array
 * (median_filter(size=3) / rank_filter(rank=4) with a full 3 x 3 footprint,
 * filters.py:1560-1701,1751-1792; skimage.filters.median's default on images):
 * one streaming launch at 8 (float32) / 2 (uint8) / 4 (16-bit) B/pixel instead of the
 * generic gather-and-sort kernel.  mode[2]: boundary modes along y and x.
 * MI_ERR_UNSUPPORTED when not applicable (the caller runs mi_rank_filter). */
int mi_median3x3(const mi_array *in, const mi_array *out, const int mode[2], double cval,
                 mi_stream stream);

/* ------------------------------------------------------------------ */
/* K4: binary erosion / dilation                                        */
/* ------------------------------------------------------------------ */
/* One iteration of erode_kernel (morphology.py:41-128, launched at :292-322).
 * `in` any real dtype (nonzero = true); `out` any real dtype (0/1 written).
 * structure: host uint8 prod(sshape).  mask may be NULL.  invert = 1 turns
 * it into dilation (morphology.py:443-461).  If changed_dev is not NULL,
 * *changed_dev (device int32) is OR-ed with 1 when any output voxel differs
 * from the input voxel -- the on-device replacement for the host-side
 * `(tmp_in == tmp_out).all()` sync at morphology.py:313,321. */
int mi_binary_erosion(const mi_array *in, const mi_array *out, const uint8_t *structure,
                      const int64_t *sshape, const int *origins, const mi_array *mask,
                      int border_value, int invert, int32_t *changed_dev, mi_stream stream);

/* `iterations` (1 .. MI_BINARY_MAX_FUSED) iterations of the same erosion / dilation in ONE launch -- the host loop of
 * morphology.py:301-327 (one launch and one host synchronisation per iteration) folded into the tile residency: the
 * volume is staged as 1 bit per voxel and the intermediate results never reach HBM (csrc/bitmorph3d.hip).  The result
 * is that of `iterations` calls of mi_binary_erosion (mask, border_value, origins applied in every iteration).
 * changed_dev: NULL or a device int32[iterations]; element j is OR-ed with 1 when iteration j + 1 changed a voxel
 * (so a run "until stable" stops at the first zero).  3-D volumes of 1-byte voxels with rows that are a multiple of
 * 16 bytes; anything else returns MI_ERR_UNSUPPORTED with nothing queued and the caller iterates mi_binary_erosion. */
#define MI_BINARY_MAX_FUSED 8
/* binary_opening (closing = 0) / binary_closing (closing = 1) with `iterations` iterations of each half in ONE launch
 * (morphology.py:464-613 run the two halves as separate calls with a temporary volume): stages 1 .. iterations are the
 * first operation, the rest the second with the mirrored structure; 2 * iterations <= MI_BINARY_MAX_FUSED, odd structure
 * extents, origin 0; otherwise MI_ERR_UNSUPPORTED with nothing queued (the caller runs the two halves). */
int mi_binary_open_close_fused(const mi_array *in, const mi_array *out, const uint8_t *structure,
                               const int64_t *sshape, const mi_array *mask, int border_value, int closing,
                               int iterations, mi_stream stream);
/* One launch of a masked dilation's block-wise fill towards its fixed point -- binary_propagation / binary_fill_holes
 * (morphology.py:684-766: dilation with iterations = -1 inside a mask).  Every workgroup sweeps a block of the volume IN
 * PLACE (bits in LDS; whole runs of mask bits along x filled per sweep by the carry of an addition) until nothing inside
 * the block changes, its halo being what the neighbours held when the launch began; the operator is monotone, so repeating
 * launches (in -> out, ping-pong) until *changed_dev stays 0 reaches exactly the fixed point the reference's
 * one-iteration-per-launch loop reaches.  structure / origins in the form mi_binary_erosion takes with invert = 1
 * (already mirrored).  MI_ERR_UNSUPPORTED outside the envelope (3-D byte volumes with a byte mask, rows of 64 .. 2048
 * voxels, a structure that holds its centre): the caller iterates mi_binary_erosion_fused. */
int mi_binary_propagation_step(const mi_array *in, const mi_array *out, const uint8_t *structure,
                               const int64_t *sshape, const int *origins, const mi_array *mask,
                               int border_value, int32_t *changed_dev, mi_stream stream);
int mi_binary_erosion_fused(const mi_array *in, const mi_array *out, const uint8_t *structure,
                            const int64_t *sshape, const int *origins, const mi_array *mask,
                            int border_value, int invert, int iterations, int32_t *changed_dev, mi_stream stream);

/* One launch of grey-level morphological reconstruction (skimage.morphology.reconstruction; the reference runs its inner
 * loop on the host, cupyimg/skimage/morphology/greyreconstruct.py:227-231).  With S = the offsets d = position - offsets of
 * the true cells of `structure` (host uint8 prod(sshape); the cell at `offsets` itself is ignored), `out` is `in` moved
 * towards the fixed point of
 *     R[q] <- min(mask[q], max(R[q], max over d in S of R[q - d]))         method 0, dilation
 *     R[q] <- max(mask[q], min(R[q], min over d in S of R[q - d]))         method 1, erosion
 * (positions outside the array contribute nothing).  The operator is monotone: repeating launches (in -> out, ping-pong)
 * until flags_dev[0] stays 0 reaches the unique fixed point, bit for bit, whatever a launch does inside.  2-D / 3-D arrays
 * of uint8 / int16 / uint16 / float32 with the 3^n box or the connectivity-1 cross centred on its middle: every workgroup
 * relaxes a block of the array in LDS until nothing inside it changes (csrc/reconstruct.hip: greyrec3_kernel), its halo being
 * what the neighbours held when the launch began; anything else: one step of the rule per launch.  in, out, mask:
 * C-contiguous, one shape, one dtype; out overlaps neither.  flags_dev: device int32[2], zeroed by the caller; [0] is OR-ed
 * with 1 when a voxel of out differs from in, [1] when in > mask (erosion: in < mask) somewhere.  float16: MI_ERR_UNSUPPORTED
 * with nothing queued (the caller converts to float32, which is exact for an operation that only compares and copies). */
int mi_grey_reconstruction_step(const mi_array *in, const mi_array *out, const mi_array *mask, const uint8_t *structure,
                                const int64_t *sshape, const int *offsets, int method, int32_t *flags_dev, mi_stream stream);

/* One iteration of Chambolle's projection algorithm for total-variation denoising (skimage.restoration.denoise_tv_chambolle;
 * the reference runs an iteration as about 25 whole-array operations and synchronises with the host for its stopping test,
 * cupyimg/skimage/restoration/_denoise.py:44-86).  Two launches are queued: the iteration kernel and a one-workgroup energy /
 * stop step; nothing synchronises.  With tau = 1 / (2 * image.ndim), T the image dtype and all arithmetic in T, products and
 * sums rounded one by one:
 *     d(q)   = -((p_0(q) + p_1(q)) + ...), then for a = 0, 1, ...: d += p_a(q - e_a) where q_a >= 1
 *     out(q) = image(q) + d(q);   g_a(q) = out(q + e_a) - out(q) where q_a < n_a - 1, else 0
 *     norm   = sqrt((g_0 g_0 + g_1 g_1) + ...);   den = norm * T(tau / weight) + 1;   p_out_a = (p_in_a - T(tau) g_a) / den
 *     E_i    = (sum d d + weight * sum norm) / image.size        both sums and E in double, in an order fixed by the shape
 * image: C-contiguous float32 / float64 of rank 1 .. MI_MAX_NDIM.  p_in, p_out: C-contiguous (image.ndim, image.size) arrays of
 * the image's dtype, component a of voxel q at [a][q]; the caller zeroes p_in before iteration 0 and swaps the two between
 * calls; p_out may hold anything (every element is written) and is not p_in.  work_dev: MI_TV_WORK_BYTES of device memory
 * that one run of the algorithm keeps to itself.  Its first MI_TV_STATE_BYTES are the state block, zeroed by the caller
 * before iteration 0: int32 stopped, int32 stop_iter, int32 done (iterations that ran), int32 unused, double E_prev, double
 * E_0, double E of the last iteration that ran; the rest holds the workgroups' partial sums and needs no initialisation.
 * `iteration` counts from 0.  The stop step of iteration i >= 1 sets stopped = 1 and stop_iter = i when
 * |E_prev - E_i| < eps * E_0, else E_prev = E_i.  Every launch queued after that reads `stopped` first and touches nothing, so
 * the caller may queue iterations in batches and read the state block once per batch.  After a stop the p to use (the
 * reference returns `out` as computed at the start of the iteration that stopped, _denoise.py:55,82-87) is the p_in of
 * iteration stop_iter, that is the buffer that was p_in in every call with iteration = stop_iter mod 2; the same holds for
 * the last iteration when the loop runs out.  2-D and 3-D arrays: a fused kernel that streams along axis 0 with `out` in a
 * two-plane window in LDS and reads image and p_in once, tile halos apart (csrc/tv_chambolle.hip: tv_fused_kernel); other
 * ranks: one thread per voxel.  Other dtypes: MI_ERR_UNSUPPORTED with nothing queued (the caller converts). */
#define MI_TV_STATE_BYTES 64
#define MI_TV_MAX_PARTIALS 65536
#define MI_TV_WORK_BYTES (MI_TV_STATE_BYTES + 16 * MI_TV_MAX_PARTIALS)
int mi_tv_chambolle_step(const mi_array *image, const mi_array *p_in, const mi_array *p_out, double weight, double eps,
                         int iteration, void *work_dev, mi_stream stream);
/* out = image + d(p), d as above: the denoised image for a given dual field.  out: C-contiguous, the image's shape and dtype,
 * overlaps neither image nor p. */
int mi_tv_chambolle_output(const mi_array *image, const mi_array *p, const mi_array *out, mi_stream stream);

/* The Hessian family (skimage.feature.hessian_matrix / hessian_matrix_eigvals, skimage.filters.frangi / sato / meijering;
 * cupyimg/skimage/feature/corner.py:141-211, 260-309, cupyimg/skimage/filters/ridges.py:112-533): what follows the Gaussian
 * of one scale.  All arithmetic in the dtype T of the smoothed array g (float32 / float64, C-contiguous, rank 1 ..
 * MI_MAX_NDIM, at least 2 samples along every axis), products and sums rounded one by one.
 *
 * mi_hessian_matrix: out[e] = gradient(gradient(g)[a0], axis = a1), numpy.gradient with unit spacing and edge_order 1
 * ((f[i+1] - f[i-1]) / 2 inside, f[1] - f[0] and f[n-1] - f[n-2] at the ends, applied twice), for the e-th pair (a0, a1) of
 * combinations_with_replacement(axes, 2), axes = ndim-1 .. 0 (order_xy = 0, the reference's order "rc") or 0 .. ndim-1
 * (order_xy = 1, "xy"); bit-identical to NumPy on the same g.  out: C-contiguous (ndim (ndim + 1) / 2, g.size) of g's dtype.
 * Rank 2 and 3: one launch that stages tiles of g with a two-sample halo in LDS (one read of g, 3 or 6 writes); other ranks
 * one thread per voxel.
 *
 * mi_symmetric_eigvals: the eigenvalues, decreasing, of the symmetric ndim x ndim matrices whose upper triangles, row by row,
 * are elems[0 .. ndim (ndim + 1) / 2) (each of `size` values): out C-contiguous (ndim, size) of the same dtype.  2 x 2: the
 * reference's closed form operation by operation; larger: cyclic Jacobi, every eigenvalue within a few eps * ||A||_F of the
 * exact one (LAPACK is not bit-reproduced).
 *
 * mi_ridge_scale: Hessian elements in "rc" order from g, times T(sigma^2), eigenvalues, ordering and one of
 *   MI_RIDGE_EIGENVALUES  out: (ndim, g.size) of g's dtype, the eigenvalues ordered by `sorting` (NONE = decreasing, VAL =
 *                         increasing, ABS = stable sort of the decreasing list by magnitude)
 *   MI_RIDGE_FRANGI       p0, p1, p2 = 2 alpha^2, 2 beta^2, 2 gamma^2; 2-D and 3-D
 *   MI_RIDGE_SATO         2-D and 3-D
 *   MI_RIDGE_MEIJERING    p0 = alpha; scratch: a volume of g's shape and dtype that receives aux; work_dev: 8 bytes the
 *                         caller set to 0xff before the call, afterwards the order-preserving key of min(aux) (a double's
 *                         bits, inverted when negative, else with the sign bit set); a second launch normalises by that
 *                         minimum read on the device
 * for the three responses out is float64 of g's shape and is updated in place: out = max(out, response).  2-D and 3-D: one
 * launch from the staged tile with nothing but out written; other ranks, or after mi_debug_set_ridges(.., .., 1): the
 * elements in pool memory, then one thread per voxel -- the same arithmetic, the same bits. */
#define MI_RIDGE_EIGENVALUES 0
#define MI_RIDGE_FRANGI 1
#define MI_RIDGE_SATO 2
#define MI_RIDGE_MEIJERING 3
#define MI_RIDGE_SORT_NONE 0
#define MI_RIDGE_SORT_VAL 1
#define MI_RIDGE_SORT_ABS 2
int mi_hessian_matrix(const mi_array *g, const mi_array *out, int order_xy, mi_stream stream);
int mi_symmetric_eigvals(const mi_array *elems, const mi_array *out, int ndim, mi_stream stream);
int mi_ridge_scale(const mi_array *g, const mi_array *out, int kind, int sorting, double sigma, double p0, double p1, double p2,
                   const mi_array *scratch, void *work_dev, mi_stream stream);
/* a[a <= 0] = value in place (the last step of skimage.filters.hessian, ridges.py:634); a: C-contiguous float64 */
int mi_ridge_fill_nonpositive(const mi_array *a, double value, mi_stream stream);

/* skimage.exposure.equalize_adapthist (contrast limited adaptive histogram equalisation, cupyimg/skimage/exposure/
 * _adapthist.py:86-275) as three launches without a host round trip; the reference pads the image, gathers every contextual
 * region into a 2-D array, clips the histograms in a Python loop on the host and blends in 2^ndim rounds of whole-array
 * operations.  Bit-identical to it.  With s_a the shape, k_a the kernel size, K = prod(k), every floating-point operation
 * rounded on its own (the source is compiled without contraction):
 *   1  u = img_as_uint(image): uint8 x 257; uint16 as it is; floats uint16(clip(rint(x * 65535), 0, 65535)) in the image dtype
 *   2  g = uint16(rint((clip(u, umin, umax) - umin) / (umax - umin) * 16383.0 + 0.0)) in float64, umin and umax over the whole
 *      image; min(u, 16383) when umin == umax
 *   3  b = g // (1 + 16384 // nbins)
 *   4  contextual regions of side k_a aligned to the image origin, ceil(s_a / k_a) per axis (the reference's int(S_a / k_a) - 1
 *      on its padded shape S_a = k_a (ceil(s_a / k_a) + 1)); a region that ends beyond the image reads b at the reflected
 *      index (numpy.pad "reflect": period 2 (s_a - 1), an axis of length 1 repeats its sample); nothing is padded in memory
 *   5  per region h = the nbins-bin histogram of b, clipped at `clip_limit`:
 *        E = sum max(h - c, 0); h = min(h, c); incr = E // nbins; upper = c - incr
 *        where h < upper: h += incr, E -= incr;  then where upper <= h < c: E -= c - h, h = c
 *        while E > 0: E0 = E; for index = 0 .. nbins - 1: step = max(1, #(h < c) // E); the bins index, index + step, ...
 *        that are below c gain 1 each and E loses their number; the round ends when E <= 0 (E may go below 0); the loop
 *        ends after a round that changed nothing
 *   6  map = int64(min(float64(cumsum(h)) * (16383 / K) + 0, 16383))
 *   7  voxel i: p_a = i_a + k_a // 2, cell B_a = p_a // k_a, j_a = p_a % k_a, c_a = j_a / k_a in float64.  For every corner e in
 *      itertools.product((0, 1), repeat = ndim) order: region r_a = clip(B_a - 1 + e_a, 0, regions_a - 1), weight w_a = c_a
 *      where e_a = 1, else 1 - c_a; term = float32(float64(map_r[b(i)]) * ((w_(n-1) * w_(n-2)) * ... * w_0)); the terms are
 *      added in float32 in that order; v = uint16(sum), truncated
 *   8  f = float64(v) * (1.0 / 65535); out = (f - fmin) / (fmax - fmin) * 1.0 + 0.0 with fmin, fmax over the whole array, f
 *      itself when they are equal
 * image: C-contiguous uint8 / uint16 / float32 / float64 of rank 1 .. MI_CLAHE_MAX_NDIM (other dtypes: MI_ERR_UNSUPPORTED,
 * nothing queued); kernel: host int[ndim], each at least 1, prod(kernel) at most 2^30; umin, umax: the extrema of u (step 1 of
 * the image's extrema: the conversion is monotone); nbins 1 .. MI_CLAHE_GRAY; maps: C-contiguous uint16 (regions, nbins),
 * regions in row-major order.
 *
 * mi_clahe_maps (steps 1 - 6): one workgroup per region histograms in LDS (a histogram per wave up to 1024 bins, merged before
 * the clip; one shared histogram above that, or after mi_debug_set_clahe(.., 1)), clips with one workgroup reduction per stage
 * and per strided pass, and writes the region's row of maps.  clip_limit: 1 .. prod(kernel).
 * mi_clahe_apply (steps 1 - 3, 7): out: C-contiguous uint16 of the image's shape, receives v.  work_dev: MI_CLAHE_WORK_BYTES of
 * device memory the caller set to 0xff; afterwards uint32 [0] = min v, [1] = 65535 - max v (one pair of atomics per
 * workgroup).  Rank 2 and 3 with (nbins << ndim) * 2 <= 65536 bytes of mappings and sum(kernel) <= 1024: a workgroup per slab of
 * an interpolation cell with the cell's 2^ndim mappings and the coefficients in LDS; otherwise, or after
 * mi_debug_set_clahe(1, ..): one thread per voxel, mappings from global memory -- the same arithmetic, the same bits.
 * mi_clahe_finish (step 8): v uint16, out float64, both C-contiguous of one shape; reads work_dev on the device. */
#define MI_CLAHE_MAX_NDIM 4
#define MI_CLAHE_GRAY 16384
#define MI_CLAHE_WORK_BYTES 16
int mi_clahe_maps(const mi_array *image, const int *kernel, double umin, double umax, int nbins, int64_t clip_limit,
                  const mi_array *maps, mi_stream stream);
int mi_clahe_apply(const mi_array *image, const int *kernel, double umin, double umax, int nbins, const mi_array *maps,
                   const mi_array *out, void *work_dev, mi_stream stream);
int mi_clahe_finish(const mi_array *v, const mi_array *out, const void *work_dev, mi_stream stream);

/* out = numpy.interp(image, xp, fp) in float64: with j the last knot at or below x, fp[j] + ((fp[j+1] - fp[j]) / (xp[j+1] -
 * xp[j])) * (x - xp[j]), slope times difference first; fp[0] below xp[0], fp[n-1] above xp[n-1], fp[j] where x == xp[j]; NaN
 * stays NaN (skimage.exposure.equalize_hist, for which the reference pulls the image to the host, exposure.py:253-256).
 * image: C-contiguous uint8 / uint16 / float32 / float64; xp (increasing), fp: device float64 vectors of 1 ..
 * MI_INTERP_MAX_KNOTS knots, staged in LDS up to 4096 knots, searched in global memory above; out: float64, the image's shape. */
#define MI_INTERP_MAX_KNOTS 65536
int mi_interp_map(const mi_array *image, const mi_array *xp, const mi_array *fp, const mi_array *out, mi_stream stream);

/* skimage.exposure.rescale_intensity (exposure.py:439-463): x = clip(image, imin, imax), then ((x - imin) / (imax - imin)) *
 * (omax - omin) + omin, every operation rounded on its own, in float32 for a float32 image (the four scalars and the two
 * differences, formed in double, rounded to float32 first) and in float64 for every other dtype; with imin == imax only
 * clip(x, omin, omax).  The result is converted to out's dtype by truncation.  image, out: C-contiguous, one shape, any
 * dtype but float16. */
int mi_rescale_intensity(const mi_array *image, const mi_array *out, double imin, double imax, double omin, double omax,
                         mi_stream stream);

/* Morphological snakes (skimage.segmentation.morphological_chan_vese / morphological_geodesic_active_contour, sup_inf, inf_sup;
 * cupyimg/skimage/segmentation/morphsnakes.py:55-92, 347-378, 468-510; csrc/morphsnakes.hip).  The level set u is a C-contiguous
 * int8 array of 0 and 1 of rank 2 or 3, the image a C-contiguous float32 / float64 array (T) of the same shape (other dtypes:
 * MI_ERR_UNSUPPORTED with nothing queued, the caller converts).  An iteration is a chain of radius-1 stages; voxels outside the
 * array count as 0 in the morphological ones:
 *     dilate / erode  u' = OR / AND of u over the 3^ndim neighbourhood where double(image) > mask_threshold, else u
 *     acwe    du_a = numpy.gradient(u) along axis a ((u[+1] - u[-1]) / 2 inside, one-sided differences at the two ends); where some
 *             du_a != 0: b = T(lambda1) (I - c1)^2 - T(lambda2) (I - c0)^2 in T, b < 0: u' = 1, b > 0: u' = 0; else u' = u
 *     gac     aux = ((0 + gI_0 du_0) + gI_1 du_1) + ..., gI = numpy.gradient(image), in T; aux > 0: u' = 1, aux < 0: u' = 0
 *     SI      u' = OR over the 9 planes (rank 3) / 4 lines (rank 2) P of morphsnakes.py:33-49 of (AND of u over P)    (sup_inf)
 *     IS      u' = AND over the same P of (OR of u over P)                                                             (inf_sup)
 * Smoothing step number j of a call (j = `first`, first + 1, ... over the `smoothing` steps of this iteration) is SI o IS for even
 * j and IS o SI for odd j.  The first launch of a chain runs the update stages and up to MI_SNAKE_FUSED_SMOOTHING smoothing
 * steps on overlapped boxes in LDS, every further launch two smoothing steps; launches alternate between u_out and u_tmp and
 * the last writes u_out.  u_in is only read; u_tmp (same shape, needed when the chain has more than one launch) is scratch.
 * No launch depends on data: their number is a function of `smoothing` alone, and nothing synchronises.
 * work_dev: MI_SNAKE_WORK_BYTES of device memory one run keeps to itself; its first MI_SNAKE_STATE_BYTES are the state block:
 * double c0, c1 (the means outside and inside, rounded to T), double[4] the sums of image (1 - u), image u, (1 - u), u, double[2]
 * the result of mi_snake_order_stats; the rest holds the workgroups' partial sums and needs no initialisation.
 * mi_snake_acwe_init: the four sums of (image, u), in double in an order fixed by the shape, and c0 = T(sum image (1 - u)) /
 * T(sum (1 - u) + 1e-8), c1 likewise, into the state block.  mi_snake_acwe_step: one iteration with the c0, c1 of the state
 * block; its last launch accumulates the sums of the new u and a one-workgroup launch renews c0 and c1. */
#define MI_SNAKE_STATE_BYTES 64
#define MI_SNAKE_MAX_PARTIALS 65536
#define MI_SNAKE_WORK_BYTES (MI_SNAKE_STATE_BYTES + 32 * MI_SNAKE_MAX_PARTIALS)
#define MI_SNAKE_FUSED_SMOOTHING 2
int mi_snake_acwe_init(const mi_array *image, const mi_array *u, void *work_dev, mi_stream stream);
int mi_snake_acwe_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, double lambda1,
                       double lambda2, int smoothing, int first, void *work_dev, mi_stream stream);
/* One MorphGAC iteration: balloon > 0: a dilate stage first, balloon < 0: an erode stage, 0: none; then gac and the smoothing. */
int mi_snake_gac_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, double mask_threshold,
                      int balloon, int smoothing, int first, mi_stream stream);
/* nops (1 .. 32) operators in a row, operator i = SI when bit i of ops is set, IS otherwise. */
int mi_snake_curvature(const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, int nops, unsigned ops, mi_stream stream);
/* The order statistics number k0 and k1 (from 0) of a C-contiguous float32 / float64 array, as doubles at bytes 48 .. 63 of the
 * state block: a radix select over order-preserving keys, 8 bits a pass, two launches a pass; nothing is sorted or stored. */
int mi_snake_order_stats(const mi_array *image, int64_t k0, int64_t k1, void *work_dev, mi_stream stream);
/* out (int8) = src > 0 (nonzero = 0) or src != 0 (nonzero = 1); src: C-contiguous, any dtype but float16. */
int mi_snake_binarize(const mi_array *src, const mi_array *out, int nonzero, mi_stream stream);
/* out = 1 / sqrt(1 + T(alpha) gradnorm) in T, every operation rounded on its own (inverse_gaussian_gradient, morphsnakes.py:266) */
int mi_snake_inverse_gradient(const mi_array *gradnorm, const mi_array *out, double alpha, mi_stream stream);

/* The TV-L1 optical flow solver (skimage.registration.optical_flow_tvl1; cupyimg/skimage/registration/_optical_flow.py:20-158,
 * which runs a fixed-point iteration as about 140 whole-array operations; csrc/tvl1.hip).  The images are C-contiguous float32 /
 * float64 arrays (T) of rank nd = 2 .. 4 with at least 2 samples along every axis (numpy.gradient's rule; other dtypes:
 * MI_ERR_UNSUPPORTED with nothing queued); flow, grad and coords have shape (nd, *shape), proj (nd, nd, *shape), all of dtype T
 * and C-contiguous.  All arithmetic in T, every product and sum rounded on its own, sums over the component axis left to right;
 * a fixed number of iterations gives the bits of a NumPy transcription of the reference.  Nothing synchronises.
 *
 * mi_tvl1_coords: coords_a(q) = T(q_a) + flow_a(q), the sampling points of the warp.
 * mi_tvl1_prepare (once per warp; w = the warped moving image):
 *     grad_a = numpy.gradient(w) along axis a: (w(q + e_a) - w(q - e_a)) / 2 inside, one-sided differences at the two ends
 *     NI     = (grad_0 grad_0 + grad_1 grad_1) + ..., 1 where that is 0
 *     rho_0  = (w - reference) - ((grad_0 flow_0 + grad_1 flow_1) + ...)
 * mi_tvl1_data (the data term, in place on `flow`, which then is the reference's flow_auxiliary):
 *     rho = rho_0 + ((grad_0 flow_0 + grad_1 flow_1) + ...)
 *     where |rho| <= T(f0) NI: flow_a -= (rho grad_a) / NI;  elsewhere: flow_a -= (T(f0) sign(rho)) grad_a
 * mi_tvl1_reg (the regularisation), for every flow component c with v = flow_aux[c], p^0 = proj_in[c], u^0 = v, for s = 1, 2:
 *     g_a    = u^(s-1)(q + e_a) - u^(s-1)(q) where q_a < n_a - 1, else 0
 *     norm   = sqrt((g_0 g_0 + g_1 g_1) + ...) * T(f1) + 1;   p^s_a = (p^(s-1)_a - T(dt) g_a) / norm
 *     d      = -((p^s_0(q) + p^s_1(q)) + ...), then for a = 0, 1, ...: d += p^s_a(q - e_a) where q_a >= 1;   u^s = v + d
 *   flow_out[c] = u^2, proj_out[c] = p^2.  flow_out is not flow_aux and proj_out is not proj_in (no workgroup reads what another
 *   writes in the same launch); the caller zeroes proj once per pyramid level and swaps the buffers between calls.  Rank 2 and
 *   3: one launch (tvl1_reg_fused_kernel: a workgroup stages one component of a tile of flow_aux with a halo of 2 voxels either
 *   way, and of proj_in with 2 voxels towards smaller and 1 towards larger indices, in LDS, streams along axis 0 and runs both
 *   steps in one tile residency).  Other ranks, or after mi_debug_set_tvl1(.., 1): four launches with one thread per voxel
 *   straight from global memory, p^1 and u^1 in scratch_dev, which then holds mi_tvl1_scratch_size elements of T (0 on the
 *   fused route, where scratch_dev may be NULL).  *launches (may be NULL) receives the number of launches queued.
 * mi_tvl1_diff_sum: sum (a - b)^2 over two arrays of one shape, the difference and its square in T, the sum in double from
 *   per-workgroup partials in an order fixed by the size (no floating-point atomics); work_dev: MI_TVL1_WORK_BYTES of device
 *   memory, the sum is the double at its start once the two launches have run. */
#define MI_TVL1_WORK_BYTES 16384
int mi_tvl1_coords(const mi_array *flow, const mi_array *coords, mi_stream stream);
int mi_tvl1_prepare(const mi_array *warped, const mi_array *reference, const mi_array *flow, const mi_array *grad,
                    const mi_array *ni, const mi_array *rho0, mi_stream stream);
int mi_tvl1_data(const mi_array *grad, const mi_array *ni, const mi_array *rho0, const mi_array *flow, double f0, mi_stream stream);
int mi_tvl1_scratch_size(const mi_array *flow, int64_t *elements);
int mi_tvl1_reg(const mi_array *flow_aux, const mi_array *proj_in, const mi_array *flow_out, const mi_array *proj_out,
                void *scratch_dev, double dt, double f1, int *launches, mi_stream stream);
int mi_tvl1_diff_sum(const mi_array *a, const mi_array *b, void *work_dev, mi_stream stream);

/* The n-D edge operators of skimage.filters -- sobel, scharr, prewitt, magnitude and single axis
 * (cupyimg/skimage/filters/edges.py:128-200, which runs a 3-D magnitude as three dense convolutions plus seven whole-array
 * passes; the mask: edges.py:55-65; csrc/edges.hip).  image: C-contiguous float32 / float64 (T; other dtypes:
 * MI_ERR_UNSUPPORTED with nothing queued) of rank 1 .. 8; out: float64, the image's shape; mask: NULL or the ERODED mask as a
 * bool / uint8 array of that shape; weights: naxes x 3^rank host doubles, per edge axis the dense kernel of edges.py:188-191
 * already flipped for correlation, C order; mode / cval as for mi_correlate_nd (the reference drops cval, edges.py:192).
 *     r_a = T(sum over the non-zero taps in C order, from 0.0, of double(x) * w), each product and sum rounded on its own
 *     out = 0.0; for every edge axis in order: out = out + double(magnitude ? r_a * r_a : r_a), the square in T
 *     magnitude: out = out / rank; out = sqrt(out)            (edges.py:197-199: by the rank, not by naxes)
 *     mask:      out = out * double(mask)                     (edges.py:64: -x * 0 = -0.0, NaN * 0 = NaN)
 *   magnitude == 0 takes exactly one edge axis (the signed response; 0.0 + -0.0 = +0.0 as in the reference).  Rank 2 and 3:
 *   one launch (edge_fused_kernel: a box of the image with a one-sample halo in LDS, borders by index arithmetic, the
 *   per-axis responses never in memory).  Other ranks, or after mi_debug_set_edges(.., 1): one mi_correlate_nd per edge axis
 *   into a pooled scratch array plus per-voxel launches, the same bits.  Nothing synchronises.
 * mi_edge_pair_magnitude (roberts, farid; edges.py:599-611, 759-769): out = sqrt(a * a + b * b) / T(divisor) on float32 /
 *   float64 arrays of one shape and dtype T, every operation in T and rounded on its own; out may be a or b.
 * mi_threshold_masks (apply_hysteresis_threshold, cupyimg/skimage/filters/thresholding.py:1218-1220): low is clipped to high
 *   per voxel (the smaller of the two; a NaN of either stays), then mask_low = image > low, mask_high = image > high in one
 *   launch, every operand as a double; image: any dtype but float16 and 64-bit integers; low /
 *   high: NULL (then the scalar low_value / high_value) or float64 arrays of the image's shape; the masks: bool / uint8. */
/* The stage of skimage.feature.canny between the smoothing and the hysteresis (cupyimg/skimage/feature/_canny.py:191-288, some
 * forty masked temporaries there).  smoothed: C-contiguous float64 image (ny, nx) -- _canny.py:46-50 divides by a float64
 * array, so the stage is float64 for every input dtype; eroded: the 3 x 3-eroded mask (border value 0, _canny.py:201-202) as
 * bool / uint8; magnitude (float64), local_max, high_mask, low_mask (bool / uint8; the last two may both be NULL): outputs.
 *     isobel, jsobel = scipy.ndimage.sobel(smoothed, axis = 0 / 1), mode 'reflect': two correlate1d passes in SciPy's order,
 *                      d = x(l) * 0.0 + (x(l - 1) - x(l + 1)) * -1.0 along the axis, then d(l) * 2.0 + (d(l - 1) + d(l + 1)) * 1.0
 *     magnitude      = sqrt(isobel * isobel + jsobel * jsobel), each operation rounded on its own (the reference calls
 *                      hypot, whose last bit is libm's: the one deliberate deviation)
 *     local_max      = eroded & (magnitude > 0) & [the class test], the four direction classes of _canny.py:210-275 with
 *                      their predicates, w and `c2 * w + c1 * (1 - w) <= m` uncontracted, evaluated in the reference's
 *                      order so that a later class overwrites an earlier one where predicates overlap
 *     high_mask      = local_max & (magnitude >= high),  low_mask = local_max & (magnitude >= low)
 *   One launch (canny_nms_kernel: a tile of `smoothed` with a halo of 2 in LDS -- one sample for Sobel, one for the neighbours'
 *   magnitudes; magnitudes outside the image are computed from reflected samples and never consulted, because `eroded` is
 *   false on the border ring).  After mi_debug_set_edges(.., 1): the Sobel responses by mi_correlate1d into pooled scratch
 *   arrays and two launches with one thread per pixel straight from global memory, the same bits.
 * mi_canny_threshold: the two masks alone from magnitude and local_max (use_quantiles: the thresholds come from the magnitude).
 * mi_masked_copy: out = mask ? image : 0 on arrays of any dtype (_canny.py:47-48: a copy, so NaN and negative samples under the
 *   mask leave no trace); out may be image.
 * mi_canny_normalize: out = double(smoothed) / (bleed_over + DBL_EPSILON) (_canny.py:50), the sum and the quotient rounded on
 *   their own; smoothed float32 / float64, bleed_over and out float64; out may be bleed_over (or smoothed, when float64). */
int mi_masked_copy(const mi_array *image, const mi_array *mask, const mi_array *out, mi_stream stream);
int mi_canny_normalize(const mi_array *smoothed, const mi_array *bleed_over, const mi_array *out, mi_stream stream);
int mi_canny_nms(const mi_array *smoothed, const mi_array *eroded, const mi_array *magnitude, const mi_array *local_max,
                 const mi_array *high_mask, const mi_array *low_mask, double high, double low, mi_stream stream);
int mi_canny_threshold(const mi_array *magnitude, const mi_array *local_max, const mi_array *high_mask, const mi_array *low_mask,
                       double high, double low, mi_stream stream);
int mi_edge_filter(const mi_array *image, const mi_array *out, const mi_array *mask, const double *weights, int naxes,
                   int magnitude, int mode, double cval, mi_stream stream);
int mi_edge_pair_magnitude(const mi_array *a, const mi_array *b, const mi_array *out, double divisor, mi_stream stream);
int mi_threshold_masks(const mi_array *image, const mi_array *low, const mi_array *high, double low_value, double high_value,
                       const mi_array *mask_low, const mi_array *mask_high, mi_stream stream);

/* skimage.feature.structure_tensor and the corner detectors (cupyimg/skimage/feature/corner.py:18-43, 125-136, 566-590, 658-671,
 * 728-743, 812-830; csrc/corners.hip).  image: C-contiguous float32 / float64 (T; other dtypes: MI_ERR_UNSUPPORTED with nothing
 * queued) of rank 1 .. 8.
 * mi_structure_products: out is a block of T with `rank` rows (products == 0) or rank (rank + 1) / 2 rows (products != 0) of
 *   image.size elements; its rows are contiguous and a whole number of elements apart (they may be padded).
 *     d_a  = scipy.ndimage.sobel(image, axis = a, mode, cval) in SciPy's own arithmetic: correlate1d with [-1, 0, 1] along a,
 *            then with [1, 2, 1] along every other axis in ascending order, every pass accumulated in double as
 *            x(l) * 0.0 + (x(l - 1) - x(l + 1)) * -1.0   or   d(l) * 2.0 + (d(l - 1) + d(l + 1)) * 1.0   (the `* 0.0` term stays: an
 *            infinite centre gives NaN) and rounded to T before the next pass reads it
 *     mode 'constant': every pass extends its own input line with the double cval, so an intermediate outside the array along the
 *            pass axis IS cval (this is not the Sobel filter of the cval-padded image); every other mode: the index map
 *     products == 0: row a = d_a;  products != 0: row e = d_i * d_j in T, (i, j) the e-th of combinations_with_replacement(axes, 2)
 *     reverse != 0 (2-D only, order 'xy'): the derivatives are reversed first
 *   Rank 2 and 3: one launch (st_fused_kernel: a box of the image with a one-sample halo in LDS, every axis's rounded passes from
 *   registers; the derivatives never exist in memory on the product route).  Other ranks, or after mi_debug_set_corners(.., 1):
 *   one st_pass_kernel launch per pass through pooled scratch arrays and st_product_kernel, the same bits.
 * mi_corner_response: one pointwise launch over elems, a (3, size) block Arr, Arc, Acc of T (kind 4: a (6, size) block imx, imy,
 *   imxx, imxy, imyx, imyy; row 4 is not read), rows as above; every operation in T, in the reference's order, rounded on its own:
 *     0 harris 'k':   detA = Arr * Acc; detA -= Arc * Arc; traceA = Arr + Acc; out0 = detA - (T(k) * traceA) * traceA
 *     1 harris 'eps': out0 = (2 * detA) / (traceA + T(eps))
 *     2 shi-tomasi:   out0 = (Arr + Acc) - sqrt((Arr - Acc)^2 + (4 * Arc) * Arc) / 2
 *     3 foerstner:    out0 = w = detA / traceA, out1 = q = (4 * detA) / (traceA * traceA) where traceA != 0, else 0 (float64 outputs)
 *     4 kitchen-rosenfeld: out0 = ((imxx * imy) * imy + (imyy * imx) * imx - ((2 * imxy) * imx) * imy) / (imx * imx + imy * imy)
 *                     where the denominator is not 0, else 0 (a float64 output)
 *   out0 (out1: kind 3 only, else NULL): C-contiguous, image.size elements, of T for kinds 0 .. 2 and float64 for 3 and 4.
 * Nothing synchronises and nothing is read by the host. */
int mi_structure_products(const mi_array *image, const mi_array *out, int products, int reverse, int mode, double cval, mi_stream stream);
int mi_corner_response(const mi_array *elems, const mi_array *out0, const mi_array *out1, int kind, double k, double eps, mi_stream stream);

/* skimage.feature.match_template (cupyimg/skimage/feature/template.py:125-205; csrc/template.hip): the normalised cross-correlation
 * of an image (rank 2) or a volume (rank 3) with a template of the same rank, one launch.
 *   image: C-contiguous uint8, uint16, int16, float32 or float64 (other dtypes: MI_ERR_UNSUPPORTED with nothing queued; the caller
 *   converts); tmpl: C-contiguous float64, 1 <= tmpl.shape[a] <= image.shape[a]; out: C-contiguous float64 of image.shape
 *   (pad_input != 0) or image.shape - tmpl.shape + 1.
 *   mode: the index map that numpy.pad's mode of the reference amounts to -- 'constant' MI_MODE_CONSTANT (cval), 'edge'
 *   MI_MODE_NEAREST, 'reflect' MI_MODE_MIRROR, 'symmetric' MI_MODE_REFLECT, 'wrap' MI_MODE_GRID_WRAP (MI_MODE_WRAP means the same) --
 *   applied as often as it takes: the template may be as long as the axis.
 *   Per axis the window of output index o starts at image index o - t / 2 (pad_input) or o, t = tmpl.shape[a].  Over the window,
 *   every sample converted to double first, every product and sum a double rounded on its own, the taps in raster order:
 *     x = x + I * T;   s1 = s1 + I;   s2 = s2 + I * I
 *     num = x - s1 * mean;   d = s2 - (s1 * s1) / V;   d = d * ssd;   d = d < 0 ? 0 : d (a NaN stays);   den = sqrt(d)
 *     out = den > DBL_EPSILON ? num / den : 0.0
 *   mean, ssd: the template's mean and sum of squared deviations from it, formed by the caller; V = tmpl.size.  A window that holds
 *   a NaN or an infinity gives 0.0.
 *   mt_fused_kernel stages a tile's windows in LDS and walks templates whose box does not fit in slabs; mt_generic_kernel (one thread
 *   per output, the same bits) runs after mi_debug_set_match_template(1) and for templates more than about 690 columns wide.
 * Nothing synchronises and nothing is read by the host. */
int mi_match_template(const mi_array *image, const mi_array *tmpl, const mi_array *out, int pad_input, int mode, double cval, double mean,
                      double ssd, mi_stream stream);

/* One iteration of Richardson-Lucy deconvolution (skimage.restoration.richardson_lucy; cupyimg/skimage/restoration/
 * deconvolution.py:356-416, where an iteration is two whole-array convolutions, a division, an optional where and a multiply;
 * csrc/richardson_lucy.hip).
 *   image, u_in, u_out: C-contiguous float32 or float64 arrays of one shape and dtype T, rank 1 to MI_MAX_NDIM (other dtypes:
 *   MI_ERR_UNSUPPORTED with nothing queued; the caller converts); u_out overlaps neither of the others.  psf: the point spread
 *   function, already rounded to T, as HOST doubles in C order, psf_shape[d] >= 1 samples along axis d (image.ndim entries).
 * With s = psf_shape, per axis, and every sample outside the image a 0 that is multiplied and added like any other:
 *     c[i]     = sum_k psf[k] * u_in[i + (s - 1) / 2 - k]      the taps in C order of the reversed PSF (t = s - 1 - k)
 *     r[i]     = image[i] / c[i];   r[i] = 0 where use_epsilon and c[i] < T(filter_epsilon)
 *     u_out[i] = u_in[i] * sum_j psf[j] * r[i - s / 2 + j]     the taps in C order of j
 *     clip:      u_out > 1 -> 1, u_out < -1 -> -1
 * Taps whose PSF value is 0.0 are skipped; every other product is formed and added in double from +0.0 and each sum is rounded
 * once to T (mi_correlate_nd's rule without acc_f32); the division and the last product are single operations in T; nothing is
 * guarded, NaN, infinities and a zero c propagate.
 *   Ranks 2 and 3: rl_fused_kernel, one launch, u and r in LDS rings streamed along axis 0, r never in memory; PSFs whose rings
 *   do not fit 64 KiB of LDS, the other ranks and mi_debug_set_richardson_lucy(1): rl_ratio_kernel + rl_update_kernel, two
 *   launches with r in scratch_dev (image.size elements of T; NULL: the call takes and returns a block of the pool itself).
 *   mi_richardson_lucy_needs_scratch says which of the two a call with this image and PSF shape takes now.
 * Nothing synchronises and nothing is read by the host. */
int mi_richardson_lucy_needs_scratch(const mi_array *image, const int64_t *psf_shape, int *needs_scratch);
int mi_richardson_lucy_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const double *psf, const int64_t *psf_shape,
                            double filter_epsilon, int use_epsilon, int clip, void *scratch_dev, mi_stream stream);

/* ------------------------------------------------------------------ */
/* K5: interpolation, spline order 0 and 1                              */
/* ------------------------------------------------------------------ */
/* coords: (ndim, *out.shape) C-contiguous f32 or f64
 * (interpolation.py:271-394, kernel _interp_kernels.py:595-621). */
int mi_map_coordinates(const mi_array *in, const mi_array *coords, const mi_array *out,
                       int order, int mode, double cval, mi_stream stream);

/* matrix: host doubles (ndim, ndim+1) row-major, c = M[:, :n] @ o + M[:, n]
 * (interpolation.py:397-561, kernel _interp_kernels.py:723-751; the diagonal
 * zoom+shift form :655-688 is the same entry point with a diagonal M). */
int mi_affine_transform(const mi_array *in, const mi_array *out, const double *matrix,
                        int order, int mode, double cval, mi_stream stream);

/* B-spline interpolation of order 2..5 (interpolation.py:105-268 spline_filter,
 * :271-561 map_coordinates / affine_transform with order > 1; kernels
 * _spline_prefilter_core.py, _spline_kernel_weights.py, _interp_kernels.py:473-549).
 * The caller builds the float64 coefficient array -- mi_spline_pad (copy of any
 * real dtype, extended by npad samples per side on every axis: pad_mode 0 edge
 * replication, 1 cval; SciPy pads by 12 for `nearest` / `grid-constant`, else 0.
 * The ring of pad_mode 1 holds cval CAST TO THE DTYPE OF `in` (C truncation for integers, != 0 for bool, rounded to
 * float32 for float32), as SciPy pads the image itself before it filters: -1000.3 is -1000 in an int16 image.  The
 * cval handed to mi_spline_map_coordinates / mi_spline_affine_transform, read beyond the ring, stays as given.)
 * followed by mi_spline_filter1d along every axis (spline_mode 0 mirror,
 * 1 reflect, 2 grid-wrap: reflect for reflect / nearest, grid-wrap for grid-wrap,
 * mirror otherwise) -- and interpolates it; coordinates refer to the unpadded
 * array.  Rank <= 8 (r3; float32 coefficients: rank <= 3).
 * spline_mode | 0x100 (mi_spline_filter1d, mi_spline_prefilter): only the kernels whose
 * arithmetic is SciPy's operation for operation (no blocked recursion) -- pass it when the
 * interpolated result will be rounded to an integer dtype, where the last bit of a
 * coefficient decides exact .5 ties.
 * r5 -- axes that hold SAMPLES.  An affine transform that maps an axis onto itself with an
 * integral shift evaluates the spline at the samples of that axis, where it returns them: the
 * prefilter pass along the axis and the taps along it cancel (SciPy's `rotate` filters the two
 * axes of the rotation plane only; the reference's `rotate`, interpolation.py:576-709, filters
 * all of them -- the results agree to rounding).  mi_spline_prefilter with
 * spline_mode | MI_SPLINE_SKIP_AXIS(d) leaves axis d unfiltered;
 * mi_spline_affine_transform with order | MI_SPLINE_SAMPLES_AXIS(d) interpolates such an array
 * (order 3, float32 coefficients, rank 3, ONE such axis: x -- `rotate` with the default axes --
 * or the axis the streaming kernel walks along) and answers MI_ERR_UNSUPPORTED when no kernel
 * evaluates the axis as a single tap: the caller then filters it after all
 * (mi_spline_filter1d; the passes commute) and calls again without the flag. */
#define MI_SPLINE_SKIP_AXIS(d) (0x200 << (d))
#define MI_SPLINE_SAMPLES_AXIS(d) (0x100 << (d))
int mi_spline_pad(const mi_array *in, const mi_array *out, int npad, int pad_mode, double cval,
                  mi_stream stream);
int mi_spline_filter1d(const mi_array *data, int axis, int order, int spline_mode, mi_stream stream);
/* mi_spline_pad followed by mi_spline_filter1d along every axis longer than one sample, in one call
 * (the loop of spline_filter, interpolation.py:185-268); without padding and conversion the first
 * pass reads `in` directly instead of copying it first.  pad_mode 1 fills the ring with cval cast to in's dtype
 * (see mi_spline_pad above).
 * Precision of the streaming passes (orders 2 / 3 on volumes of >= 16384 lines: the default route; r5 advisor
 * finding): the causal sweep's running values stay in the COEFFICIENT type between the two sweeps -- rounded to
 * float32 on the float32 route -- and a line starts from a 20-term truncated sum; the one-thread-per-line kernels
 * keep them in double.  Bound: 1 ulp of a float32 coefficient (the whole-volume order-3 tests hold 2e-5 against
 * SciPy's double); strided and contiguous axes round differently.  spline_mode | 0x100 (exact) selects the
 * double-state kernels. */
int mi_spline_prefilter(const mi_array *in, const mi_array *out, int order, int spline_mode, int npad,
                        int pad_mode, double cval, mi_stream stream);
int mi_spline_map_coordinates(const mi_array *coef, const mi_array *coords, const mi_array *out,
                              int order, int mode, double cval, int npad, mi_stream stream);
int mi_spline_affine_transform(const mi_array *coef, const mi_array *out, const double *matrix,
                               int order, int mode, double cval, int npad, mi_stream stream);

/* ------------------------------------------------------------------ */
/* multi-GPU: slab partition on axis 0, halo exchange over RCCL/xGMI    */
/* (new design; the reference is single-GPU)      */
/* ------------------------------------------------------------------ */
#define MI_UNIQUE_ID_BYTES 128
int mi_comm_unique_id(char id[MI_UNIQUE_ID_BYTES]);
int mi_comm_init_rank(mi_comm *comm, int nranks, int rank, const char id[MI_UNIQUE_ID_BYTES]);
int mi_comm_destroy(mi_comm comm);
/* Slab buffer layout on every rank: [lo halo planes][n local planes][hi halo planes],
 * plane_bytes each.  Sends the first `hi` / last `lo` local planes to the
 * previous / next rank and receives into the halo regions, all inside one
 * ncclGroupStart/End.  prev/next < 0 means no neighbour (global edge). */
int mi_halo_exchange(mi_comm comm, void *slab, size_t plane_bytes, int64_t n_local, int lo,
                     int hi, int prev_rank, int next_rank, mi_stream stream);

/* n point-to-point transfers in ONE RCCL group: ptrs[i] / nbytes[i] sent to (is_send[i] != 0) or received from rank
 * peers[i].  Between one pair of ranks the sends of one side must come in the order of the receives of the other
 * (RCCL matches them by order).  Used once per call by the output-sharded interpolation to fetch the input planes a
 * rank's output planes read (the pre-image slab) -- not a collective, nothing in a timed step. */
int mi_comm_sendrecv(mi_comm comm, int n, void *const ptrs[], const size_t nbytes[], const int peers[],
                     const int is_send[], mi_stream stream);

/* One filtering step of a slab rank: fused separable filter of the extended
 * slab [lo halo | local planes | hi halo] (a side without neighbour has no
 * halo planes) with the exchange overlapped:
 *   stream      : record input_free | interior planes ....... | wait halos_ready | edge planes
 *   comm_stream : wait input_free   | RCCL send/recv of halos | record halos_ready
 * overlap = 1 selects that schedule, 0 the plain one (exchange, then one
 * launch over all local planes, both on `stream`), -1 decides by halo size:
 * the two cross-stream waits and the extra launch cost ~20 us, so overlapping
 * pays from ~8 MiB of halo per direction.  Only the local planes of ext_out
 * are meaningful (kernels longer than 9 taps also overwrite its halo planes).  With overlap = 1, MI_ERR_UNSUPPORTED is returned before anything is
 * queued when the fused kernel does not take plane ranges for the request. */
int mi_slab_separable3d_f32(mi_comm comm, const mi_array *ext_in, const mi_array *ext_out,
                            const double *const weights[3], const int wlen[3], const int origin[3],
                            const int mode[3], double cval, int lo, int hi, int prev_rank, int next_rank,
                            int overlap, mi_stream comm_stream, mi_event input_free,
                            mi_event halos_ready, mi_stream stream);

/* r4 -- the pipelined slab schedule: `nbuf` (2 or 3; 1 = serial) resident input slabs per rank, one output slab.
 * The halo exchange of the NEXT input runs on an internal high-priority comm stream underneath the single launch that
 * filters the current one (steady state: step time = max(kernel, exchange); no split launch, no wait on the critical
 * path).  All slabs are extended buffers [lo halo | local planes | hi halo] of one shape.
 *   mi_slab_pipe_step(pipe, submit, compute): "input `submit` is final -- as of the work queued on `stream` so far --
 *       exchange its halos" and / or "filter input `compute` into the output slab" (-1 = nothing); a buffer must be
 *       submitted before it is computed;
 *   mi_slab_pipe_run(pipe, nsteps, use_graph): nsteps steps of the rotation 0, 1, .., nbuf-1, 0, .. with the
 *       submits nbuf-1 steps ahead (resident inputs: benchmarks, repeated filtering); use_graph > 0 replays a captured
 *       hipGraph of one rotation (or of `use_graph` steps, rounded down to whole rotations) where possible and queues
 *       directly otherwise;
 *   mi_slab_pipe_info: graph_state 0 not tried / 1 in use / -1 capture refused; planes_ok 0 = the kernel takes no plane
 *       ranges and filters the halo planes of the output too (scratch).
 * Every refusal (MI_ERR_UNSUPPORTED, argument errors) comes from mi_slab_pipe_create, before anything is queued. */
typedef void *mi_slab_pipe;
int mi_slab_pipe_create(mi_slab_pipe *pipe, mi_comm comm, int nbuf, const mi_array *const ext_in[],
                        const mi_array *ext_out, const double *const weights[3], const int wlen[3],
                        const int origin[3], const int mode[3], double cval, int lo, int hi, int prev_rank,
                        int next_rank, mi_stream stream);
int mi_slab_pipe_destroy(mi_slab_pipe pipe);
int mi_slab_pipe_step(mi_slab_pipe pipe, int submit, int compute);
int mi_slab_pipe_run(mi_slab_pipe pipe, int nsteps, int use_graph);
int mi_slab_pipe_info(mi_slab_pipe pipe, int *graph_state, int *graph_steps, int *planes_ok);

/* ---- selection, gather and sorting (csrc/select.hip): results whose size depends on the data.
 * Limits shared by the family: C-contiguous arrays of any real dtype except float16, at most 2^31 - 1 elements
 * (MI_ERR_UNSUPPORTED above, before anything is queued); empty inputs return MI_OK without a launch.  No kernel waits on
 * another workgroup and no output position depends on the order in which waves arrive: the results are reproducible bit for
 * bit.
 *
 * Compaction is a count call and a write call around one allocation of the caller's.  `work` is a 1-D uint8 array of at
 * least mi_select_work_bytes(a.size) bytes, uninitialised; the count call leaves the per-tile counts, their exclusive scan and
 * the total there, reads the total back into *total (the one synchronisation) and the write call, given the same array and
 * the same `work`, recomputes the predicate and scatters.  The predicate is "nonzero in the array's own dtype": NaN counts,
 * -0.0 does not.  layout 0: out is (K,) int64, the flat indices in raster order; 1: (K, ndim), the unravelled indices as rows
 * (argwhere); 2: (ndim, K), as columns (nonzero).  K = *total; a shorter `out` receives the first entries only. */
int mi_select_work_bytes(int64_t n, int64_t *bytes);
int mi_select_count(const mi_array *a, const mi_array *work, int64_t *total, mi_stream stream);
int mi_select_write(const mi_array *a, const mi_array *work, const mi_array *out, int layout, mi_stream stream);
/* out[k, :] = a[indices[k], :] with `a` seen as (a.size / inner, inner) and int64 indices (negative ones count from the end).
 * An index out of range sets *flag_dev (device int32, zeroed by the caller) to 1, reads nothing and stores 0. */
int mi_take(const mi_array *a, const mi_array *indices, const mi_array *out, int64_t inner, int32_t *flag_dev, mi_stream stream);
/* Stable argsort of a 1-D array: idx_out (int64) = numpy.argsort(a, kind="stable"), index for index; with `descending`
 * numpy.argsort(-a, kind="stable") (integers negate with wrap-around, as NumPy's do; bool negates logically).  -0.0 sorts
 * equal to +0.0 and every NaN last, in the original order.  sorted_out (the array's dtype) = a[idx_out].  Either output may be
 * NULL.  An LSD radix sort, 8 bits a pass (as many passes as the dtype has bytes), of (key, index) pairs between two pooled
 * buffers; a pass is a per-workgroup digit histogram, a scan and a stable scatter.  Nothing synchronises. */
int mi_argsort(const mi_array *a, const mi_array *idx_out, const mi_array *sorted_out, int descending, mi_stream stream);
/* Peak candidates of skimage.feature.peak_local_max (peak.py:37-71) through the same count / write pair: voxel i is a
 * candidate when image[i] == image_max[i] (skipped when image_max is NULL), image[i] > threshold -- compared in the image's
 * dtype for float32 / float64, in double for integers, as NumPy 2 evaluates `image > float(threshold)` -- and its index along
 * every axis d lies in [border[d], shape[d] - border[d]) (border NULL: none).  *n_equal = the number of voxels with
 * image == image_max (0 without image_max).  The write call stores the unravelled indices as (K, ndim) int64 rows in raster
 * order and the voxels' values as (K,) of the image's dtype.  No bool images. */
int mi_peak_count(const mi_array *image, const mi_array *image_max, double threshold, const int64_t *border, const mi_array *work,
                  int64_t *total, int64_t *n_equal, mi_stream stream);
int mi_peak_write(const mi_array *image, const mi_array *image_max, double threshold, const int64_t *border, const mi_array *work,
                  const mi_array *coords_out, const mi_array *values_out, mi_stream stream);
/* Greedy spacing (ensure_spacing of _shared/coord.py, the loop of corner.py:929-945) of K distinct points given in rank order
 * as (K, ndim) int64 rows.  mi_spacing_init zeroes `map` (int32, the image's shape), stores rank + 1 at every point and sets
 * status (K uint8) to 2 = live; *bad = 1 when a point lies outside the map (it is left out).  mi_spacing_rounds runs `nrounds`
 * rounds of two launches: a live point is kept (status 1) when no live point of lower rank conflicts with it, then live points
 * in conflict with a kept one are rejected (status 0); *live = 1 when a point was still live after the last round.  Two points
 * conflict when their distance is < spacing (inclusive 0) or <= spacing (inclusive 1), in exact integers: max |d| for p_norm
 * 0, sum |d| for 1, sum d^2 against spacing^2 for 2.  Rounds without live points change nothing.  Both calls synchronise
 * (one 4-byte read). */
int mi_spacing_init(const mi_array *coords, const mi_array *map, const mi_array *status, int *bad, mi_stream stream);
int mi_spacing_rounds(const mi_array *coords, const mi_array *map, const mi_array *status, int64_t spacing, int p_norm, int inclusive,
                      int nrounds, int *live, mi_stream stream);
/* out (bool, C-contiguous) = false everywhere, true at the (K, out.ndim) int64 points inside it */
int mi_scatter_true(const mi_array *coords, const mi_array *out, mi_stream stream);

/* ---- region tables of a label image (csrc/regionprops.hip): find_objects, regionprops, remove_small_objects.
 * Labels are C-contiguous int32 / int64; row r of every table belongs to label r + 1, the tables have max_label rows, and
 * labels <= 0 or above max_label belong to no region.  Every table is written in full by the call that fills it (pool memory
 * arrives dirty).  No kernel waits on another workgroup, and the number of launches does not depend on max_label.  Nothing
 * synchronises.
 *
 * mi_rp_extent: ext (int64, (max_label, 1 + 3 ndim)) = voxel count | smallest index per axis | largest index + 1 per axis |
 * sum of the indices per axis; a label no voxel carries has count 0 (its minima are then -1, its maxima 0).  Integer atomics: exact, reproducible.
 * Any rank from 1 to MI_MAX_NDIM. */
int mi_rp_extent(const mi_array *labels, const mi_array *ext, mi_stream stream);
/* mi_rp_moments (ranks 2 and 3): raw and / or central (float64, (max_label, 4^ndim), either may be NULL) = the moments up to
 * order 3 per axis, M[p][q][r] = sum w dz^p dy^q dx^r, in box coordinates (index - smallest index): raw about 0, central about
 * the region's centroid raw[1, 0, ..] / raw[0, 0, ..]; w = 1, or the intensity converted to double.  centres (float64,
 * (max_label, 2, ndim)) receives the box origin and that centroid.  Unweighted: one sweep serves both tables (the centroid
 * follows from ext).  Weighted: a sweep for raw, and one more for central, which needs raw.  Double atomics: exact while every
 * term and partial sum is an integer below 2^53, otherwise the last bits depend on the arrival order. */
int mi_rp_moments(const mi_array *labels, const mi_array *intensity, const mi_array *ext, const mi_array *raw, const mi_array *central,
                  const mi_array *centres, mi_stream stream);
/* mi_rp_finish: out (float64, (max_label, stride)) = the derived columns of skimage's RegionProperties in the reference's
 * operation order, for ndim 2 (stride 40) or 3 (stride 96): bbox_area, extent, equivalent_diameter, centroid[ndim],
 * local_centroid[ndim], moments_normalized[4^ndim], moments_hu[7], inertia_tensor[ndim^2], inertia_tensor_eigvals[ndim],
 * major_axis_length, minor_axis_length, eccentricity, orientation.  raw: the WEIGHTED raw table (the two centroids are then
 * the weighted ones), NULL for the unweighted columns; central NULL: the row is the short one, the columns before
 * moments_normalized only (stride 7 in 2-D, 9 in 3-D).  Rows of absent labels and the 2-D-only columns in 3-D are NaN. */
int mi_rp_finish(const mi_array *ext, int ndim, const mi_array *raw, const mi_array *central, const mi_array *out, mi_stream stream);
/* mi_rp_keep, mode 0: out = src where ext[label - 1, 0] >= min_size, else 0 (src and out of one element size; any dtype);
 * mode 1: out = (src == 0) as 0 / 1 (labels and ext unused); mode 2: out = !(ext[label - 1, 0] >= min_size) as 0 / 1. */
int mi_rp_keep(const mi_array *labels, const mi_array *src, const mi_array *ext, int64_t min_size, int mode, const mi_array *out,
               mi_stream stream);
/* mi_rp_crop (ranks 1 to 3): out, a C-contiguous box at `origin`, = (labels[box] == label) as bool, or with an intensity image
 * intensity[box] where that holds and 0 elsewhere, in the intensity's dtype. */
int mi_rp_crop(const mi_array *labels, const mi_array *intensity, int64_t label, const int64_t *origin, const mi_array *out,
               mi_stream stream);

/* ---- skimage.filters thresholding and the ordering operators of the array layer (csrc/threshold.hip, -ffp-contract=off)
 *
 * mi_window_mean_std (_mean_std, threshold_niblack, threshold_sauvola; cupyimg/skimage/filters/thresholding.py:1003-1179): the
 *   sums S of x and Q of x^2 over the window of window[d] (odd, >= 1) samples per axis centred on every sample, the image
 *   extended as numpy.pad(mode="reflect") extends it (period 2 (n - 1) per axis, an axis of one sample repeats it) by index
 *   arithmetic, then with n = prod(window), each operation rounded on its own:
 *     m = S / n;  g2 = Q / n;  s = sqrt(g2 - m m < 0 ? 0 : g2 - m m)
 *     kind 0: out0 = m, out1 = s;  kind 1: out0 = m - k s;  kind 2: out0 = m (1 + k (s / r - 1))      (out1 NULL for 1 and 2)
 *   image: any dtype but float16, C-contiguous, rank 1 to 8; outputs float64.  bool and the integers of 16 bits or fewer are
 *   summed in integer registers (exact); every other dtype as doubles, a window's terms added along the last axis first, each
 *   axis from its lowest index, every partial sum from 0 -- on every route, so the routes agree bit for bit.  Ranks 2 and 3:
 *   one launch of win_fused_kernel (a tile and its halo in LDS, sums axis by axis; volumes streamed plane by plane through a
 *   ring of per-plane sums); other ranks, a window of 2^31 / max|x| samples or more, or after mi_debug_set_threshold(.., 1):
 *   win_generic_kernel, one thread per output.  Nothing synchronises.
 * mi_li_sums (threshold_li, :751-759): over the finite samples x of a C-contiguous image, with y = x - shift (integers:
 *   x - shift_int in int64; floats: rounded to the image's dtype), result[0 .. 5] = count and sum of the y > threshold (y as a
 *   double), count and sum of the others, min x, max x.  Counts are int64; sums and extrema int64 for integer images (exact),
 *   double for float32 / float64.  Two launches (per-workgroup parts in a tree of fixed shape, then one workgroup over the
 *   parts in index order): the same bits on every run.  bool, uint64 and float16 are converted by the caller.  Synchronises.
 * mi_min_adjacent_diff: the smallest positive x[i + 1] - x[i] of a sorted 1-D array as a double (+inf: none); floats: of
 *   the samples shifted as above, non-finite ones skipped.  Synchronises.
 * mi_multiotsu_search (threshold_multiotsu, :1230-1341): cum_p / cum_s: nbins + 1 host doubles, the running sums from 0 of
 *   the normalised histogram p and of index * p.  Every strictly increasing tuple t_1 < .. < t_{classes-1} <= nbins - 2 is
 *   evaluated: the sum over the classes, from the lowest, of S_k^2 / P_k (differences of the tables; 0 where P_k = 0), in
 *   float64.  thresholds (host, classes - 1) = the tuple of the largest sum, the lexicographically smallest among equals,
 *   whatever order the workgroups finish in; best (may be NULL) = that sum.  classes 2 to 5, at most 2^34 tuples.  Synchronises.
 * mi_compare: out (bool) = a op b, op 0 >, 1 >=, 2 <, 3 <=; b an array of a's shape or NULL: then the scalar.  ctype is the
 *   common type the caller worked out as NumPy does: 0 integers, compared exactly across signedness (the scalar is
 *   scalar_hi 2^64 + scalar_lo - 2^64, scalar_hi 0 .. 2: two's complement with one more bit either way); 1 float32 (operands
 *   float32 holds exactly); 2 float64.  NaN compares false.  One launch; nothing synchronises. */
int mi_window_mean_std(const mi_array *image, const int *window, int kind, double k, double r, const mi_array *out0,
                       const mi_array *out1, mi_stream stream);
int mi_li_sums(const mi_array *image, double threshold, double shift, int64_t shift_int, void *result, mi_stream stream);
int mi_min_adjacent_diff(const mi_array *sorted, double shift, double *result, mi_stream stream);
int mi_multiotsu_search(const double *cum_p, const double *cum_s, int nbins, int classes, int64_t *thresholds, double *best,
                        mi_stream stream);
int mi_compare(int op, const mi_array *a, const mi_array *b, int ctype, double scalar, int scalar_hi, uint64_t scalar_lo,
               const mi_array *out, mi_stream stream);

/* ---- skimage.segmentation boundaries and relabelling, skimage.util.map_array, unique (csrc/segment.hip).  Integer compares
 * and integer atomic minima only: every result is the same bits on every run.  Nothing synchronises.
 *
 * mi_find_boundaries (find_boundaries, cupyimg/skimage/segmentation/boundaries.py:160-180): labels of any integer dtype or bool
 *   (bool as uint8), C-contiguous, rank 1 to 8; out bool.  N1(p): neighbours at city-block distance <= connectivity, N(p): the
 *   3^ndim window, both clamped to the array; MAX the dtype's largest value; g(v) = MAX where v == background, else v.
 *     mode 0 thick: some q in N1(p) has L[q] != L[p];  mode 1 inner: thick and L[p] != background;
 *     mode 2 outer: thick and (L[p] == background or max over N of L != min over N of g(L))
 *   has_background 0: the background is no value of the dtype (no voxel is background); else `background` holds its bits.
 *   Ranks 2 and 3: one launch on a core box plus halo in LDS; other ranks or mi_debug_set_boundaries(.., 1): one thread a voxel.
 * mi_find_boundaries_subpixel (:9-47): out has 2 s - 1 samples per axis.  An element with every coordinate even is false; any
 *   other is true when {MAX} + {0 if a coordinate is 0 or 2 s - 2} + {labels of the pixels its 3^ndim window covers: c / 2 along
 *   an even coordinate c, (c - 1) / 2 and (c + 1) / 2 along an odd one} has more than two distinct values.
 * mi_paint_boundaries (mark_boundaries, :249-252): image (M, N, 3) float32 / float64, boundaries (M, N) bool: the colour where
 *   the boundary is set; with outline_color, that colour where it is not but one of its 3 x 3 neighbours (clamped) is.
 * mi_map_array_table / mi_map_array_search (cupyimg/skimage/util/_map_array.py): out[i] = output_vals[j] for the lowest j with
 *   keys[j] == input[i], zero bits without one.  input and keys: one integer dtype; output_vals and out: one dtype of 1 to 8
 *   bytes.  Table: key_min is the smallest key as an order-preserving unsigned value (signed dtypes: the sign-extended value with
 *   bit 63 flipped), range = largest - smallest + 1; a table of range int32 from the pool is filled, set by atomicMin and gathered
 *   through (use_lds: each workgroup copies it to LDS first; range <= 16384).  Search: sorted_keys ascending, perm[k] the
 *   position of sorted_keys[k] in the caller's keys (a stable sort), output_vals in the caller's order.
 * mi_unique_heads: heads[i] = i == 0 or sorted[i] != sorted[i - 1] (bits).  mi_unique_counts: counts[k] = pos[k + 1] - pos[k],
 *   the last against n.  mi_unique_inverse: inverse[perm[i]] = (number of k with pos[k] <= i) - 1.
 * mi_join_key: key (int64) = mul * r1 + r2 for integer fields of one shape. */
int mi_find_boundaries(const mi_array *labels, int connectivity, int mode, int has_background, int64_t background, const mi_array *out,
                       mi_stream stream);
int mi_find_boundaries_subpixel(const mi_array *labels, const mi_array *out, mi_stream stream);
int mi_paint_boundaries(const mi_array *boundaries, const mi_array *image, const double *color, const double *outline_color, mi_stream stream);
int mi_map_array_table(const mi_array *input, const mi_array *keys, const mi_array *output_vals, const mi_array *out, uint64_t key_min,
                       int64_t range, int use_lds, mi_stream stream);
int mi_map_array_search(const mi_array *input, const mi_array *sorted_keys, const mi_array *perm, const mi_array *output_vals,
                        const mi_array *out, mi_stream stream);
int mi_unique_heads(const mi_array *sorted, const mi_array *heads, mi_stream stream);
int mi_unique_counts(const mi_array *pos, int64_t n, const mi_array *counts, mi_stream stream);
int mi_unique_inverse(const mi_array *pos, const mi_array *perm, const mi_array *inverse, mi_stream stream);
int mi_join_key(const mi_array *r1, const mi_array *r2, int64_t mul, const mi_array *key, mi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355IMG_H */
