// corners.hip -- skimage.feature.structure_tensor and the corner detectors built on it (corner_harris, corner_shi_tomasi,
// corner_foerstner, corner_kitchen_rosenfeld): the Sobel derivatives of every axis and their pairwise products as one launch,
// and one pointwise launch per detector response.
//
// Reference path replaced: cupyimg/skimage/feature/corner.py:18-43, 125-136 (per axis one ndi.sobel of `rank` 1-D passes, then
// one whole-array multiply per element) and corner.py:566-590, 658-671, 728-743, 812-830 (6 to 10 whole-array passes).
//
// T is the image dtype (float32 / float64); this file is compiled with -ffp-contract=off, every product and sum rounds on its
// own.  The contract (include/mi355img.h, tests/helpers/corner_ref.py) is scipy.ndimage.sobel's own arithmetic:
//     d_a   = the image after correlate1d with [-1, 0, 1] along a, then [1, 2, 1] along every other axis in ascending order
//     pass  = T( x(l) * 0.0 + (x(l - 1) - x(l + 1)) * -1.0 )   or   T( x(l) * 2.0 + (x(l - 1) + x(l + 1)) * 1.0 )  in double
//             (every pass is rounded to T before the next one reads it; the `* 0.0` term makes an infinite centre a NaN)
//     P_ij  = d_i * d_j in T, (i, j) in combinations_with_replacement(axes, 2), the axes reversed first for order 'xy'
// A pass extends ITS OWN input line: for every mode but 'constant' that is the index map of the mode, so a pass output outside
// the array equals the pass output at the mapped position and the 3^rank samples around a voxel, each coordinate mapped on
// its own, determine every pass.  For 'constant' the line is extended with the double cval itself: an intermediate outside
// the array ALONG THE PASS AXIS is cval, not a derivative of constants, so the kernel substitutes cval per pass from the
// voxel's coordinates.
//
// st_fused_kernel<T, RANK, PRODUCTS, CONST>: the box scaffolding of skimage_common.hpp.  A workgroup of 256 threads owns core
// boxes of t_z x t_y x t_x voxels (RANK 2: t_y x t_x pixels), stages each with a one-sample halo in LDS through the boundary map,
// then a wave takes rows of the box with its lanes along x: the 3^RANK samples go to registers once and serve the three (two)
// rounded passes of every axis.  It stores the RANK derivatives (PRODUCTS false) or the RANK (RANK + 1) / 2 products as
// full rows of one (n, size) block; on the product route the derivatives never exist in memory.  The planner's box is
// 8 x 8 x 64 (float64: 4 x 8 x 64) voxels, 32 x 64 pixels: at most 6600 (3960) staged elements, 26 (31) KiB of LDS.
//
// Every other rank, or after mi_debug_set_corners(.., 1): st_pass_kernel makes one 3-tap pass along one axis through pooled
// scratch arrays (mode and cval honoured per pass, as SciPy does), st_product_kernel forms the products: the same bits.
//
// corner_response_kernel<T, KIND, VEC>: one pointwise launch over the tensor elements Arr, Arc, Acc (Kitchen-Rosenfeld: imx, imy,
// imxx, imxy, imyy), 16-byte accesses where the rows are aligned, every operation in the order and dtype of corner.py.
#include "skimage_common.hpp"

namespace mi {

constexpr int kStNT = 256;
constexpr int kStLdsBytes = 32 * 1024;

static Knob g_st_small{0}, g_st_generic{0};

struct StParams : BoxDims {
    int mode;           // filter_mode()
    int reverse;        // order 'xy': the derivatives are taken last axis first
    double cval;
    int64_t ostride;    // elements between two rows of the output block
};

// SciPy's correlate1d on three samples, centre tap first, rounded to T: [-1, 0, 1] (antisymmetric) and [1, 2, 1] (symmetric)
template <typename T>
__device__ __forceinline__ T st_diff(double xm, double x0, double xp)
{
    double t = x0 * 0.0;
    t += (xm - xp) * -1.0;
    return (T)t;
}
template <typename T>
__device__ __forceinline__ T st_smooth(double xm, double x0, double xp)
{
    double t = x0 * 2.0;
    t += (xm + xp) * 1.0;
    return (T)t;
}

template <typename T, int RANK, bool PRODUCTS, bool CONST>
__global__ void __launch_bounds__(kStNT)
st_fused_kernel(const T *__restrict__ in, T *__restrict__ out, const StParams p, const int64_t nboxes)
{
    __shared__ T tile[kStLdsBytes / sizeof(T)];
    constexpr int KZ = RANK == 3 ? 3 : 1;
    const int ey = p.t[1] + 2, ex = p.t[2] + 2;         // rows and columns of the staged box
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t box = blockIdx.x; box < nboxes; box += gridDim.x) {
        int z0, y0, x0;
        box_origin(p, box, z0, y0, x0);
        stage_halo1_box<T, RANK, kStNT>(tile, in, p, p.mode, z0, y0, x0);
        __syncthreads();
        for (int row = wave; row < p.t[0] * p.t[1]; row += kStNT / 64) {
            const int cz = row / p.t[1], cy = row - cz * p.t[1];
            const int z = z0 + cz, y = y0 + cy;
            if (z >= p.n[0] || y >= p.n[1]) continue;
            for (int cx = lane; cx < p.t[2]; cx += 64) {
                const int x = x0 + cx;
                if (x >= p.n[2]) continue;
                double v[KZ][3][3];
#pragma unroll
                for (int kz = 0; kz < KZ; kz++)
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) v[kz][ky][kx] = (double)tile[((cz + kz) * ey + (cy + ky)) * ex + (cx + kx)];
                // 'constant': the neighbour below / above along an axis lies outside the array, the pass along that axis reads cval
                const bool lo0 = z == 0, hi0 = z == p.n[0] - 1, lo1 = y == 0, hi1 = y == p.n[1] - 1, lo2 = x == 0, hi2 = x == p.n[2] - 1;
                auto sub = [&](bool outside, double s) -> double {
                    if constexpr (CONST) return outside ? p.cval : s;
                    else return s;
                };
                T d[RANK], dd[3], s[3];
                if constexpr (RANK == 3) {
                    // axis 0: the difference along z, smoothed along y, then along x
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
#pragma unroll
                        for (int ky = 0; ky < 3; ky++) dd[ky] = st_diff<T>(sub(lo0, v[0][ky][kx]), v[1][ky][kx], sub(hi0, v[2][ky][kx]));
                        s[kx] = st_smooth<T>(sub(lo1, (double)dd[0]), (double)dd[1], sub(hi1, (double)dd[2]));
                    }
                    d[0] = st_smooth<T>(sub(lo2, (double)s[0]), (double)s[1], sub(hi2, (double)s[2]));
                    // axis 1: the difference along y, smoothed along z, then along x
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
#pragma unroll
                        for (int kz = 0; kz < 3; kz++) dd[kz] = st_diff<T>(sub(lo1, v[kz][0][kx]), v[kz][1][kx], sub(hi1, v[kz][2][kx]));
                        s[kx] = st_smooth<T>(sub(lo0, (double)dd[0]), (double)dd[1], sub(hi0, (double)dd[2]));
                    }
                    d[1] = st_smooth<T>(sub(lo2, (double)s[0]), (double)s[1], sub(hi2, (double)s[2]));
                    // axis 2: the difference along x, smoothed along z, then along y
#pragma unroll
                    for (int ky = 0; ky < 3; ky++) {
#pragma unroll
                        for (int kz = 0; kz < 3; kz++) dd[kz] = st_diff<T>(sub(lo2, v[kz][ky][0]), v[kz][ky][1], sub(hi2, v[kz][ky][2]));
                        s[ky] = st_smooth<T>(sub(lo0, (double)dd[0]), (double)dd[1], sub(hi0, (double)dd[2]));
                    }
                    d[2] = st_smooth<T>(sub(lo1, (double)s[0]), (double)s[1], sub(hi1, (double)s[2]));
                } else {
                    // axis 0: the difference along y, smoothed along x
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) dd[kx] = st_diff<T>(sub(lo1, v[0][0][kx]), v[0][1][kx], sub(hi1, v[0][2][kx]));
                    d[0] = st_smooth<T>(sub(lo2, (double)dd[0]), (double)dd[1], sub(hi2, (double)dd[2]));
                    // axis 1: the difference along x, smoothed along y
#pragma unroll
                    for (int ky = 0; ky < 3; ky++) dd[ky] = st_diff<T>(sub(lo2, v[0][ky][0]), v[0][ky][1], sub(hi2, v[0][ky][2]));
                    d[1] = st_smooth<T>(sub(lo1, (double)dd[0]), (double)dd[1], sub(hi1, (double)dd[2]));
                }
                if (p.reverse) {
#pragma unroll
                    for (int a = 0; a < RANK / 2; a++) {
                        const T h = d[a];
                        d[a] = d[RANK - 1 - a];
                        d[RANK - 1 - a] = h;
                    }
                }
                T *o = out + ((int64_t)z * p.n[1] + y) * p.n[2] + x;
                if constexpr (PRODUCTS) {
                    int e = 0;
#pragma unroll
                    for (int a = 0; a < RANK; a++)
#pragma unroll
                        for (int b = a; b < RANK; b++) o[(e++) * p.ostride] = d[a] * d[b];
                } else {
#pragma unroll
                    for (int a = 0; a < RANK; a++) o[a * p.ostride] = d[a];
                }
            }
        }
        __syncthreads();
    }
}

// one 3-tap pass along one axis of the array seen as (outer, n, inner): the antisymmetric or the symmetric form, the
// neighbours through the boundary map ('constant': the double cval), accumulated in double and rounded to T
template <typename T>
__global__ void __launch_bounds__(kStNT)
st_pass_kernel(const T *__restrict__ in, T *__restrict__ out, int64_t total, int64_t n, int64_t inner, int anti, int mode, double cval)
{
    for (int64_t i = (int64_t)blockIdx.x * kStNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kStNT) {
        const int64_t l = (i / inner) % n;
        const int64_t lm = bmap_near<int64_t>(l - 1, n, mode), lp = bmap_near<int64_t>(l + 1, n, mode);
        const double x0 = (double)in[i];
        const double xm = lm < 0 ? cval : (double)in[i + (lm - l) * inner];
        const double xp = lp < 0 ? cval : (double)in[i + (lp - l) * inner];
        out[i] = anti ? st_diff<T>(xm, x0, xp) : st_smooth<T>(xm, x0, xp);
    }
}

// out[e] = d[i] * d[j] in T for (i, j) in combinations_with_replacement(axes, 2); d: (rank, total), reversed for order 'xy'
template <typename T>
__global__ void __launch_bounds__(kStNT)
st_product_kernel(const T *__restrict__ d, T *__restrict__ out, int64_t total, int64_t ostride, int rank, int reverse)
{
    for (int64_t i = (int64_t)blockIdx.x * kStNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kStNT) {
        int e = 0;
        for (int a = 0; a < rank; a++) {
            const T da = d[(int64_t)(reverse ? rank - 1 - a : a) * total + i];
            for (int b = a; b < rank; b++) out[(e++) * ostride + i] = da * d[(int64_t)(reverse ? rank - 1 - b : b) * total + i];
        }
    }
}

// ------------------------------------------------------------------ the detector responses (corner.py), every operation in T
enum { kCrHarrisK = 0, kCrHarrisEps = 1, kCrShiTomasi = 2, kCrFoerstner = 3, kCrKitchenRosenfeld = 4 };

// r0 (and r1 for Foerstner) of one pixel; a .. e: Arr, Arc, Acc (Kitchen-Rosenfeld: imx, imy, imxx, imxy, imyy)
template <typename T, int KIND, typename O>
__device__ __forceinline__ void corner_point(T a, T b, T c, T d, T e, T k, T eps, O &r0, O &r1)
{
    if constexpr (KIND == kCrKitchenRosenfeld) {
        const T imx = a, imy = b, imxx = c, imxy = d, imyy = e;
        T num = imxx * imy;                 // corner.py:571-579
        num = num * imy;
        T tmp = imyy * imx;
        tmp = tmp * imx;
        num = num + tmp;
        tmp = T(2) * imxy;
        tmp = tmp * imx;
        tmp = tmp * imy;
        num = num - tmp;
        T den = imx * imx;                  // :582-583
        const T q = imy * imy;
        den = den + q;
        r0 = den != T(0) ? (O)(num / den) : O(0);           // :585-588
    } else if constexpr (KIND == kCrShiTomasi) {
        T tmp = a - c;                      // corner.py:733-741
        tmp = tmp * tmp;
        T tmp2 = T(4) * b;
        tmp2 = tmp2 * b;
        tmp = tmp + tmp2;
        tmp = sqrt_t<T>(tmp);
        tmp = tmp / T(2);
        T r = a + c;
        r = r - tmp;
        r0 = (O)r;
    } else {
        T det = a * c;                      // corner.py:661-664, 815-818
        const T q = b * b;
        det = det - q;
        const T trace = a + c;
        if constexpr (KIND == kCrHarrisK) {
            T t = k * trace;                // :667
            t = t * trace;
            r0 = (O)(det - t);
        } else if constexpr (KIND == kCrHarrisEps) {
            const T n2 = T(2) * det;        // :669
            const T de = trace + eps;
            r0 = (O)(n2 / de);
        } else {
            if (trace != T(0)) {            // :820-828
                r0 = (O)(det / trace);
                const T tsq = trace * trace;
                const T n4 = T(4) * det;
                r1 = (O)(n4 / tsq);
            } else {
                r0 = O(0);
                r1 = O(0);
            }
        }
    }
}

template <typename U, int N>
struct alignas(sizeof(U) * N > 16 ? 16 : sizeof(U) * N) StVec {
    U v[N];
};

template <typename T, int KIND, int VEC>
__global__ void __launch_bounds__(kStNT)
corner_response_kernel(const T *__restrict__ elems, int64_t stride, void *__restrict__ out0, void *__restrict__ out1, int64_t size, double k, double eps)
{
    using O = typename std::conditional<(KIND >= kCrFoerstner), double, T>::type;
    constexpr int NIN = KIND == kCrKitchenRosenfeld ? 5 : 3;
    const T kt = (T)k, et = (T)eps;
    const int64_t nvec = size / VEC;
    const int64_t gid = (int64_t)blockIdx.x * kStNT + threadIdx.x, gstride = (int64_t)gridDim.x * kStNT;
    for (int64_t i = gid; i < nvec; i += gstride) {
        StVec<T, VEC> a[5];
#pragma unroll
        for (int r = 0; r < NIN; r++) a[r] = *(const StVec<T, VEC> *)(elems + (int64_t)(r == 4 ? 5 : r) * stride + i * VEC);
        StVec<O, VEC> r0, r1;
#pragma unroll
        for (int l = 0; l < VEC; l++) {
            r1.v[l] = O(0);
            corner_point<T, KIND, O>(a[0].v[l], a[1].v[l], a[2].v[l], NIN == 5 ? a[3].v[l] : T(0), NIN == 5 ? a[4].v[l] : T(0), kt, et, r0.v[l], r1.v[l]);
        }
        *(StVec<O, VEC> *)((O *)out0 + i * VEC) = r0;
        if constexpr (KIND == kCrFoerstner) *(StVec<O, VEC> *)((O *)out1 + i * VEC) = r1;
    }
    if constexpr (VEC > 1) {
        for (int64_t i = nvec * VEC + gid; i < size; i += gstride) {
            O r0, r1 = O(0);
            corner_point<T, KIND, O>(elems[i], elems[stride + i], elems[2 * stride + i], NIN == 5 ? elems[3 * stride + i] : T(0),
                                     NIN == 5 ? elems[5 * stride + i] : T(0), kt, et, r0, r1);
            ((O *)out0)[i] = r0;
            if constexpr (KIND == kCrFoerstner) ((O *)out1)[i] = r1;
        }
    }
}

static int st_grid(int64_t n)
{
    return capped_grid(n, kStNT, 8192);
}

template <typename T, int RANK>
static int st_fused(const mi_array *image, T *out, int64_t ostride, int products, int reverse, int mode, double cval, hipStream_t s)
{
    StParams p;
    memset(&p, 0, sizeof(p));
    int64_t nboxes;
    const int rc = plan_halo1_box(image, g_st_small != 0, kStLdsBytes, &p, &nboxes);
    if (rc == MI_ERR_INTERNAL) set_error("structure_products: the staged box does not fit the kernel's LDS");
    if (rc) return rc;
    p.mode = mode;
    p.reverse = reverse;
    p.cval = cval;
    p.ostride = ostride;
    const int grid = box_grid(nboxes);
    const T *in = (const T *)image->data;
#define ST_LAUNCH(P, C) hipLaunchKernelGGL((st_fused_kernel<T, RANK, P, C>), dim3(grid), dim3(kStNT), 0, s, in, out, p, nboxes)
    if (products) {
        if (mode == MI_MODE_CONSTANT) ST_LAUNCH(true, true);
        else ST_LAUNCH(true, false);
    } else {
        if (mode == MI_MODE_CONSTANT) ST_LAUNCH(false, true);
        else ST_LAUNCH(false, false);
    }
#undef ST_LAUNCH
    MI_HIP(hipGetLastError());
    note_kernel("mi::st_fused_kernel<%s,%d,%s> grid=%d box=%dx%dx%d (one launch: staged box with a one-sample halo, every axis's "
                "rounded passes from registers)",
                sizeof(T) == 4 ? "float32" : "float64", RANK, products ? "products" : "derivatives", grid, p.t[0], p.t[1], p.t[2]);
    return MI_OK;
}

template <typename T>
static int st_generic(const mi_array *image, T *out, int64_t ostride, int products, int reverse, int mode, double cval, hipStream_t s)
{
    const int rank = image->ndim;
    const int64_t total = numel(image);
    // two arrays for the passes to alternate between and, on the product route, the derivatives of every axis
    void *scratch = nullptr;
    int rc;
    if ((rc = pool_alloc(&scratch, (size_t)(2 + (products ? rank : 0)) * (size_t)total * sizeof(T), s))) return rc;
    T *tmp[2] = {(T *)scratch, (T *)scratch + total};
    T *der = (T *)scratch + 2 * total;
    const int grid = st_grid(total);
    int launches = 0;
    for (int a = 0; a < rank; a++) {
        T *dest = products ? der + (int64_t)a * total : out + (int64_t)(reverse ? rank - 1 - a : a) * ostride;
        int axes[MI_MAX_NDIM], np = 0;
        axes[np++] = a;
        for (int b = 0; b < rank; b++)
            if (b != a) axes[np++] = b;
        const T *src = (const T *)image->data;
        for (int k = 0; k < np; k++) {
            T *dst = k == np - 1 ? dest : tmp[k & 1];
            int64_t inner = 1;
            for (int b = axes[k] + 1; b < rank; b++) inner *= image->shape[b];
            hipLaunchKernelGGL((st_pass_kernel<T>), dim3(grid), dim3(kStNT), 0, s, src, dst, total, image->shape[axes[k]], inner, (int)(k == 0), mode, cval);
            src = dst;
            launches++;
        }
    }
    if (products) hipLaunchKernelGGL((st_product_kernel<T>), dim3(grid), dim3(kStNT), 0, s, (const T *)der, out, total, ostride, rank, reverse);
    const hipError_t e = hipGetLastError();
    pool_free(scratch);
    MI_HIP(e);
    note_kernel("mi::st_generic<%s> grid=%d %s rank %d (%d st_pass_kernel launches%s)", sizeof(T) == 4 ? "float32" : "float64", grid,
                products ? "products" : "derivatives", rank, launches, products ? ", st_product_kernel" : "");
    return MI_OK;
}

template <typename T>
static int st_dispatch(const mi_array *image, T *out, int64_t ostride, int products, int reverse, int mode, double cval, hipStream_t s)
{
    if (!g_st_generic && (image->ndim == 2 || image->ndim == 3)) {
        const int rc = image->ndim == 3 ? st_fused<T, 3>(image, out, ostride, products, reverse, mode, cval, s)
                                        : st_fused<T, 2>(image, out, ostride, products, reverse, mode, cval, s);
        if (rc != MI_ERR_UNSUPPORTED) return rc;
    }
    return st_generic<T>(image, out, ostride, products, reverse, mode, cval, s);
}

// a (rows, size) block whose rows are contiguous and a whole number of elements apart
static bool is_row_block(const mi_array *a, int64_t rows, int64_t size)
{
    const int64_t item = (int64_t)dtype_size(a->dtype);
    if (a->ndim != 2 || a->shape[0] != rows || a->shape[1] != size) return false;
    if (size > 1 && a->strides[1] != item) return false;
    return rows == 1 || (a->strides[0] % item == 0 && a->strides[0] >= size * item);
}

static bool ranges_overlap(const void *a, int64_t abytes, const void *b, int64_t bbytes)
{
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

template <typename T, int KIND>
static int cr_launch(const mi_array *elems, void *out0, void *out1, int64_t size, double k, double eps, hipStream_t s, const char *kind)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const int64_t stride = elems->shape[0] > 1 ? elems->strides[0] / (int64_t)sizeof(T) : size;
    const bool aligned = !((uintptr_t)elems->data & 15) && !((uintptr_t)out0 & 15) && !((uintptr_t)out1 & 15) && (stride * (int64_t)sizeof(T)) % 16 == 0;
    const int grid = st_grid(aligned ? (size + VEC - 1) / VEC : size);
    if (aligned)
        hipLaunchKernelGGL((corner_response_kernel<T, KIND, VEC>), dim3(grid), dim3(kStNT), 0, s, (const T *)elems->data, stride, out0, out1, size, k, eps);
    else
        hipLaunchKernelGGL((corner_response_kernel<T, KIND, 1>), dim3(grid), dim3(kStNT), 0, s, (const T *)elems->data, stride, out0, out1, size, k, eps);
    MI_HIP(hipGetLastError());
    note_kernel("mi::corner_response_kernel<%s,%s> grid=%d vec=%d (one pointwise launch)", sizeof(T) == 4 ? "float32" : "float64", kind, grid,
                aligned ? VEC : 1);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_corners(int small_tiles, int force_generic)
{
    g_st_small = small_tiles != 0;
    g_st_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_structure_products(const mi_array *image, const mi_array *out, int products, int reverse, int mode, double cval, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(out, "out"))) return rc;
    const int rank = image->ndim;
    MI_REQUIRE(rank >= 1, MI_ERR_INVALID_ARG, "structure_products: arrays of rank 1 to 8");
    if (image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("structure_products: float32 and float64 images only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    const int64_t total = numel(image);
    const int64_t rows = products ? (int64_t)rank * (rank + 1) / 2 : rank;
    MI_REQUIRE(out->dtype == image->dtype && is_row_block(out, rows, total), MI_ERR_INVALID_ARG,
               "structure_products: the output is a (rank or rank (rank + 1) / 2, image.size) block of the image's dtype with contiguous rows");
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "structure_products needs a C-contiguous image");
    MI_REQUIRE(!reverse || rank == 2, MI_ERR_INVALID_ARG, "structure_products: the reversed order is for 2-D images only");
    MI_REQUIRE(mode >= MI_MODE_REFLECT && mode <= MI_MODE_GRID_CONSTANT, MI_ERR_INVALID_ARG, "structure_products: unknown mode");
    if (total == 0) return MI_OK;
    const int64_t item = (int64_t)dtype_size(image->dtype);
    const int64_t ostride = rows > 1 ? out->strides[0] / item : total;
    MI_REQUIRE(!ranges_overlap(image->data, total * item, out->data, ((rows - 1) * ostride + total) * item), MI_ERR_INVALID_ARG,
               "structure_products: the output may not share memory with the image");
    mode = filter_mode(mode);
    hipStream_t s = resolve_stream(stream);
    if (image->dtype == MI_F32) return st_dispatch<float>(image, (float *)out->data, ostride, products != 0, reverse != 0, mode, cval, s);
    return st_dispatch<double>(image, (double *)out->data, ostride, products != 0, reverse != 0, mode, cval, s);
}

extern "C" int mi_corner_response(const mi_array *elems, const mi_array *out0, const mi_array *out1, int kind, double k, double eps, mi_stream stream)
{
    int rc;
    if ((rc = check_array(elems, "elems")) || (rc = check_array(out0, "out0"))) return rc;
    MI_REQUIRE(kind >= kCrHarrisK && kind <= kCrKitchenRosenfeld, MI_ERR_INVALID_ARG, "corner_response: unknown detector");
    MI_REQUIRE((out1 != nullptr) == (kind == kCrFoerstner), MI_ERR_INVALID_ARG, "corner_response: a second output for Foerstner's detector only");
    if (out1 && (rc = check_array(out1, "out1"))) return rc;
    if (elems->dtype != MI_F32 && elems->dtype != MI_F64) {
        set_error("corner_response: float32 and float64 elements only");
        return MI_ERR_UNSUPPORTED;
    }
    const int64_t size = numel(out0);
    MI_REQUIRE(is_row_block(elems, kind == kCrKitchenRosenfeld ? 6 : 3, size), MI_ERR_INVALID_ARG,
               "corner_response: the elements are a (3, size) block (Kitchen-Rosenfeld: (6, size)) with contiguous rows");
    const int odt = kind >= kCrFoerstner ? (int)MI_F64 : (int)elems->dtype;
    for (const mi_array *o : {out0, out1})
        MI_REQUIRE(!o || (o->dtype == odt && numel(o) == size && is_contiguous(o)), MI_ERR_INVALID_ARG,
                   "corner_response: C-contiguous outputs of the image's size, float64 for Foerstner and Kitchen-Rosenfeld, else of the elements' dtype");
    if (size == 0) return MI_OK;
    const int64_t item = (int64_t)dtype_size(elems->dtype), oitem = (int64_t)dtype_size(odt);
    const int64_t ebytes = ((elems->shape[0] - 1) * (elems->strides[0] / item) + size) * item;
    MI_REQUIRE(!ranges_overlap(elems->data, ebytes, out0->data, size * oitem) && (!out1 || (!ranges_overlap(elems->data, ebytes, out1->data, size * oitem) &&
               !ranges_overlap(out0->data, size * oitem, out1->data, size * oitem))), MI_ERR_INVALID_ARG,
               "corner_response: the outputs may not share memory with the elements or each other");
    hipStream_t s = resolve_stream(stream);
    void *o0 = out0->data, *o1 = out1 ? out1->data : nullptr;
    const bool f32 = elems->dtype == MI_F32;
#define CR_CASE(KIND, NAME) \
    case KIND: return f32 ? cr_launch<float, KIND>(elems, o0, o1, size, k, eps, s, NAME) : cr_launch<double, KIND>(elems, o0, o1, size, k, eps, s, NAME)
    switch (kind) {
    CR_CASE(kCrHarrisK, "harris_k");
    CR_CASE(kCrHarrisEps, "harris_eps");
    CR_CASE(kCrShiTomasi, "shi_tomasi");
    CR_CASE(kCrFoerstner, "foerstner");
    default: break;
    }
    return f32 ? cr_launch<float, kCrKitchenRosenfeld>(elems, o0, o1, size, k, eps, s, "kitchen_rosenfeld")
               : cr_launch<double, kCrKitchenRosenfeld>(elems, o0, o1, size, k, eps, s, "kitchen_rosenfeld");
#undef CR_CASE
}
