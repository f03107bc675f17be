// edges.hip -- the n-D edge operators of skimage.filters (sobel, scharr, prewitt: magnitude and single axis) as one launch, and
// the two threshold masks of apply_hysteresis_threshold.
//
// Reference path replaced: cupyimg/skimage/filters/edges.py:128-200 (_generic_edge_filter), which runs a 3-D magnitude as
// three dense 3 x 3 x 3 convolutions plus seven whole-array passes on a zeroed float64 volume, and edges.py:55-65 (the mask).
//
// T is the image dtype (float32 / float64); this file is compiled with -ffp-contract=off, every product and sum rounds on
// its own.  W_a: the dense 3^rank weights of edge axis a in correlation form (the caller flips the convolution kernel), C
// order.  For one output voxel q:
//     r_a   = T( sum over the taps k with W_a[k] != 0, in C order, from 0.0:  double(x(q + k - 1)) * W_a[k] )
//             (scipy.ndimage's NI_Correlate: a double accumulator that starts at 0, zero weights skipped, then the cast;
//              outside the array x is the mode's sample, for 'constant' the double cval itself)
//     out   = 0.0;  for a in the requested axes, in order:  out = out + double(magnitude ? r_a * r_a : r_a)   (the square in T)
//     magnitude:  out = out / ndim;  out = sqrt(out)
//     mask:       out = out * double(mask(q))      (mask: the eroded mask as bytes; -x * 0 = -0.0, NaN * 0 = NaN)
// (edges.py:180 starts `output` as float64 zeros and adds into it: a single-axis response of -0.0 comes out as +0.0.)
//
// edge_fused_kernel<T, RANK, CONST, FMA>: a workgroup of 256 threads owns core boxes of t_z x t_y x t_x voxels (RANK 2: t_y x t_x
// pixels), one after the other.  It stages the box plus one sample either way in LDS, every staged index resolved through the
// boundary map of the mode (no padded copy exists; CONST: mode 'constant', out-of-range samples are replaced by cval at the
// tap), then a wave takes rows of the box with its lanes along x: the 3^RANK samples go to registers once and serve every
// edge axis.  The per-axis responses never exist in memory.  The planner's box is 8 x 8 x 64 (float64: 4 x 8 x 64) voxels,
// 32 x 64 pixels: at most 6600 (3960) staged elements, 26 (31) KiB of LDS, five workgroups a CU.
//
// Ranks 1 and >= 4, or after mi_debug_set_edges(.., 1): the same arithmetic as one mi_correlate_nd per edge axis into a
// scratch array of T, edge_accumulate_kernel after each and edge_finish_kernel at the end (one thread per voxel).
#include "skimage_common.hpp"

namespace mi {

constexpr int kEdNT = 256;
constexpr int kEdLdsBytes = 32 * 1024;

static Knob g_ed_small{0}, g_ed_generic{0};

struct EdParams : BoxDims {
    int na;             // edge axes
    int edim[3];        // per edge axis: the axis (0 .. 2 of nz, ny, nx) whose centre plane holds the zero weights
    int magnitude;
    int mode;           // filter_mode()
    double cval;
    double ndim;
    double w[3][27];    // per edge axis: 3^RANK weights, correlation form, C order
};

// The response of one edge axis before the cast: the taps in C order from 0.0, the centre plane along axis E (the zero
// weights: [1, 0, -1] has its zero there) left out at compile time.  FMA: the products are exact (float32 samples times
// weights that are float32 values: 48 bits), so the fused multiply-add rounds what the separate product and sum round.
template <int NTAP, int E, bool FMA>
__device__ __forceinline__ double edge_response(const double (&v)[NTAP], const double *__restrict__ w)
{
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NTAP; k++) {
        const int i = E == 0 ? k / 9 : (E == 1 ? (k / 3) % 3 : k % 3);
        if (i == 1) continue;
        if constexpr (FMA) acc = __builtin_fma(v[k], w[k], acc);
        else acc += v[k] * w[k];
    }
    return acc;
}

template <typename T, int RANK, bool CONST, bool FMA>
__global__ void __launch_bounds__(kEdNT)
edge_fused_kernel(const T *__restrict__ in, const uint8_t *__restrict__ mask, double *__restrict__ out, const EdParams p, const int64_t nboxes)
{
    __shared__ T tile[kEdLdsBytes / sizeof(T)];
    constexpr int HZ = RANK == 3 ? 1 : 0;
    constexpr int KZ = RANK == 3 ? 3 : 1;
    constexpr int NTAP = KZ * 9;
    const int ey = p.t[1] + 2, ex = p.t[2] + 2;         // rows and columns of the staged box
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t box = blockIdx.x; box < nboxes; box += gridDim.x) {
        int z0, y0, x0;
        box_origin(p, box, z0, y0, x0);
        stage_halo1_box<T, RANK, kEdNT>(tile, in, p, p.mode, z0, y0, x0);
        __syncthreads();
        for (int row = wave; row < p.t[0] * p.t[1]; row += kEdNT / 64) {
            const int cz = row / p.t[1], cy = row - cz * p.t[1];
            const int z = z0 + cz, y = y0 + cy;
            if (z >= p.n[0] || y >= p.n[1]) continue;
            for (int cx = lane; cx < p.t[2]; cx += 64) {
                const int x = x0 + cx;
                if (x >= p.n[2]) continue;
                double v[NTAP];
#pragma unroll
                for (int kz = 0; kz < KZ; kz++)
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) {
                            double s = (double)tile[((cz + kz) * ey + (cy + ky)) * ex + (cx + kx)];
                            if constexpr (CONST) {
                                const int qz = z + kz - HZ, qy = y + ky - 1, qx = x + kx - 1;
                                if (qz < 0 || qz >= p.n[0] || qy < 0 || qy >= p.n[1] || qx < 0 || qx >= p.n[2]) s = p.cval;
                            }
                            v[(kz * 3 + ky) * 3 + kx] = s;
                        }
                double o = 0.0;
                for (int a = 0; a < p.na; a++) {
                    double acc;
                    if (RANK == 3 && p.edim[a] == 0) acc = edge_response<NTAP, 0, FMA>(v, p.w[a]);
                    else if (p.edim[a] == 1) acc = edge_response<NTAP, 1, FMA>(v, p.w[a]);
                    else acc = edge_response<NTAP, 2, FMA>(v, p.w[a]);
                    const T r = (T)acc;
                    o = o + (double)(p.magnitude ? r * r : r);
                }
                if (p.magnitude) {
                    o = o / p.ndim;
                    o = __builtin_sqrt(o);
                }
                const int64_t i = ((int64_t)z * p.n[1] + y) * p.n[2] + x;
                if (mask) o = o * (double)(mask[i] != 0);
                out[i] = o;
            }
        }
        __syncthreads();
    }
}

// out = (first ? 0.0 : out) + double(square ? r * r : r), the square in T
template <typename T>
__global__ void __launch_bounds__(kEdNT)
edge_accumulate_kernel(const T *__restrict__ resp, double *__restrict__ out, int64_t total, int first, int square)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        const T r = resp[i];
        const double o = first ? 0.0 : out[i];
        out[i] = o + (double)(square ? r * r : r);
    }
}

__global__ void __launch_bounds__(kEdNT)
edge_finish_kernel(double *__restrict__ out, const uint8_t *__restrict__ mask, int64_t total, int magnitude, double ndim)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        double o = out[i];
        if (magnitude) {
            o = o / ndim;
            o = __builtin_sqrt(o);
        }
        if (mask) o = o * (double)(mask[i] != 0);
        out[i] = o;
    }
}

// out = sqrt(a * a + b * b) / T(divisor), every operation in T and rounded on its own (roberts, farid: edges.py:599-611, 759-769)
template <typename T>
__global__ void __launch_bounds__(kEdNT)
edge_pair_kernel(const T *__restrict__ a, const T *__restrict__ b, T *__restrict__ out, int64_t total, T divisor)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        const T p = a[i] * a[i];
        T q = b[i] * b[i];
        q = q + p;
        q = sqrt_t<T>(q);
        out[i] = q / divisor;
    }
}

// mask_low = image > min(low, high), mask_high = image > high, every operand as a double (exact for every dtype up to 32-bit integers
// and float64); low / high: per-voxel float64 arrays or, where the pointer is NULL, the scalar
__global__ void __launch_bounds__(kEdNT)
threshold_masks_kernel(const void *__restrict__ image, int dtype, const double *__restrict__ low_a, const double *__restrict__ high_a,
                       double low_s, double high_s, uint8_t *__restrict__ mask_low, uint8_t *__restrict__ mask_high, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        const double v = load_as_f64(image, i, dtype);
        const double hi = high_a ? high_a[i] : high_s;
        double lo = low_a ? low_a[i] : low_s;
        if (lo > hi || hi != hi) lo = hi;                  // numpy.clip(low, None, high): the smaller one, a NaN of either stays
        mask_low[i] = (uint8_t)(v > lo);
        mask_high[i] = (uint8_t)(v > hi);
    }
}

static int ed_grid(int64_t n)
{
    return capped_grid(n, kEdNT, 8192);
}

template <typename T, int RANK, bool FMA>
static int ed_launch(const mi_array *image, const uint8_t *mask, double *out, const EdParams &p, int64_t nboxes, hipStream_t s)
{
    const int grid = box_grid(nboxes);
    if (p.mode == MI_MODE_CONSTANT)
        hipLaunchKernelGGL((edge_fused_kernel<T, RANK, true, FMA>), dim3(grid), dim3(kEdNT), 0, s, (const T *)image->data, mask, out, p, nboxes);
    else
        hipLaunchKernelGGL((edge_fused_kernel<T, RANK, false, FMA>), dim3(grid), dim3(kEdNT), 0, s, (const T *)image->data, mask, out, p, nboxes);
    MI_HIP(hipGetLastError());
    note_kernel("mi::edge_fused_kernel<%s,%d> grid=%d box=%dx%dx%d axes=%d %s%s (one launch: staged box with a one-sample halo, "
                "every edge axis from registers)",
                sizeof(T) == 4 ? "float32" : "float64", RANK, grid, p.t[0], p.t[1], p.t[2], p.na, p.magnitude ? "magnitude" : "signed",
                FMA ? " fma" : "");
    return MI_OK;
}

static int ed_fused(const mi_array *image, const uint8_t *mask, double *out, const double *weights, int naxes, int magnitude,
                    int mode, double cval, hipStream_t s)
{
    const int rank = image->ndim;
    const bool f32 = image->dtype == MI_F32;
    EdParams p;
    memset(&p, 0, sizeof(p));
    const int ntap = rank == 3 ? 27 : 9;
    int64_t nboxes;
    if (const int rc = plan_halo1_box(image, g_ed_small != 0, kEdLdsBytes, &p, &nboxes)) return rc;
    p.na = naxes;
    p.magnitude = magnitude;
    p.mode = mode;
    p.cval = cval;
    p.ndim = (double)rank;
    // the kernel leaves the zero weights out at compile time: they must be the centre plane along one axis, and nothing else
    // (true of [1, 0, -1] times non-zero smoothing weights); other weights take the unfused route
    bool exact = f32 && (mode != MI_MODE_CONSTANT || (double)(float)cval == cval);
    for (int a = 0; a < naxes; a++) {
        p.edim[a] = -1;
        for (int e = 3 - rank; e < 3 && p.edim[a] < 0; e++) {
            bool fits = true;
            for (int k = 0; k < ntap && fits; k++) {
                const int i = e == 0 ? k / 9 : (e == 1 ? (k / 3) % 3 : k % 3);
                fits = (weights[a * ntap + k] == 0.0) == (i == 1);
            }
            if (fits) p.edim[a] = e;
        }
        if (p.edim[a] < 0) return MI_ERR_UNSUPPORTED;
        for (int k = 0; k < ntap; k++) {
            p.w[a][k] = weights[a * ntap + k];
            exact = exact && (double)(float)p.w[a][k] == p.w[a][k];
        }
    }
    if (rank == 3) {
        if (exact) return ed_launch<float, 3, true>(image, mask, out, p, nboxes, s);
        return f32 ? ed_launch<float, 3, false>(image, mask, out, p, nboxes, s) : ed_launch<double, 3, false>(image, mask, out, p, nboxes, s);
    }
    if (exact) return ed_launch<float, 2, true>(image, mask, out, p, nboxes, s);
    return f32 ? ed_launch<float, 2, false>(image, mask, out, p, nboxes, s) : ed_launch<double, 2, false>(image, mask, out, p, nboxes, s);
}

// ------------------------------------------------------------------ the Canny stage (_canny.py:191-288), float64
// The class test of one pixel: i, j its Sobel responses, m its magnitude, M(dy, dx) the magnitude of a neighbour.  The four
// classes in the reference's order; where the predicates overlap (ties such as |i| == |j|, zeros) the last one that holds
// decides, as the reference's successive `local_maxima[pts] = ...` do.
template <typename F>
__device__ __forceinline__ bool canny_is_max(double i, double j, double m, F M)
{
    const double ai = __builtin_fabs(i), aj = __builtin_fabs(j);
    const bool same = (i >= 0 && j >= 0) || (i <= 0 && j <= 0);
    const bool opposite = (i <= 0 && j >= 0) || (i >= 0 && j <= 0);
    bool lm = false;
    if (same && ai >= aj) {                         // 0 .. 45 degrees (_canny.py:212-227)
        const double w = aj / ai;
        const bool plus = M(1, 1) * w + M(1, 0) * (1 - w) <= m;
        const bool minus = M(-1, -1) * w + M(-1, 0) * (1 - w) <= m;
        lm = plus && minus;
    }
    if (same && ai <= aj) {                         // 45 .. 90 degrees (:231-243)
        const double w = ai / aj;
        const bool plus = M(1, 1) * w + M(0, 1) * (1 - w) <= m;
        const bool minus = M(-1, -1) * w + M(0, -1) * (1 - w) <= m;
        lm = plus && minus;
    }
    if (opposite && ai <= aj) {                     // 90 .. 135 degrees (:247-259)
        const double w = ai / aj;
        const bool plus = M(-1, 1) * w + M(0, 1) * (1.0 - w) <= m;
        const bool minus = M(1, -1) * w + M(0, -1) * (1.0 - w) <= m;
        lm = plus && minus;
    }
    if (opposite && ai >= aj) {                     // 135 .. 180 degrees (:263-275)
        const double w = aj / ai;
        const bool plus = M(-1, 1) * w + M(-1, 0) * (1 - w) <= m;
        const bool minus = M(1, -1) * w + M(1, 0) * (1 - w) <= m;
        lm = plus && minus;
    }
    return lm;
}

// SciPy's correlate1d on three samples: [-1, 0, 1] (antisymmetric) and [1, 2, 1] (symmetric), centre tap first
__device__ __forceinline__ double canny_diff(double xm, double x0, double xp)
{
    double t = x0 * 0.0;
    t += (xm - xp) * -1.0;
    return t;
}
__device__ __forceinline__ double canny_smooth(double xm, double x0, double xp)
{
    double t = x0 * 2.0;
    t += (xm + xp) * 1.0;
    return t;
}

struct CnParams {
    int ny, nx;
    int ty, tx;         // the core tile
    int nty, ntx;
};

constexpr int kCnMaxTy = 16, kCnMaxTx = 64;

// A workgroup owns core tiles of ty x tx pixels.  S: the smoothed image on the tile plus 2 pixels either way, every index through
// the 'reflect' map; I, J, M: the Sobel responses and the magnitude on the tile plus 1 pixel either way.  A magnitude outside
// the image (from reflected samples) is never consulted: the reference pairs `pts[:-1]` with `magnitude[1:]` and so on
// (_canny.py:219-274), which only drops border pixels of pts, and pts is false there because binary_erosion with
// border_value = 0 clears the border ring of the eroded mask (_canny.py:201-203).
__global__ void __launch_bounds__(kEdNT)
canny_nms_kernel(const double *__restrict__ smoothed, const uint8_t *__restrict__ eroded, double *__restrict__ magnitude,
                 uint8_t *__restrict__ local_max, uint8_t *__restrict__ high_mask, uint8_t *__restrict__ low_mask, const double high,
                 const double low, const CnParams p, const int64_t ntiles)
{
    __shared__ double S[(kCnMaxTy + 4) * (kCnMaxTx + 4)];
    __shared__ double I[(kCnMaxTy + 2) * (kCnMaxTx + 2)], J[(kCnMaxTy + 2) * (kCnMaxTx + 2)], M[(kCnMaxTy + 2) * (kCnMaxTx + 2)];
    const int sy = p.ty + 4, sx = p.tx + 4, my = p.ty + 2, mx = p.tx + 2;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int y0 = (int)(tile / p.ntx) * p.ty, x0 = (int)(tile % p.ntx) * p.tx;
        for (int e = threadIdx.x; e < sy * sx; e += kEdNT) {
            const int r = e / sx, c = e - r * sx;
            const int gy = bmap_near<int>(y0 + r - 2, p.ny, MI_MODE_REFLECT), gx = bmap_near<int>(x0 + c - 2, p.nx, MI_MODE_REFLECT);
            S[e] = smoothed[(int64_t)gy * p.nx + gx];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < my * mx; e += kEdNT) {
            const int r = e / mx, c = e - r * mx;             // S index of this pixel: (r + 1, c + 1)
            double d[3];
            // isobel: the difference along y of the three columns, smoothed along x
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = canny_diff(S[r * sx + c + k], S[(r + 1) * sx + c + k], S[(r + 2) * sx + c + k]);
            const double is = canny_smooth(d[0], d[1], d[2]);
            // jsobel: the difference along x of the three rows, smoothed along y
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = canny_diff(S[(r + k) * sx + c], S[(r + k) * sx + c + 1], S[(r + k) * sx + c + 2]);
            const double js = canny_smooth(d[0], d[1], d[2]);
            double q = is * is;
            const double q2 = js * js;
            q = q + q2;
            I[e] = is;
            J[e] = js;
            M[e] = __builtin_sqrt(q);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < p.ty * p.tx; e += kEdNT) {
            const int r = e / p.tx, c = e - r * p.tx;
            const int y = y0 + r, x = x0 + c;
            if (y >= p.ny || x >= p.nx) continue;
            const int ce = (r + 1) * mx + c + 1;
            const double m = M[ce];
            const int64_t g = (int64_t)y * p.nx + x;
            bool lm = false;
            if (eroded[g] != 0 && m > 0) lm = canny_is_max(I[ce], J[ce], m, [&](int dy, int dx) { return M[ce + dy * mx + dx]; });
            magnitude[g] = m;
            local_max[g] = (uint8_t)lm;
            if (high_mask) {
                high_mask[g] = (uint8_t)(lm && m >= high);
                low_mask[g] = (uint8_t)(lm && m >= low);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kEdNT)
canny_magnitude_kernel(const double *__restrict__ isobel, const double *__restrict__ jsobel, double *__restrict__ magnitude, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        double q = isobel[i] * isobel[i];
        const double q2 = jsobel[i] * jsobel[i];
        q = q + q2;
        magnitude[i] = __builtin_sqrt(q);
    }
}

// one thread per pixel straight from global memory; the eroded mask keeps the neighbour reads inside the image
__global__ void __launch_bounds__(kEdNT)
canny_generic_kernel(const double *__restrict__ isobel, const double *__restrict__ jsobel, const double *__restrict__ magnitude,
                     const uint8_t *__restrict__ eroded, uint8_t *__restrict__ local_max, uint8_t *__restrict__ high_mask,
                     uint8_t *__restrict__ low_mask, double high, double low, int ny, int nx)
{
    const int64_t total = (int64_t)ny * nx;
    for (int64_t g = (int64_t)blockIdx.x * kEdNT + threadIdx.x; g < total; g += (int64_t)gridDim.x * kEdNT) {
        const int y = (int)(g / nx), x = (int)(g - (int64_t)y * nx);
        const double m = magnitude[g];
        bool lm = false;
        if (y >= 1 && y < ny - 1 && x >= 1 && x < nx - 1 && eroded[g] != 0 && m > 0)
            lm = canny_is_max(isobel[g], jsobel[g], m, [&](int dy, int dx) { return magnitude[g + (int64_t)dy * nx + dx]; });
        local_max[g] = (uint8_t)lm;
        if (high_mask) {
            high_mask[g] = (uint8_t)(lm && m >= high);
            low_mask[g] = (uint8_t)(lm && m >= low);
        }
    }
}

__global__ void __launch_bounds__(kEdNT)
canny_threshold_kernel(const double *__restrict__ magnitude, const uint8_t *__restrict__ local_max, uint8_t *__restrict__ high_mask,
                       uint8_t *__restrict__ low_mask, double high, double low, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        const bool lm = local_max[i] != 0;
        const double m = magnitude[i];
        high_mask[i] = (uint8_t)(lm && m >= high);
        low_mask[i] = (uint8_t)(lm && m >= low);
    }
}

// out = mask ? image : 0 on the bits of the samples (_canny.py:47-48: a masked copy, not a product: NaN and -x stay out)
template <typename U>
__global__ void __launch_bounds__(kEdNT)
masked_copy_kernel(const U *__restrict__ image, const uint8_t *__restrict__ mask, U *__restrict__ out, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) out[i] = mask[i] ? image[i] : U(0);
}

// out = double(smoothed) / (bleed_over + eps) (_canny.py:50), the sum and the quotient rounded on their own
template <typename T>
__global__ void __launch_bounds__(kEdNT)
canny_normalize_kernel(const T *__restrict__ smoothed, const double *__restrict__ bleed, double *__restrict__ out, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kEdNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEdNT) {
        const double d = bleed[i] + 2.220446049250313e-16;
        out[i] = (double)smoothed[i] / d;
    }
}

static bool is_byte(const mi_array *a) { return a->dtype == MI_BOOL || a->dtype == MI_U8; }

}  // namespace mi

using namespace mi;

extern "C" int mi_canny_nms(const mi_array *smoothed, const mi_array *eroded, const mi_array *magnitude, const mi_array *local_max,
                            const mi_array *high_mask, const mi_array *low_mask, double high, double low, mi_stream stream)
{
    int rc;
    if ((rc = check_array(smoothed, "smoothed")) || (rc = check_array(eroded, "eroded")) || (rc = check_array(magnitude, "magnitude")) ||
        (rc = check_array(local_max, "local_max")))
        return rc;
    MI_REQUIRE((high_mask == nullptr) == (low_mask == nullptr), MI_ERR_INVALID_ARG, "canny_nms: both threshold masks or neither");
    if (high_mask && ((rc = check_array(high_mask, "high_mask")) || (rc = check_array(low_mask, "low_mask")))) return rc;
    MI_REQUIRE(smoothed->ndim == 2, MI_ERR_INVALID_ARG, "canny_nms: 2-D images only");
    if (smoothed->dtype != MI_F64) {
        set_error("canny_nms: the smoothed image is float64 (the reference's stage is float64 for every input dtype)");
        return MI_ERR_UNSUPPORTED;
    }
    MI_REQUIRE(magnitude->dtype == MI_F64 && same_shape(smoothed, magnitude), MI_ERR_INVALID_ARG, "canny_nms: the magnitude is a float64 array of the image's shape");
    for (const mi_array *m : {eroded, local_max, high_mask, low_mask})
        MI_REQUIRE(!m || (is_byte(m) && same_shape(smoothed, m) && is_contiguous(m)), MI_ERR_INVALID_ARG,
                   "canny_nms: the masks are C-contiguous bool / uint8 arrays of the image's shape");
    MI_REQUIRE(is_contiguous(smoothed) && is_contiguous(magnitude), MI_ERR_NOT_CONTIGUOUS, "canny_nms needs C-contiguous arrays");
    MI_REQUIRE(magnitude->data != smoothed->data && local_max->data != eroded->data && (!high_mask || (high_mask->data != low_mask->data &&
               high_mask->data != eroded->data && low_mask->data != eroded->data && high_mask->data != local_max->data &&
               low_mask->data != local_max->data)), MI_ERR_INVALID_ARG, "canny_nms: the outputs may not share memory with an input or each other");
    const int64_t ny = smoothed->shape[0], nx = smoothed->shape[1], total = ny * nx;
    if (total == 0) return MI_OK;
    MI_REQUIRE(ny < ((int64_t)1 << 30) && nx < ((int64_t)1 << 30), MI_ERR_UNSUPPORTED, "canny_nms: axes shorter than 2^30");
    hipStream_t s = resolve_stream(stream);
    uint8_t *hm = high_mask ? (uint8_t *)high_mask->data : nullptr, *lo = low_mask ? (uint8_t *)low_mask->data : nullptr;
    if (!g_ed_generic) {
        const bool small = g_ed_small != 0;
        CnParams p;
        p.ny = (int)ny; p.nx = (int)nx;
        p.ty = (int)std::min<int64_t>(small ? 3 : kCnMaxTy, ny);
        p.tx = (int)std::min<int64_t>(small ? 5 : kCnMaxTx, nx);
        p.nty = (p.ny + p.ty - 1) / p.ty;
        p.ntx = (p.nx + p.tx - 1) / p.tx;
        const int64_t ntiles = (int64_t)p.nty * p.ntx;
        const int grid = box_grid(ntiles);
        hipLaunchKernelGGL(canny_nms_kernel, dim3(grid), dim3(kEdNT), 0, s, (const double *)smoothed->data, (const uint8_t *)eroded->data,
                           (double *)magnitude->data, (uint8_t *)local_max->data, hm, lo, high, low, p, ntiles);
        MI_HIP(hipGetLastError());
        note_kernel("mi::canny_nms_kernel grid=%d tile=%dx%d %s (Sobel, magnitude and non-maximum suppression in one launch, halo 2)",
                    grid, p.ty, p.tx, hm ? "masks" : "no masks");
        return MI_OK;
    }
    // the Sobel responses as SciPy's passes through scratch arrays, then one thread per pixel
    void *scratch = nullptr;
    if ((rc = pool_alloc(&scratch, (size_t)total * 3 * sizeof(double), s))) return rc;
    mi_array tmp = *smoothed, is = *smoothed, js = *smoothed;
    tmp.data = scratch;
    is.data = (double *)scratch + total;
    js.data = (double *)scratch + 2 * total;
    const double wd[3] = {-1.0, 0.0, 1.0}, ws[3] = {1.0, 2.0, 1.0};
    if (!(rc = mi_correlate1d(smoothed, &tmp, 0, wd, 3, 0, MI_MODE_REFLECT, 0.0, 0, stream)) &&
        !(rc = mi_correlate1d(&tmp, &is, 1, ws, 3, 0, MI_MODE_REFLECT, 0.0, 0, stream)) &&
        !(rc = mi_correlate1d(smoothed, &tmp, 1, wd, 3, 0, MI_MODE_REFLECT, 0.0, 0, stream)))
        rc = mi_correlate1d(&tmp, &js, 0, ws, 3, 0, MI_MODE_REFLECT, 0.0, 0, stream);
    const int grid = ed_grid(total);
    if (rc == MI_OK) {
        hipLaunchKernelGGL(canny_magnitude_kernel, dim3(grid), dim3(kEdNT), 0, s, (const double *)is.data, (const double *)js.data,
                           (double *)magnitude->data, total);
        hipLaunchKernelGGL(canny_generic_kernel, dim3(grid), dim3(kEdNT), 0, s, (const double *)is.data, (const double *)js.data,
                           (const double *)magnitude->data, (const uint8_t *)eroded->data, (uint8_t *)local_max->data, hm, lo, high, low, (int)ny, (int)nx);
    }
    const hipError_t e = hipGetLastError();
    pool_free(scratch);
    if (rc != MI_OK) return rc;
    MI_HIP(e);
    note_kernel("mi::canny_generic_kernel grid=%d (four mi_correlate1d passes, canny_magnitude_kernel, one thread per pixel)", grid);
    return MI_OK;
}

extern "C" int mi_masked_copy(const mi_array *image, const mi_array *mask, const mi_array *out, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(mask, "mask")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(out->dtype == image->dtype && same_shape(image, out) && is_byte(mask) && same_shape(image, mask), MI_ERR_INVALID_ARG,
               "masked_copy: an output of the image's dtype and a bool / uint8 mask, all of one shape");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(mask) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "masked_copy needs C-contiguous arrays");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int grid = ed_grid(total);
#define ED_MC(U) hipLaunchKernelGGL((masked_copy_kernel<U>), dim3(grid), dim3(kEdNT), 0, s, (const U *)image->data, (const uint8_t *)mask->data, (U *)out->data, total)
    switch (dtype_size(image->dtype)) {
    case 1: ED_MC(uint8_t); break;
    case 2: ED_MC(uint16_t); break;
    case 4: ED_MC(uint32_t); break;
    default: ED_MC(uint64_t); break;
    }
#undef ED_MC
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_canny_normalize(const mi_array *smoothed, const mi_array *bleed_over, const mi_array *out, mi_stream stream)
{
    int rc;
    if ((rc = check_array(smoothed, "smoothed")) || (rc = check_array(bleed_over, "bleed_over")) || (rc = check_array(out, "out"))) return rc;
    if (smoothed->dtype != MI_F32 && smoothed->dtype != MI_F64) {
        set_error("canny_normalize: a float32 / float64 smoothed image (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    MI_REQUIRE(bleed_over->dtype == MI_F64 && out->dtype == MI_F64 && same_shape(smoothed, bleed_over) && same_shape(smoothed, out), MI_ERR_INVALID_ARG,
               "canny_normalize: float64 bleed_over and output of the image's shape");
    MI_REQUIRE(is_contiguous(smoothed) && is_contiguous(bleed_over) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "canny_normalize needs C-contiguous arrays");
    const int64_t total = numel(smoothed);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int grid = ed_grid(total);
    if (smoothed->dtype == MI_F32)
        hipLaunchKernelGGL((canny_normalize_kernel<float>), dim3(grid), dim3(kEdNT), 0, s, (const float *)smoothed->data, (const double *)bleed_over->data, (double *)out->data, total);
    else
        hipLaunchKernelGGL((canny_normalize_kernel<double>), dim3(grid), dim3(kEdNT), 0, s, (const double *)smoothed->data, (const double *)bleed_over->data, (double *)out->data, total);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_canny_threshold(const mi_array *magnitude, const mi_array *local_max, const mi_array *high_mask, const mi_array *low_mask,
                                  double high, double low, mi_stream stream)
{
    int rc;
    if ((rc = check_array(magnitude, "magnitude")) || (rc = check_array(local_max, "local_max")) || (rc = check_array(high_mask, "high_mask")) ||
        (rc = check_array(low_mask, "low_mask")))
        return rc;
    MI_REQUIRE(magnitude->dtype == MI_F64 && is_contiguous(magnitude), MI_ERR_INVALID_ARG, "canny_threshold: a C-contiguous float64 magnitude");
    for (const mi_array *m : {local_max, high_mask, low_mask})
        MI_REQUIRE(is_byte(m) && same_shape(magnitude, m) && is_contiguous(m), MI_ERR_INVALID_ARG,
                   "canny_threshold: the masks are C-contiguous bool / uint8 arrays of the magnitude's shape");
    MI_REQUIRE(high_mask->data != low_mask->data && high_mask->data != local_max->data && low_mask->data != local_max->data, MI_ERR_INVALID_ARG,
               "canny_threshold: the masks may not share memory");
    const int64_t total = numel(magnitude);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    hipLaunchKernelGGL(canny_threshold_kernel, dim3(ed_grid(total)), dim3(kEdNT), 0, s, (const double *)magnitude->data,
                       (const uint8_t *)local_max->data, (uint8_t *)high_mask->data, (uint8_t *)low_mask->data, high, low, total);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_debug_set_edges(int small_tiles, int force_generic)
{
    g_ed_small = small_tiles != 0;
    g_ed_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_edge_filter(const mi_array *image, const mi_array *out, const mi_array *mask, const double *weights, int naxes,
                              int magnitude, int mode, double cval, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(out, "out"))) return rc;
    if (mask && (rc = check_array(mask, "mask"))) return rc;
    MI_REQUIRE(weights, MI_ERR_INVALID_ARG, "NULL argument");
    const int rank = image->ndim;
    MI_REQUIRE(rank >= 1, MI_ERR_INVALID_ARG, "edge_filter: arrays of rank 1 to 8");
    if (image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("edge_filter: float32 and float64 images only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    MI_REQUIRE(out->dtype == MI_F64 && same_shape(image, out), MI_ERR_INVALID_ARG, "edge_filter: the output is a float64 array of the image's shape");
    MI_REQUIRE(!mask || ((mask->dtype == MI_BOOL || mask->dtype == MI_U8) && same_shape(image, mask)), MI_ERR_INVALID_ARG,
               "edge_filter: the mask is a bool / uint8 array of the image's shape");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(out) && (!mask || is_contiguous(mask)), MI_ERR_NOT_CONTIGUOUS,
               "edge_filter needs C-contiguous arrays");
    MI_REQUIRE(naxes >= 1 && naxes <= MI_MAX_NDIM, MI_ERR_INVALID_ARG, "edge_filter: between one and 8 edge axes");
    MI_REQUIRE(magnitude || naxes == 1, MI_ERR_INVALID_ARG, "edge_filter: the signed response has one edge axis");
    MI_REQUIRE(mode >= MI_MODE_REFLECT && mode <= MI_MODE_GRID_CONSTANT, MI_ERR_INVALID_ARG, "edge_filter: unknown mode");
    MI_REQUIRE(out->data != image->data && (!mask || out->data != mask->data), MI_ERR_INVALID_ARG, "edge_filter: the output may not be an input");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    mode = filter_mode(mode);
    hipStream_t s = resolve_stream(stream);
    const uint8_t *m = mask ? (const uint8_t *)mask->data : nullptr;
    if (!g_ed_generic && (rank == 2 || rank == 3) && naxes <= 3) {
        rc = ed_fused(image, m, (double *)out->data, weights, naxes, magnitude, mode, cval, s);
        if (rc != MI_ERR_UNSUPPORTED) return rc;
    }
    // one dense correlate per edge axis through a scratch array of the image's dtype
    int64_t ntap = 1;
    int64_t wshape[MI_MAX_NDIM];
    int origins[MI_MAX_NDIM];
    for (int d = 0; d < rank; d++) {
        ntap *= 3;
        wshape[d] = 3;
        origins[d] = 0;
    }
    void *scratch = nullptr;
    if ((rc = pool_alloc(&scratch, (size_t)total * dtype_size(image->dtype), s))) return rc;
    mi_array resp = *image;
    resp.data = scratch;
    const int grid = ed_grid(total);
    for (int a = 0; a < naxes && rc == MI_OK; a++) {
        rc = mi_correlate_nd(image, &resp, weights + a * ntap, wshape, origins, mode, cval, 0, stream);
        if (rc != MI_OK) break;
        if (image->dtype == MI_F32)
            hipLaunchKernelGGL((edge_accumulate_kernel<float>), dim3(grid), dim3(kEdNT), 0, s, (const float *)scratch, (double *)out->data, total, a == 0, magnitude);
        else
            hipLaunchKernelGGL((edge_accumulate_kernel<double>), dim3(grid), dim3(kEdNT), 0, s, (const double *)scratch, (double *)out->data, total, a == 0, magnitude);
    }
    if (rc == MI_OK && (magnitude || m))
        hipLaunchKernelGGL(edge_finish_kernel, dim3(grid), dim3(kEdNT), 0, s, (double *)out->data, m, total, magnitude, (double)rank);
    const hipError_t e = hipGetLastError();
    pool_free(scratch);
    if (rc != MI_OK) return rc;
    MI_HIP(e);
    note_kernel("mi::edge_generic<%s> grid=%d axes=%d %s (one mi_correlate_nd per edge axis, edge_accumulate_kernel and "
                "edge_finish_kernel, rank %d)",
                image->dtype == MI_F32 ? "float32" : "float64", grid, naxes, magnitude ? "magnitude" : "signed", rank);
    return MI_OK;
}

extern "C" int mi_edge_pair_magnitude(const mi_array *a, const mi_array *b, const mi_array *out, double divisor, mi_stream stream)
{
    int rc;
    if ((rc = check_array(a, "a")) || (rc = check_array(b, "b")) || (rc = check_array(out, "out"))) return rc;
    if (a->dtype != MI_F32 && a->dtype != MI_F64) {
        set_error("edge_pair_magnitude: float32 and float64 arrays only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    MI_REQUIRE(b->dtype == a->dtype && out->dtype == a->dtype && same_shape(a, b) && same_shape(a, out), MI_ERR_INVALID_ARG,
               "edge_pair_magnitude: three arrays of one shape and dtype");
    MI_REQUIRE(is_contiguous(a) && is_contiguous(b) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "edge_pair_magnitude needs C-contiguous arrays");
    const int64_t total = numel(a);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int grid = ed_grid(total);
    if (a->dtype == MI_F32)
        hipLaunchKernelGGL((edge_pair_kernel<float>), dim3(grid), dim3(kEdNT), 0, s, (const float *)a->data, (const float *)b->data, (float *)out->data, total, (float)divisor);
    else
        hipLaunchKernelGGL((edge_pair_kernel<double>), dim3(grid), dim3(kEdNT), 0, s, (const double *)a->data, (const double *)b->data, (double *)out->data, total, divisor);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_threshold_masks(const mi_array *image, const mi_array *low, const mi_array *high, double low_value, double high_value,
                                  const mi_array *mask_low, const mi_array *mask_high, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(mask_low, "mask_low")) || (rc = check_array(mask_high, "mask_high"))) return rc;
    if ((low && (rc = check_array(low, "low"))) || (high && (rc = check_array(high, "high")))) return rc;
    if (image->dtype == MI_F16 || image->dtype == MI_I64 || image->dtype == MI_U64) {
        set_error("threshold_masks: images of up to 32-bit integers, float32 and float64 (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    for (const mi_array *m : {mask_low, mask_high})
        MI_REQUIRE((m->dtype == MI_BOOL || m->dtype == MI_U8) && same_shape(image, m), MI_ERR_INVALID_ARG,
                   "threshold_masks: the masks are bool / uint8 arrays of the image's shape");
    for (const mi_array *t : {low, high})
        MI_REQUIRE(!t || (t->dtype == MI_F64 && same_shape(image, t)), MI_ERR_INVALID_ARG,
                   "threshold_masks: a threshold array is a float64 array of the image's shape");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(mask_low) && is_contiguous(mask_high) && (!low || is_contiguous(low)) &&
               (!high || is_contiguous(high)), MI_ERR_NOT_CONTIGUOUS, "threshold_masks needs C-contiguous arrays");
    MI_REQUIRE(mask_low->data != mask_high->data && mask_low->data != image->data && mask_high->data != image->data, MI_ERR_INVALID_ARG,
               "threshold_masks: the masks may not share memory with each other or the image");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int grid = ed_grid(total);
    hipLaunchKernelGGL(threshold_masks_kernel, dim3(grid), dim3(kEdNT), 0, s, image->data, image->dtype, low ? (const double *)low->data : nullptr,
                       high ? (const double *)high->data : nullptr, low_value, high_value, (uint8_t *)mask_low->data, (uint8_t *)mask_high->data, total);
    MI_HIP(hipGetLastError());
    note_kernel("mi::threshold_masks_kernel grid=%d (both hysteresis masks in one launch)", grid);
    return MI_OK;
}
