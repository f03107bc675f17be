// exposure.hip -- skimage.exposure on the device: contrast limited adaptive histogram equalisation (equalize_adapthist) as three
// launches without a host round trip, and numpy.interp through a table (equalize_hist).
//
// Reference path replaced: cupyimg/skimage/exposure/_adapthist.py:86-275, which pads the image, gathers every contextual region
// into a 2-D array, pulls that array to the host for numpy.bincount and a Python redistribution loop per region, and blends
// in 2^ndim rounds of take_along_axis over block-transposed copies; exposure.py:245-257 pulls the whole image to the host for
// numpy.interp.
//
// The arithmetic is written down in include/mi355img.h above mi_clahe_maps (steps 1 .. 8); this file is compiled with
// -ffp-contract=off, every product, quotient and sum rounds on its own.
//
// clahe_maps_kernel: one workgroup per contextual region.  It reads its region straight from the image (the padded image
// never exists: reflect indexing here), histograms into LDS -- one private histogram per wave up to 1024 bins, merged before
// the clip, so that the lanes of eight waves do not queue on the few addresses a smooth region touches; one shared histogram
// above that -- then clips and redistributes as the reference does, every stage a masked elementwise update plus a workgroup
// reduction, and ends with a workgroup prefix sum that writes the mapping as uint16.
// clahe_apply_kernel (ranks 2 and 3): a workgroup owns a slab of one interpolation cell, stages the 2^ndim mappings of the cell
// and the blend coefficients j / k in LDS, recomputes the bin of every voxel from the image and blends.
// clahe_generic_kernel (ranks 1 .. 4): the same arithmetic, one thread per voxel, mappings from global memory.
// Both reduce min and max of the uint16 result into the work block with one pair of integer atomics per workgroup.
// clahe_finish_kernel: uint16 -> float64 and the final rescale, min and max read on the device.
// interp_map_kernel: numpy.interp (slope form, ends clamped) with the table in LDS when it fits, else searched in global memory.
#include "common.hpp"
#include <algorithm>

namespace mi {

constexpr int kClNd = MI_CLAHE_MAX_NDIM;
constexpr int kClMapNT = 512;                // clahe_maps_kernel: 8 waves
constexpr int kClMapNW = kClMapNT / 64;
constexpr int kClPrivateBins = 1024;         // per-wave histograms up to here: 8 x 1024 x 4 B = 32 KiB
constexpr int kClNT = 256;
constexpr int kClStageBytes = 64 * 1024;     // mappings staged by clahe_apply_kernel at most
constexpr int kClCoefMax = 1024;             // sum of the kernel sizes whose coefficients it stages
constexpr int kInterpLdsKnots = 4096;        // 2 x 8 B x 4096 = 64 KiB

struct ClGeom {
    int nd;
    int nbins, bin_size;
    int constant;                 // umin == umax
    double umin, umax, span;      // span = umax - umin
    int64_t total;
    int shape[kClNd];
    int k[kClNd];
    int nr[kClNd];                // contextual regions per axis (ns_hist)
    int64_t stride[kClNd];        // elements
    int npix, clim;               // prod(k), the clip limit
    double scale;                 // 16383 / prod(k)
};

// step 1: img_as_uint
template <typename T>
__device__ __forceinline__ uint32_t cl_as_uint(T x)
{
    if constexpr (std::is_same<T, uint8_t>::value) {
        return (uint32_t)x * 257u;
    } else if constexpr (std::is_same<T, uint16_t>::value) {
        return x;
    } else if constexpr (std::is_same<T, float>::value) {
        float t = __builtin_rintf(x * 65535.0f);
        t = fminf(fmaxf(t, 0.0f), 65535.0f);
        return (uint32_t)t;
    } else {
        double t = __builtin_rint(x * 65535.0);
        t = fmin(fmax(t, 0.0), 65535.0);
        return (uint32_t)t;
    }
}

// steps 2 and 3: the 14-bit grey level and its bin
__device__ __forceinline__ int cl_bin(uint32_t u, const ClGeom &g)
{
    uint32_t gray;
    if (g.constant) {
        gray = u < 16383u ? u : 16383u;
    } else {
        double t = fmin(fmax((double)u, g.umin), g.umax);
        t = (t - g.umin) / g.span;
        t = t * 16383.0 + 0.0;
        gray = (uint32_t)__builtin_rint(t);
    }
    return (int)(gray / (uint32_t)g.bin_size);
}

// numpy.pad(mode="reflect") for an index at or beyond 0: period 2 (n - 1), an axis of length 1 repeats its sample
__device__ __forceinline__ int cl_reflect(int i, int n)
{
    if (i < n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    return i < n ? i : p - i;
}

// Sum of two integers over the workgroup, the same value in every thread.  `red` holds two buffers of 2 * NW integers used
// in turn (`phase` counts the calls): a thread that runs ahead writes the other buffer, and it cannot run two calls ahead
// without passing the barrier of the call in between, which every reader of this buffer has then left behind.
template <int NW>
__device__ __forceinline__ void cl_reduce2(int &a, int &b, int *red, int &phase)
{
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
    }
    int *buf = red + (phase & 1) * 2 * NW;
    phase++;
    if ((threadIdx.x & 63) == 0) {
        buf[2 * (threadIdx.x >> 6)] = a;
        buf[2 * (threadIdx.x >> 6) + 1] = b;
    }
    __syncthreads();
    a = 0;
    b = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        a += buf[2 * w];
        b += buf[2 * w + 1];
    }
}

// LDS: int H[nwh * nbins] | int red[4 * NW] | int scan[NW + 1]
template <typename T>
__global__ void __launch_bounds__(kClMapNT)
clahe_maps_kernel(const T *__restrict__ img, const ClGeom g, const int nwh, uint16_t *__restrict__ maps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
    int *H = reinterpret_cast<int *>(cl_lds);
    int *red = H + (size_t)nwh * g.nbins;
    int *scan = red + 4 * kClMapNW;
    const int tid = threadIdx.x;
    const int nbins = g.nbins;
    int phase = 0;

    for (int b = tid; b < nwh * nbins; b += kClMapNT) H[b] = 0;
    __syncthreads();

    // ---- step 4: the region's origin, and its histogram
    int org[kClNd];
    {
        int r = blockIdx.x;
        for (int a = g.nd - 1; a >= 0; a--) {
            const int q = r / g.nr[a];
            org[a] = (r - q * g.nr[a]) * g.k[a];
            r = q;
        }
    }
    int *Hw = H + (nwh > 1 ? (tid >> 6) * nbins : 0);
    for (int v = tid; v < g.npix; v += kClMapNT) {
        int r = v;
        int64_t off = 0;
        for (int a = g.nd - 1; a >= 0; a--) {
            const int q = r / g.k[a];
            const int j = r - q * g.k[a];
            r = q;
            off += (int64_t)cl_reflect(org[a] + j, g.shape[a]) * g.stride[a];
        }
        atomicAdd(&Hw[cl_bin(cl_as_uint<T>(img[off]), g)], 1);
    }
    __syncthreads();
    if (nwh > 1) {
        for (int b = tid; b < nbins; b += kClMapNT) {
            int s = H[b];
            for (int w = 1; w < nwh; w++) s += H[w * nbins + b];
            H[b] = s;                                 // bin b of every wave's histogram belongs to this thread alone
        }
    }
    // (bin b is touched by thread b % NT only until the strided passes, which are fenced by the barrier inside cl_reduce2)

    // ---- step 5: clip, then redistribute in three stages
    const int clim = g.clim;
    int excess = 0, dummy = 0;
    for (int b = tid; b < nbins; b += kClMapNT) {
        const int h = H[b];
        if (h > clim) {
            excess += h - clim;
            H[b] = clim;
        }
    }
    cl_reduce2<kClMapNW>(excess, dummy, red, phase);
    int n_excess = excess;
    const int bin_incr = n_excess / nbins;
    const int upper = clim - bin_incr;
    int dec = 0, under = 0;
    for (int b = tid; b < nbins; b += kClMapNT) {
        int h = H[b];
        if (h < upper) {
            h += bin_incr;
            dec += bin_incr;
        }
        if (h >= upper && h < clim) {
            dec += clim - h;
            h = clim;
        }
        H[b] = h;
        under += h < clim;
    }
    cl_reduce2<kClMapNW>(dec, under, red, phase);
    n_excess -= dec;
    int n_under = under;
    while (n_excess > 0 && n_under > 0) {             // no bin under the limit: the reference's round that changes nothing
        for (int index = 0; index < nbins; index++) {
            const int step = max(1, n_under / n_excess);
            int cnt = 0, reached = 0;
            for (int64_t b = index + (int64_t)tid * step; b < nbins; b += (int64_t)kClMapNT * step) {
                const int h = H[b];
                if (h < clim) {
                    H[b] = h + 1;
                    cnt++;
                    reached += h + 1 == clim;
                }
            }
            cl_reduce2<kClMapNW>(cnt, reached, red, phase);
            n_excess -= cnt;
            n_under -= reached;
            if (n_excess <= 0 || n_under == 0) break; // with no bin left under the limit the rest of the round is idle
        }
    }
    __syncthreads();

    // ---- step 6: cumulative sum and mapping; thread t owns bins [t * per, (t + 1) * per)
    const int per = (nbins + kClMapNT - 1) / kClMapNT;
    const int b0 = min(tid * per, nbins), b1 = min(b0 + per, nbins);
    int mine = 0;
    for (int b = b0; b < b1; b++) mine += H[b];
    int incl = mine;
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) scan[wave] = incl;
    __syncthreads();
    int base = incl - mine;
    for (int w = 0; w < wave; w++) base += scan[w];
    uint16_t *out = maps + (int64_t)blockIdx.x * nbins;
    for (int b = b0; b < b1; b++) {
        base += H[b];
        double m = (double)base * g.scale;
        m = m + 0.0;
        m = fmin(m, 16383.0);
        out[b] = (uint16_t)(int64_t)m;
    }
}

// step 7 for one voxel: reg[a][e] = the region (clamped) on side e of axis a times its stride in regions, c[a] = j_a / k_a
template <int ND, typename M>
__device__ __forceinline__ uint32_t cl_blend(const M &map_at, const double *c)
{
    float acc = 0.0f;
#pragma unroll
    for (int e = 0; e < (1 << ND); e++) {
        // itertools.product order: axis 0 slowest; the coefficient product starts at the last axis
        double w = 0.0;
#pragma unroll
        for (int a = ND - 1; a >= 0; a--) {
            const int bit = (e >> (ND - 1 - a)) & 1;
            const double f = bit ? c[a] : 1.0 - c[a];
            w = a == ND - 1 ? f : w * f;
        }
        const float term = (float)((double)map_at(e) * w);
        acc = e == 0 ? term : acc + term;
    }
    return (uint32_t)acc;
}

__device__ __forceinline__ void cl_block_minmax(uint32_t lo, uint32_t hi, uint32_t *__restrict__ work)
{
    __shared__ uint32_t mm[2][kClNT / 64];
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_down((int)lo, o));
        hi = max(hi, (uint32_t)__shfl_down((int)hi, o));
    }
    if ((threadIdx.x & 63) == 0) {
        mm[0][threadIdx.x >> 6] = lo;
        mm[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kClNT / 64; w++) {
            lo = min(lo, mm[0][w]);
            hi = max(hi, mm[1][w]);
        }
        if (lo <= hi) {                               // a workgroup without voxels leaves the block alone
            atomicMin(&work[0], lo);
            atomicMin(&work[1], 65535u - hi);
        }
    }
}

struct ClApply {
    int ncell[kClNd];             // interpolation cells per axis (ns_proc = regions + 1)
    int slabs, slab;              // slabs per cell along axis 0, their thickness
};

// LDS: double C[sum k] | uint16 M[2^ND][nbins]
template <typename T, int ND>
__global__ void __launch_bounds__(kClNT)
clahe_apply_kernel(const T *__restrict__ img, const ClGeom g, const ClApply p, const uint16_t *__restrict__ maps,
                   uint16_t *__restrict__ out, uint32_t *__restrict__ work)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
    double *C = reinterpret_cast<double *>(cl_lds);
    int coff[ND];
    int ksum = 0;
#pragma unroll
    for (int a = 0; a < ND; a++) {
        coff[a] = ksum;
        ksum += g.k[a];
    }
    uint16_t *M = reinterpret_cast<uint16_t *>(C + ksum);
    const int tid = threadIdx.x;
    const int nbins = g.nbins;

    int cell[ND];
    int r = blockIdx.x;
    const int sl = r % p.slabs;
    r /= p.slabs;
#pragma unroll
    for (int a = ND - 1; a >= 0; a--) {
        cell[a] = r % p.ncell[a];
        r /= p.ncell[a];
    }
#pragma unroll
    for (int a = 0; a < ND; a++)
        for (int j = tid; j < g.k[a]; j += kClNT) C[coff[a] + j] = (double)j / (double)g.k[a];
#pragma unroll
    for (int e = 0; e < (1 << ND); e++) {
        int64_t reg = 0;
#pragma unroll
        for (int a = 0; a < ND; a++) {
            const int bit = (e >> (ND - 1 - a)) & 1;
            const int ra = min(max(cell[a] - 1 + bit, 0), g.nr[a] - 1);     // the mappings are edge-replicated by one region
            reg = reg * g.nr[a] + ra;
        }
        const uint16_t *src = maps + reg * nbins;
        for (int b = tid; b < nbins; b += kClNT) M[e * nbins + b] = src[b];
    }
    __syncthreads();

    // the cell's voxels: image coordinate = cell * k - k / 2 + j
    int lo[ND], ext[ND];
    int nvox = 1;                                     // at most prod(k) <= 2^30
#pragma unroll
    for (int a = 0; a < ND; a++) {
        int j0 = 0, j1 = g.k[a];
        if (a == 0) {
            j0 = sl * p.slab;
            j1 = min(j0 + p.slab, g.k[0]);
        }
        const int o = cell[a] * g.k[a] - g.k[a] / 2;
        const int i0 = max(o + j0, 0), i1 = min(o + j1, g.shape[a]);
        lo[a] = i0;
        ext[a] = max(i1 - i0, 0);
        nvox *= ext[a];
    }
    uint32_t vmin = 0xffffffffu, vmax = 0;
    for (int v = tid; v < nvox; v += kClNT) {
        int q = v;
        int64_t off = 0;
        double c[ND];
#pragma unroll
        for (int a = ND - 1; a >= 0; a--) {
            const int qq = q / ext[a];
            const int i = lo[a] + (q - qq * ext[a]);
            q = qq;
            off += (int64_t)i * g.stride[a];
            c[a] = C[coff[a] + (i - (cell[a] * g.k[a] - g.k[a] / 2))];
        }
        const int bin = cl_bin(cl_as_uint<T>(img[off]), g);
        const uint32_t val = cl_blend<ND>([&](int e) { return M[e * nbins + bin]; }, c);
        out[off] = (uint16_t)val;
        vmin = min(vmin, val & 0xffffu);
        vmax = max(vmax, val & 0xffffu);
    }
    cl_block_minmax(vmin, vmax, work);
}

template <typename T, int ND>
__global__ void __launch_bounds__(kClNT)
clahe_generic_kernel(const T *__restrict__ img, const ClGeom g, const uint16_t *__restrict__ maps, uint16_t *__restrict__ out,
                     uint32_t *__restrict__ work)
{
    uint32_t vmin = 0xffffffffu, vmax = 0;
    const int nbins = g.nbins;
    for (int64_t v = (int64_t)blockIdx.x * kClNT + threadIdx.x; v < g.total; v += (int64_t)gridDim.x * kClNT) {
        int64_t q = v;
        double c[ND];
        int cell[ND];
#pragma unroll
        for (int a = ND - 1; a >= 0; a--) {
            const int64_t qq = q / g.shape[a];
            const int i = (int)(q - qq * g.shape[a]);
            q = qq;
            const int pp = i + g.k[a] / 2;
            cell[a] = pp / g.k[a];
            c[a] = (double)(pp - cell[a] * g.k[a]) / (double)g.k[a];
        }
        const int bin = cl_bin(cl_as_uint<T>(img[v]), g);
        const uint32_t val = cl_blend<ND>([&](int e) {
            int64_t reg = 0;
#pragma unroll
            for (int a = 0; a < ND; a++) {
                const int bit = (e >> (ND - 1 - a)) & 1;
                reg = reg * g.nr[a] + min(max(cell[a] - 1 + bit, 0), g.nr[a] - 1);
            }
            return maps[reg * nbins + bin];
        }, c);
        out[v] = (uint16_t)val;
        vmin = min(vmin, val & 0xffffu);
        vmax = max(vmax, val & 0xffffu);
    }
    cl_block_minmax(vmin, vmax, work);
}

// step 8
__global__ void __launch_bounds__(kClNT)
clahe_finish_kernel(const uint16_t *__restrict__ v, double *__restrict__ out, int64_t total, const uint32_t *__restrict__ work)
{
    const uint32_t lo = work[0], hi = 65535u - work[1];
    const double inv = 1.0 / 65535;
    const double fmin_ = (double)lo * inv, fmax_ = (double)hi * inv;
    const double span = fmax_ - fmin_;
    for (int64_t i = (int64_t)blockIdx.x * kClNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kClNT) {
        double f = (double)v[i] * inv;
        if (lo != hi) {
            f = (f - fmin_) / span;
            f = f * 1.0 + 0.0;
        }
        out[i] = f;
    }
}

// numpy.interp for one value: j = the last knot at or below x; ends clamped; slope form, with NumPy's two retries when the
// slope form gives NaN
template <typename P>
__device__ __forceinline__ double interp_one(double x, const P xp, const P fp, int n)
{
    if (x != x) return x;
    if (n == 1) return fp[0];
    if (x > xp[n - 1]) return fp[n - 1];
    if (x < xp[0]) return fp[0];
    int lo = 0, hi = n;                               // xp[lo] <= x < xp[hi] (xp[n] = +inf)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x >= xp[mid]) lo = mid; else hi = mid;
    }
    const int j = lo;
    if (j == n - 1) return fp[j];
    if (xp[j] == x) return fp[j];
    const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    double r = slope * (x - xp[j]) + fp[j];
    if (r != r) {
        r = slope * (x - xp[j + 1]) + fp[j + 1];
        if (r != r && fp[j] == fp[j + 1]) r = fp[j];
    }
    return r;
}

template <typename T, bool LDS>
__global__ void __launch_bounds__(kClNT)
interp_map_kernel(const T *__restrict__ in, double *__restrict__ out, int64_t total, const double *__restrict__ xp,
                  const double *__restrict__ fp, int n)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
    const double *X = xp, *F = fp;
    if (LDS) {
        double *sx = reinterpret_cast<double *>(cl_lds), *sf = sx + n;
        for (int i = threadIdx.x; i < n; i += kClNT) {
            sx[i] = xp[i];
            sf[i] = fp[i];
        }
        __syncthreads();
        X = sx;
        F = sf;
    }
    for (int64_t i = (int64_t)blockIdx.x * kClNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kClNT)
        out[i] = interp_one((double)in[i], X, F, n);
}

// skimage.exposure.rescale_intensity: F = float for float32 images (NumPy keeps the image dtype against Python scalars), else
// double; the scalars arrive already rounded to F
template <typename F>
__global__ void __launch_bounds__(kClNT)
rescale_kernel(const void *__restrict__ in, int in_dt, void *__restrict__ out, int out_dt, int64_t total, F imin, F imax, F den, F mul,
               F omin, F omax, int clip_only)
{
    for (int64_t i = (int64_t)blockIdx.x * kClNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kClNT) {
        F x = (F)load_as_f64(in, i, in_dt);
        x = x < imin ? imin : (x > imax ? imax : x);
        if (clip_only) {
            x = x < omin ? omin : (x > omax ? omax : x);
        } else {
            x = (x - imin) / den;
            x = x * mul;
            x = x + omin;
        }
        store_as(out, i, out_dt, (double)x);
    }
}

// test hook: ranks 2 and 3 through the per-voxel kernel; one shared histogram whatever the number of bins
static Knob g_cl_generic{0}, g_cl_shared{0};

static const char *cl_dtype_name(int dt)
{
    return dt == MI_U8 ? "uint8" : dt == MI_U16 ? "uint16" : dt == MI_F32 ? "float32" : "float64";
}

// shared argument checks; fills g
static int cl_geom(const mi_array *image, const int *kernel, double umin, double umax, int nbins, int64_t clim, const mi_array *maps,
                   ClGeom *g)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(maps, "maps"))) return rc;
    MI_REQUIRE(kernel, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(image->ndim >= 1 && image->ndim <= kClNd, MI_ERR_INVALID_ARG, "clahe: ranks 1 to 4");
    if (image->dtype != MI_U8 && image->dtype != MI_U16 && image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("clahe: uint8, uint16, float32 and float64 images only");
        return MI_ERR_UNSUPPORTED;
    }
    MI_REQUIRE(is_contiguous(image) && is_contiguous(maps), MI_ERR_NOT_CONTIGUOUS, "clahe needs C-contiguous arrays");
    MI_REQUIRE(nbins >= 1 && nbins <= MI_CLAHE_GRAY, MI_ERR_INVALID_ARG, "clahe: nbins must be 1 .. 16384");
    MI_REQUIRE(umin <= umax && umin >= 0.0 && umax <= 65535.0, MI_ERR_INVALID_ARG, "clahe: umin, umax must be the uint16 range of the image");
    memset(g, 0, sizeof(*g));
    g->nd = image->ndim;
    g->nbins = nbins;
    g->bin_size = 1 + MI_CLAHE_GRAY / nbins;
    g->umin = umin;
    g->umax = umax;
    g->span = umax - umin;
    g->constant = umin == umax;
    int64_t st = 1, npix = 1, nreg = 1;
    for (int a = image->ndim - 1; a >= 0; a--) {
        MI_REQUIRE(image->shape[a] >= 1 && image->shape[a] < ((int64_t)1 << 30), MI_ERR_INVALID_ARG, "clahe: empty or oversized axis");
        MI_REQUIRE(kernel[a] >= 1 && kernel[a] < (1 << 30), MI_ERR_INVALID_ARG, "clahe: kernel sizes must be at least 1");
        g->shape[a] = (int)image->shape[a];
        g->k[a] = kernel[a];
        g->nr[a] = (int)((image->shape[a] + kernel[a] - 1) / kernel[a]);
        g->stride[a] = st;
        st *= image->shape[a];
        npix *= kernel[a];
        nreg *= g->nr[a];
        MI_REQUIRE(npix <= ((int64_t)1 << 30), MI_ERR_INVALID_ARG, "clahe: a contextual region holds at most 2^30 voxels");
    }
    g->total = st;
    g->npix = (int)npix;
    MI_REQUIRE(clim >= 1 && clim <= npix, MI_ERR_INVALID_ARG, "clahe: the clip limit must be 1 .. prod(kernel)");
    g->clim = (int)clim;
    g->scale = 16383.0 / (double)npix;
    MI_REQUIRE(nreg < ((int64_t)1 << 31) / 2, MI_ERR_INVALID_ARG, "clahe: too many contextual regions");
    MI_REQUIRE(maps->dtype == MI_U16 && maps->ndim == 2 && maps->shape[0] == nreg && maps->shape[1] == nbins, MI_ERR_INVALID_ARG,
               "maps must be uint16 of shape (regions, nbins)");
    return MI_OK;
}

#define CL_BY_DTYPE(GO)                                 \
    do {                                                \
        switch (image->dtype) {                         \
        case MI_U8: GO(uint8_t); break;                 \
        case MI_U16: GO(uint16_t); break;               \
        case MI_F32: GO(float); break;                  \
        default: GO(double); break;                     \
        }                                               \
    } while (0)

template <typename T>
static int launch_cl_maps(const mi_array *image, const ClGeom &g, int nwh, size_t lds, int grid, uint16_t *maps, hipStream_t s)
{
    static PerDeviceOnce attr;
    if (!attr) {
        MI_HIP(hipFuncSetAttribute((const void *)clahe_maps_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        attr = true;
    }
    hipLaunchKernelGGL((clahe_maps_kernel<T>), dim3((unsigned)grid), dim3(kClMapNT), lds, s, (const T *)image->data, g, nwh, maps);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

template <typename T, int ND>
static int launch_cl_apply(const mi_array *image, const ClGeom &g, const ClApply &p, size_t lds, int grid, const uint16_t *maps,
                           uint16_t *out, uint32_t *work, hipStream_t s)
{
    static PerDeviceOnce attr;
    if (!attr) {
        MI_HIP(hipFuncSetAttribute((const void *)clahe_apply_kernel<T, ND>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        attr = true;
    }
    hipLaunchKernelGGL((clahe_apply_kernel<T, ND>), dim3((unsigned)grid), dim3(kClNT), lds, s, (const T *)image->data, g, p, maps, out, work);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

template <typename T, bool LDS>
static int launch_interp(const mi_array *image, const mi_array *out, int64_t total, const double *xp, const double *fp, int n, hipStream_t s)
{
    static PerDeviceOnce attr;
    if (LDS && !attr) {
        MI_HIP(hipFuncSetAttribute((const void *)interp_map_kernel<T, LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        attr = true;
    }
    dim3 grid;
    grid_for(total, kClNT, &grid);
    hipLaunchKernelGGL((interp_map_kernel<T, LDS>), grid, dim3(kClNT), LDS ? (size_t)16 * n : 0, s, (const T *)image->data,
                       (double *)out->data, total, xp, fp, n);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_clahe(int force_generic, int force_shared_hist)
{
    g_cl_generic = force_generic != 0;
    g_cl_shared = force_shared_hist != 0;
    return MI_OK;
}

extern "C" int mi_clahe_maps(const mi_array *image, const int *kernel, double umin, double umax, int nbins, int64_t clip_limit,
                             const mi_array *maps, mi_stream stream)
{
    ClGeom g;
    int rc;
    if ((rc = cl_geom(image, kernel, umin, umax, nbins, clip_limit, maps, &g))) return rc;
    hipStream_t s = resolve_stream(stream);
    const int nwh = (nbins <= kClPrivateBins && !g_cl_shared) ? kClMapNW : 1;
    const size_t lds = ((size_t)nwh * nbins + 4 * kClMapNW + kClMapNW + 1) * sizeof(int);
    const int grid = (int)maps->shape[0];
#define CL_MAPS(T) rc = launch_cl_maps<T>(image, g, nwh, lds, grid, (uint16_t *)maps->data, s)
    CL_BY_DTYPE(CL_MAPS);
#undef CL_MAPS
    if (rc) return rc;
    note_kernel("mi::clahe_maps_kernel<%s> grid=%d bins=%d %s (one workgroup per contextual region: histogram, clip and mapping in LDS)",
                cl_dtype_name(image->dtype), grid, nbins, nwh > 1 ? "per-wave histograms" : "shared histogram");
    return MI_OK;
}

extern "C" int mi_clahe_apply(const mi_array *image, const int *kernel, double umin, double umax, int nbins, const mi_array *maps,
                              const mi_array *out, void *work_dev, mi_stream stream)
{
    ClGeom g;
    int rc;
    if ((rc = cl_geom(image, kernel, umin, umax, nbins, 1, maps, &g)) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(same_shape(image, out) && out->dtype == MI_U16 && is_contiguous(out), MI_ERR_INVALID_ARG,
               "out must be C-contiguous uint16 of the image's shape");
    MI_REQUIRE(out->data != image->data, MI_ERR_INVALID_ARG, "out may not be the image");
    hipStream_t s = resolve_stream(stream);
    const uint16_t *mp = (const uint16_t *)maps->data;
    uint16_t *op = (uint16_t *)out->data;
    uint32_t *work = (uint32_t *)work_dev;
    int ksum = 0;
    for (int a = 0; a < g.nd; a++) ksum += g.k[a];
    const size_t stage = ((size_t)nbins << g.nd) * sizeof(uint16_t);
    if (!g_cl_generic && (g.nd == 2 || g.nd == 3) && stage <= (size_t)kClStageBytes && ksum <= kClCoefMax) {
        ClApply p;
        int64_t cells = 1;
        for (int a = 0; a < g.nd; a++) {
            p.ncell[a] = g.nr[a] + 1;
            cells *= p.ncell[a];
        }
        // slabs along axis 0 of a cell: enough workgroups to fill the device several times over, as long as a workgroup
        // keeps some 4096 voxels to pay for staging the mappings
        int64_t want = std::max<int64_t>(1, std::min<int64_t>((8192 + cells - 1) / cells, ((int64_t)g.npix + 4095) / 4096));
        want = std::min<int64_t>(want, g.k[0]);
        p.slab = (int)((g.k[0] + want - 1) / want);
        p.slabs = (g.k[0] + p.slab - 1) / p.slab;
        if (cells * p.slabs < ((int64_t)1 << 31)) {
            const int grid = (int)(cells * p.slabs);
            const size_t lds = (size_t)ksum * sizeof(double) + stage;
#define CL_APPLY(T)                                                                                   \
    rc = g.nd == 3 ? launch_cl_apply<T, 3>(image, g, p, lds, grid, mp, op, work, s)                   \
                   : launch_cl_apply<T, 2>(image, g, p, lds, grid, mp, op, work, s)
            CL_BY_DTYPE(CL_APPLY);
#undef CL_APPLY
            if (rc) return rc;
            note_kernel("mi::clahe_apply_kernel<%s,%d> grid=%d slabs=%d (the %d mappings of a cell and the coefficients in LDS: %zu bytes)",
                        cl_dtype_name(image->dtype), g.nd, grid, p.slabs, 1 << g.nd, lds);
            return MI_OK;
        }
    }
    dim3 grid;
    grid_for(g.total, kClNT, &grid);
#define CL_GEN_ND(T, ND) \
    hipLaunchKernelGGL((clahe_generic_kernel<T, ND>), grid, dim3(kClNT), 0, s, (const T *)image->data, g, mp, op, work)
#define CL_GEN(T)                                   \
    do {                                            \
        switch (g.nd) {                             \
        case 1: CL_GEN_ND(T, 1); break;             \
        case 2: CL_GEN_ND(T, 2); break;             \
        case 3: CL_GEN_ND(T, 3); break;             \
        default: CL_GEN_ND(T, 4); break;            \
        }                                           \
    } while (0)
    CL_BY_DTYPE(CL_GEN);
#undef CL_GEN
#undef CL_GEN_ND
    MI_HIP(hipGetLastError());
    note_kernel("mi::clahe_generic_kernel<%s,%d> grid=%u (one thread per voxel, mappings from global memory)",
                cl_dtype_name(image->dtype), g.nd, grid.x);
    return MI_OK;
}

extern "C" int mi_clahe_finish(const mi_array *v, const mi_array *out, const void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = check_array(v, "v")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(v->dtype == MI_U16 && out->dtype == MI_F64 && same_shape(v, out), MI_ERR_INVALID_ARG,
               "clahe_finish: uint16 in, float64 out, one shape");
    MI_REQUIRE(is_contiguous(v) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "clahe needs C-contiguous arrays");
    const int64_t total = numel(v);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    dim3 grid;
    grid_for(total, kClNT, &grid);
    hipLaunchKernelGGL(clahe_finish_kernel, grid, dim3(kClNT), 0, s, (const uint16_t *)v->data, (double *)out->data, total,
                       (const uint32_t *)work_dev);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_interp_map(const mi_array *image, const mi_array *xp, const mi_array *fp, const mi_array *out, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(xp, "xp")) || (rc = check_array(fp, "fp")) || (rc = check_array(out, "out")))
        return rc;
    MI_REQUIRE(xp->dtype == MI_F64 && fp->dtype == MI_F64 && xp->ndim == 1 && fp->ndim == 1 && xp->shape[0] == fp->shape[0],
               MI_ERR_INVALID_ARG, "interp_map: xp and fp are float64 vectors of one length");
    MI_REQUIRE(xp->shape[0] >= 1 && xp->shape[0] <= MI_INTERP_MAX_KNOTS, MI_ERR_INVALID_ARG, "interp_map: 1 .. 65536 knots");
    MI_REQUIRE(out->dtype == MI_F64 && same_shape(image, out), MI_ERR_INVALID_ARG, "interp_map: out is float64 of the image's shape");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(out) && is_contiguous(xp) && is_contiguous(fp), MI_ERR_NOT_CONTIGUOUS,
               "interp_map needs C-contiguous arrays");
    if (image->dtype != MI_U8 && image->dtype != MI_U16 && image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("interp_map: uint8, uint16, float32 and float64 images only");
        return MI_ERR_UNSUPPORTED;
    }
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int n = (int)xp->shape[0];
    const double *x = (const double *)xp->data, *f = (const double *)fp->data;
    const bool lds = n <= kInterpLdsKnots;
#define CL_INTERP(T) rc = lds ? launch_interp<T, true>(image, out, total, x, f, n, s) : launch_interp<T, false>(image, out, total, x, f, n, s)
    CL_BY_DTYPE(CL_INTERP);
#undef CL_INTERP
    if (rc) return rc;
    note_kernel("mi::interp_map_kernel<%s,%s> knots=%d (numpy.interp through a table)", cl_dtype_name(image->dtype),
                lds ? "LDS" : "global", n);
    return MI_OK;
}

extern "C" int mi_rescale_intensity(const mi_array *image, const mi_array *out, double imin, double imax, double omin, double omax,
                                    mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(same_shape(image, out), MI_ERR_INVALID_ARG, "rescale_intensity: out has the image's shape");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "rescale_intensity needs C-contiguous arrays");
    if (image->dtype == MI_F16 || out->dtype == MI_F16) {
        set_error("float16 arrays are storage only: convert with mi_copy (to float32) around this call");
        return MI_ERR_UNSUPPORTED;
    }
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    dim3 grid;
    grid_for(total, kClNT, &grid);
    const int clip_only = imin == imax;
    if (image->dtype == MI_F32)
        hipLaunchKernelGGL(rescale_kernel<float>, grid, dim3(kClNT), 0, s, image->data, image->dtype, out->data, out->dtype, total,
                           (float)imin, (float)imax, (float)(imax - imin), (float)(omax - omin), (float)omin, (float)omax, clip_only);
    else
        hipLaunchKernelGGL(rescale_kernel<double>, grid, dim3(kClNT), 0, s, image->data, image->dtype, out->data, out->dtype, total,
                           imin, imax, imax - imin, omax - omin, omin, omax, clip_only);
    MI_HIP(hipGetLastError());
    return MI_OK;
}
