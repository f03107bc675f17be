// threshold.hip -- skimage.filters thresholding (cupyimg/skimage/filters/thresholding.py) and the ordering operators of
// core.ndarray.  Built with -ffp-contract=off: every product, sum, quotient and square root is rounded on its own.
//
//   mi_window_mean_std   _mean_std / threshold_niblack / threshold_sauvola (thresholding.py:1003-1179): the sums of x and x^2
//                        over a box window with numpy.pad's 'reflect' border, by index arithmetic.  Ranks 2 and 3:
//                        win_fused_kernel (a tile plus its halo in LDS, the sums formed axis by axis, volumes streamed
//                        plane by plane through a ring of per-plane sums); every other rank: win_generic_kernel (one thread
//                        per output).  Both add the terms of a window in one order -- along the last axis first, each axis
//                        from its lowest index, every partial sum started from 0 -- so they agree bit for bit on floats too.
//   mi_li_sums           one launch per iteration of threshold_li (:636-765): counts and sums of the finite samples above
//                        and at or below a threshold, in a fixed order.
//   mi_min_adjacent_diff the smallest positive gap of a sorted array (threshold_li's default tolerance).
//   mi_multiotsu_search  exhaustive search of threshold_multiotsu (:1230-1341).
//   mi_compare           a > b, a >= b, a < b, a <= b in the common type NumPy picks.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "skimage_common.hpp"

namespace mi {

static Knob g_th_small{0};
static Knob g_th_generic{0};

constexpr int kThNT = 256;
constexpr int kThLdsBytes = 64 * 1024;          // per workgroup, without an attribute: two to three workgroups per CU

// index i of an axis of n samples extended as numpy.pad(mode="reflect") extends it: period 2 (n - 1), an axis of one sample repeats it
template <typename I>
__device__ __forceinline__ I reflect_index(I i, I n)
{
    if (n == 1) return 0;
    const I p = 2 * n - 2;
    if (i < 0) i = -i;
    if (i >= p) i %= p;
    return i < n ? i : p - i;
}

// ------------------------------------------------------------------ window sums
// V = int32_t: the integer dtypes of 16 bits or fewer and bool, summed in integer registers (exact); V = double: every
// other dtype, the sample as astype(float64) gives it.
template <typename V> struct WinAcc;
template <> struct WinAcc<int32_t> {
    typedef int64_t S;            // generic kernel
    typedef int32_t FS;           // fused kernel: the planner checked prod(w) * max|x| < 2^31
    typedef uint64_t Q;
    static __device__ __forceinline__ Q sq(int32_t v) { return (Q)((uint32_t)v * (uint32_t)v); }     // |v| < 2^16: below 2^32
};
template <> struct WinAcc<double> {
    typedef double S;
    typedef double FS;
    typedef double Q;
    static __device__ __forceinline__ Q sq(double v) { return v * v; }
};

template <typename V>
__device__ __forceinline__ V win_load(const void *p, int64_t i, int dt)
{
    if constexpr (std::is_same<V, int32_t>::value) {
        switch (dt) {
        case MI_BOOL: return (int32_t)(((const uint8_t *)p)[i] != 0);
        case MI_I8:   return (int32_t)((const int8_t *)p)[i];
        case MI_U8:   return (int32_t)((const uint8_t *)p)[i];
        case MI_I16:  return (int32_t)((const int16_t *)p)[i];
        default:      return (int32_t)((const uint16_t *)p)[i];
        }
    } else {
        return load_as_f64(p, i, dt);
    }
}

struct WinOut {
    int kind;               // 0: mean and standard deviation, 1: Niblack, 2: Sauvola (the kernels' KIND)
    double k, r, n;
    double *o0, *o1;
};

// KIND is a template parameter: with a run-time switch here the compiler merged the three stores into one whose base
// pointer it left unset on the Sauvola path (read in the ISA of the first build; that launch faulted).
template <int KIND>
__device__ __forceinline__ void win_finish(const WinOut &o, int64_t i, double S, double Q)
{
    const double m = S / o.n;
    const double g2 = Q / o.n;
    const double d = g2 - m * m;
    const double s = __builtin_sqrt(d < 0.0 ? 0.0 : d);        // clip(d, 0, None): a NaN stays
    if constexpr (KIND == 0) {
        o.o0[i] = m;
        o.o1[i] = s;
    } else if constexpr (KIND == 1) {
        o.o0[i] = m - o.k * s;
    } else {
        o.o0[i] = m * (1.0 + o.k * (s / o.r - 1.0));
    }
}

struct WinGeom {
    int nd;
    int64_t total;
    int64_t shape[MI_MAX_NDIM];
    int64_t stride[MI_MAX_NDIM];      // elements
    int w[MI_MAX_NDIM];
};

// one thread per output: the window walked as nested loops, one partial sum per axis
template <typename V, int KIND>
__global__ void __launch_bounds__(kThNT) win_generic_kernel(const void *__restrict__ in, int dt, WinGeom g, WinOut o)
{
    typedef typename WinAcc<V>::S ST;
    typedef typename WinAcc<V>::Q QT;
    const int last = g.nd - 1;
    for (int64_t i = (int64_t)blockIdx.x * kThNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kThNT) {
        int64_t c[MI_MAX_NDIM];
        int idx[MI_MAX_NDIM];
        ST accS[MI_MAX_NDIM];
        QT accQ[MI_MAX_NDIM];
        int64_t rem = i;
        for (int d = last; d >= 0; d--) {
            const int64_t q = rem / g.shape[d];
            c[d] = rem - q * g.shape[d] - g.w[d] / 2;           // first sample of the window along d
            rem = q;
            idx[d] = 0;
            accS[d] = 0;
            accQ[d] = 0;
        }
        ST totS = 0;
        QT totQ = 0;
        for (;;) {
            int64_t base = 0;
            for (int d = 0; d < last; d++) base += reflect_index<int64_t>(c[d] + idx[d], g.shape[d]) * g.stride[d];
            ST a = 0;
            QT q = 0;
            for (int t = 0; t < g.w[last]; t++) {
                const V v = win_load<V>(in, base + reflect_index<int64_t>(c[last] + t, g.shape[last]), dt);
                a += v;
                q += WinAcc<V>::sq(v);
            }
            int d = last - 1;
            for (;;) {
                if (d < 0) break;
                accS[d] += a;
                accQ[d] += q;
                if (++idx[d] < g.w[d]) break;
                a = accS[d];
                q = accQ[d];
                accS[d] = 0;
                accQ[d] = 0;
                idx[d] = 0;
                d--;
            }
            if (d < 0) {
                totS = a;
                totQ = q;
                break;
            }
        }
        win_finish<KIND>(o, i, (double)totS, (double)totQ);
    }
}

// Tiles of a 2-D / 3-D array (images: nz = 1): t[0] planes form a chunk a workgroup streams through, t[1] x t[2] is its tile.
struct WinBox {
    int n[3], t[3], nt[3], w[3];
};

static __host__ __device__ inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

template <typename V, int RANK>
static size_t win_lds_bytes(const WinBox &b)
{
    const size_t ey = b.t[1] + b.w[1] - 1, ex = b.t[2] + b.w[2] - 1, tx = b.t[2], ty = b.t[1];
    size_t n = align8(ey * ex * sizeof(V)) + align8(ey * tx * sizeof(typename WinAcc<V>::FS)) + ey * tx * sizeof(typename WinAcc<V>::Q);
    if (RANK == 3) n += (size_t)b.w[0] * ty * tx * (sizeof(typename WinAcc<V>::FS) + sizeof(typename WinAcc<V>::Q));
    return n;
}

// Images: the tile and its halo are staged once, summed along x, then along y, and the thresholds written.  Volumes: a
// workgroup walks the planes of its chunk (plus the halo planes); each plane's tile goes through the same two passes into
// one slot of a ring of w[0] per-plane sums, and an output plane is the sum of the ring's slots from the oldest on.  Every
// window sum is formed afresh: nothing is carried from one output to the next.
template <typename V, int RANK, int KIND>
__global__ void __launch_bounds__(kThNT) win_fused_kernel(const void *__restrict__ in, int dt, WinBox b, int64_t nboxes, WinOut o)
{
    typedef typename WinAcc<V>::FS ST;
    typedef typename WinAcc<V>::Q QT;
    extern __shared__ __align__(16) unsigned char th_lds[];
    const int hz = b.w[0] / 2, hy = b.w[1] / 2, hx = b.w[2] / 2;
    const int tz = b.t[0], ty = b.t[1], tx = b.t[2];
    const int ey = ty + 2 * hy, ex = tx + 2 * hx;
    V *A = (V *)th_lds;
    ST *BS = (ST *)(th_lds + align8((size_t)ey * ex * sizeof(V)));
    QT *BQ = (QT *)((unsigned char *)BS + align8((size_t)ey * tx * sizeof(ST)));
    QT *RQ = BQ + (size_t)ey * tx;                       // ring (volumes only)
    ST *RS = (ST *)(RQ + (size_t)b.w[0] * ty * tx);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NW = kThNT / 64;

    for (int64_t box = blockIdx.x; box < nboxes; box += gridDim.x) {
        const int bx = (int)(box % b.nt[2]);
        const int64_t rest = box / b.nt[2];
        const int by = (int)(rest % b.nt[1]), bz = (int)(rest / b.nt[1]);
        const int z0 = bz * tz, y0 = by * ty, x0 = bx * tx;
        const int zend = min(z0 + tz, b.n[0]);
        const int nplanes = RANK == 3 ? zend - z0 + 2 * hz : 1;
        for (int sz = 0; sz < nplanes; sz++) {
            const int gz = RANK == 3 ? reflect_index<int>(z0 - hz + sz, b.n[0]) : 0;
            // stage the tile and its halo of this plane: a wave takes rows, its lanes along x
            for (int sy = wave; sy < ey; sy += NW) {
                const int gy = reflect_index<int>(y0 - hy + sy, b.n[1]);
                const int64_t row = ((int64_t)gz * b.n[1] + gy) * b.n[2];
                for (int sx = lane; sx < ex; sx += 64)
                    A[sy * ex + sx] = win_load<V>(in, row + reflect_index<int>(x0 - hx + sx, b.n[2]), dt);
            }
            __syncthreads();
            // along x
            for (int sy = wave; sy < ey; sy += NW)
                for (int x = lane; x < tx; x += 64) {
                    const V *p = A + sy * ex + x;
                    ST a = 0;
                    QT q = 0;
                    for (int t = 0; t < b.w[2]; t++) {
                        const V v = p[t];
                        a += v;
                        q += WinAcc<V>::sq(v);
                    }
                    BS[sy * tx + x] = a;
                    BQ[sy * tx + x] = q;
                }
            __syncthreads();
            // along y
            const int slot = RANK == 3 ? sz % b.w[0] : 0;
            for (int y = wave; y < ty; y += NW)
                for (int x = lane; x < tx; x += 64) {
                    ST a = 0;
                    QT q = 0;
                    for (int t = 0; t < b.w[1]; t++) {
                        a += BS[(y + t) * tx + x];
                        q += BQ[(y + t) * tx + x];
                    }
                    if (RANK == 3) {
                        RS[(slot * ty + y) * tx + x] = a;
                        RQ[(slot * ty + y) * tx + x] = q;
                    } else if (y0 + y < b.n[1] && x0 + x < b.n[2]) {
                        win_finish<KIND>(o, (int64_t)(y0 + y) * b.n[2] + x0 + x, (double)a, (double)q);
                    }
                }
            if (RANK == 3) {
                __syncthreads();
                // along z: the planes z0 - hz + sz - (w - 1) .. z0 - hz + sz are in the ring, the oldest in slot (sz + 1) % w
                const int zo = z0 + sz - 2 * hz;
                if (sz >= b.w[0] - 1 && zo < zend)
                    for (int y = wave; y < ty; y += NW)
                        for (int x = lane; x < tx; x += 64) {
                            if (y0 + y >= b.n[1] || x0 + x >= b.n[2]) continue;
                            ST a = 0;
                            QT q = 0;
                            for (int t = 0; t < b.w[0]; t++) {
                                const int sl = (sz + 1 + t) % b.w[0];
                                a += RS[(sl * ty + y) * tx + x];
                                q += RQ[(sl * ty + y) * tx + x];
                            }
                            win_finish<KIND>(o, ((int64_t)zo * b.n[1] + y0 + y) * b.n[2] + x0 + x, (double)a, (double)q);
                        }
                // the next plane's passes write A, B and a ring slot only behind two more barriers
            }
        }
        __syncthreads();
    }
}

// MI_ERR_UNSUPPORTED: not for the fused kernel (an axis of 2^30 samples or more, or no tile fits the LDS budget)
template <typename V, int RANK>
static int win_plan(const mi_array *image, const int *w, bool small, WinBox *b, int64_t *nboxes, size_t *lds)
{
    for (int d = 0; d < 3; d++) {
        const int a = d - (3 - RANK);
        const int64_t n = a < 0 ? 1 : image->shape[a];
        if (n >= ((int64_t)1 << 30)) return MI_ERR_UNSUPPORTED;
        b->n[d] = (int)n;
        b->w[d] = a < 0 ? 1 : w[a];
    }
    b->t[0] = RANK == 3 ? (small ? 2 : 64) : 1;
    b->t[1] = small ? 3 : (RANK == 3 ? 8 : 32);
    b->t[2] = small ? 5 : 64;
    for (int d = 0; d < 3; d++) b->t[d] = std::min(b->t[d], b->n[d]);
    while ((*lds = win_lds_bytes<V, RANK>(*b)) > (size_t)kThLdsBytes) {
        if (b->t[1] > 1) b->t[1] = (b->t[1] + 1) / 2;
        else if (b->t[2] > 1) b->t[2] = (b->t[2] + 1) / 2;
        else return MI_ERR_UNSUPPORTED;
    }
    *nboxes = 1;
    for (int d = 0; d < 3; d++) {
        b->nt[d] = (b->n[d] + b->t[d] - 1) / b->t[d];
        *nboxes *= b->nt[d];
    }
    return MI_OK;
}

template <typename V, int RANK>
static int win_fused(const mi_array *image, const int *w, const WinOut &o, hipStream_t s)
{
    WinBox b;
    int64_t nboxes;
    size_t lds;
    const int rc = win_plan<V, RANK>(image, w, g_th_small != 0, &b, &nboxes, &lds);
    if (rc) return rc;
    const int grid = box_grid(nboxes);
    const void *in = image->data;
    const int dt = (int)image->dtype;
    if (o.kind == 0) hipLaunchKernelGGL((win_fused_kernel<V, RANK, 0>), dim3(grid), dim3(kThNT), lds, s, in, dt, b, nboxes, o);
    else if (o.kind == 1) hipLaunchKernelGGL((win_fused_kernel<V, RANK, 1>), dim3(grid), dim3(kThNT), lds, s, in, dt, b, nboxes, o);
    else hipLaunchKernelGGL((win_fused_kernel<V, RANK, 2>), dim3(grid), dim3(kThNT), lds, s, in, dt, b, nboxes, o);
    MI_HIP(hipGetLastError());
    note_kernel("mi::win_fused_kernel<%s,%d> grid=%d tile=%dx%dx%d window=%dx%dx%d lds=%zu kind=%d", sizeof(V) == 4 ? "int32" : "float64", RANK, grid,
                b.t[0], b.t[1], b.t[2], b.w[0], b.w[1], b.w[2], lds, o.kind);
    return MI_OK;
}

template <typename V>
static int win_generic(const mi_array *image, const int *w, const WinOut &o, hipStream_t s)
{
    WinGeom g;
    memset(&g, 0, sizeof(g));
    g.nd = image->ndim;
    int64_t st = 1;
    for (int d = image->ndim - 1; d >= 0; d--) {
        g.shape[d] = image->shape[d];
        g.stride[d] = st;
        g.w[d] = w[d];
        st *= image->shape[d];
    }
    g.total = st;
    const int grid = capped_grid(g.total, kThNT, 1 << 16);
    const void *in = image->data;
    const int dt = (int)image->dtype;
    if (o.kind == 0) hipLaunchKernelGGL((win_generic_kernel<V, 0>), dim3(grid), dim3(kThNT), 0, s, in, dt, g, o);
    else if (o.kind == 1) hipLaunchKernelGGL((win_generic_kernel<V, 1>), dim3(grid), dim3(kThNT), 0, s, in, dt, g, o);
    else hipLaunchKernelGGL((win_generic_kernel<V, 2>), dim3(grid), dim3(kThNT), 0, s, in, dt, g, o);
    MI_HIP(hipGetLastError());
    note_kernel("mi::win_generic_kernel<%s> grid=%d rank %d kind=%d", sizeof(V) == 4 ? "int32" : "float64", grid, g.nd, o.kind);
    return MI_OK;
}

template <typename V>
static int win_dispatch(const mi_array *image, const int *w, const WinOut &o, bool fused_ok, hipStream_t s)
{
    if (fused_ok && !g_th_generic && (image->ndim == 2 || image->ndim == 3)) {
        const int rc = image->ndim == 3 ? win_fused<V, 3>(image, w, o, s) : win_fused<V, 2>(image, w, o, s);
        if (rc != MI_ERR_UNSUPPORTED) return rc;
    }
    return win_generic<V>(image, w, o, s);
}

// ------------------------------------------------------------------ Li's iteration
// part[0 .. 5]: count above, sum above, count at or below, sum at or below, smallest, largest -- of the finite samples; the
// sums are of (x - shift), rounded to T for floats as NumPy's in-place `image -= image_min` rounds it, and compared with
// the threshold as doubles.  Integers: counts, sums and extrema are int64 (exact); floats: the sums and extrema are doubles.
union LiWord {
    int64_t i;
    double d;
};
struct LiPart {
    LiWord v[6];
};

template <bool INT>
__device__ __forceinline__ void li_merge(LiPart &a, const LiPart &b)
{
    a.v[0].i += b.v[0].i;
    a.v[2].i += b.v[2].i;
    if (INT) {
        a.v[1].i += b.v[1].i;
        a.v[3].i += b.v[3].i;
        a.v[4].i = b.v[4].i < a.v[4].i ? b.v[4].i : a.v[4].i;
        a.v[5].i = b.v[5].i > a.v[5].i ? b.v[5].i : a.v[5].i;
    } else {
        a.v[1].d += b.v[1].d;
        a.v[3].d += b.v[3].d;
        a.v[4].d = fmin(a.v[4].d, b.v[4].d);
        a.v[5].d = fmax(a.v[5].d, b.v[5].d);
    }
}

template <bool INT>
__device__ __forceinline__ LiPart li_empty()
{
    LiPart p;
    for (int k = 0; k < 4; k++) p.v[k].i = 0;           // the bits of 0.0 too
    if (INT) {
        p.v[4].i = INT64_MAX;
        p.v[5].i = INT64_MIN;
    } else {
        p.v[4].d = INFINITY;
        p.v[5].d = -INFINITY;
    }
    return p;
}

// the workgroup's parts, one per thread, folded in a fixed tree: lanes of a wave first, then the waves
template <bool INT>
__device__ __forceinline__ void li_block_reduce(LiPart &mine, LiPart *sh)
{
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int sft = 1; sft < kThNT; sft <<= 1) {
        if ((threadIdx.x & (2 * sft - 1)) == 0) li_merge<INT>(sh[threadIdx.x], sh[threadIdx.x + sft]);
        __syncthreads();
    }
    mine = sh[0];
}

template <typename T, bool INT>
__global__ void __launch_bounds__(kThNT) li_partial_kernel(const T *__restrict__ x, int64_t n, double thr, double shift, int64_t shift_i,
                                                           LiPart *__restrict__ part)
{
    __shared__ LiPart sh[kThNT];
    LiPart p = li_empty<INT>();
    const T sh_t = (T)shift;
    for (int64_t i = (int64_t)blockIdx.x * kThNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThNT) {
        const T v = x[i];
        if constexpr (INT) {
            const int64_t sv = (int64_t)v - shift_i;
            if ((double)sv > thr) {
                p.v[0].i += 1;
                p.v[1].i += sv;
            } else {
                p.v[2].i += 1;
                p.v[3].i += sv;
            }
            p.v[4].i = (int64_t)v < p.v[4].i ? (int64_t)v : p.v[4].i;
            p.v[5].i = (int64_t)v > p.v[5].i ? (int64_t)v : p.v[5].i;
        } else {
            if (!(fabs((double)v) < INFINITY)) continue;          // NaN and +-inf take no part
            const T sv = v - sh_t;
            if ((double)sv > thr) {
                p.v[0].i += 1;
                p.v[1].d += (double)sv;
            } else {
                p.v[2].i += 1;
                p.v[3].d += (double)sv;
            }
            p.v[4].d = fmin(p.v[4].d, (double)v);
            p.v[5].d = fmax(p.v[5].d, (double)v);
        }
    }
    li_block_reduce<INT>(p, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

template <bool INT>
__global__ void __launch_bounds__(kThNT) li_final_kernel(const LiPart *__restrict__ part, int nparts, LiPart *__restrict__ out)
{
    __shared__ LiPart sh[kThNT];
    LiPart p = li_empty<INT>();
    for (int k = threadIdx.x; k < nparts; k += kThNT) li_merge<INT>(p, part[k]);
    li_block_reduce<INT>(p, sh);
    if (threadIdx.x == 0) *out = p;
}

// smallest positive x[i + 1] - x[i] of a sorted array, as a double (+inf: none); floats: the gap of the shifted samples, in T
template <typename T, bool INT>
__global__ void __launch_bounds__(kThNT) min_gap_kernel(const T *__restrict__ x, int64_t n, double shift, double *__restrict__ part)
{
    __shared__ double sh[kThNT];
    double best = INFINITY;
    const T sh_t = (T)shift;
    for (int64_t i = (int64_t)blockIdx.x * kThNT + threadIdx.x; i + 1 < n; i += (int64_t)gridDim.x * kThNT) {
        const T a = x[i], b = x[i + 1];
        if constexpr (INT) {
            if (b > a) best = fmin(best, (double)((uint64_t)b - (uint64_t)a));
        } else {
            if (!(fabs((double)a) < INFINITY) || !(fabs((double)b) < INFINITY)) continue;
            const T d = (T)(b - sh_t) - (T)(a - sh_t);
            if (d > (T)0) best = fmin(best, (double)d);
        }
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int sft = kThNT / 2; sft > 0; sft >>= 1) {
        if ((int)threadIdx.x < sft) sh[threadIdx.x] = fmin(sh[threadIdx.x], sh[threadIdx.x + sft]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// ------------------------------------------------------------------ multi-Otsu
// Thresholds t_1 < .. < t_K (bin indices, t_K <= nbins - 2) cut the bins into K + 1 classes; cP / cS: nbins + 1 running sums of
// p and of index * p, from 0.  The objective is the sum over the classes, from the lowest, of S_k^2 / P_k (0 where P_k = 0).
// A workgroup takes a run of the lexicographically ordered prefixes (t_1 .. t_{K-1}); its threads take the values of t_K.
struct MoParams {
    int nbins, K, bits;
    int64_t nprefix, chunk;
};
struct MoBest {
    double val;
    uint64_t key;          // the tuple, `bits` bits per threshold, t_1 in the highest: smaller key = lexicographically smaller tuple
};

__device__ __forceinline__ bool mo_better(const MoBest &a, const MoBest &b) { return a.val > b.val || (a.val == b.val && a.key < b.key); }

__device__ __forceinline__ double mo_term(const double *cP, const double *cS, int lo, int hi)      // bins lo .. hi
{
    const double P = cP[hi + 1] - cP[lo];
    const double S = cS[hi + 1] - cS[lo];
    return P > 0.0 ? S * S / P : 0.0;
}

__device__ __forceinline__ int64_t mo_choose(int64_t n, int k)       // k <= 2
{
    if (n < k) return 0;
    return k == 0 ? 1 : (k == 1 ? n : n * (n - 1) / 2);
}

__device__ __forceinline__ void mo_block_reduce(MoBest &mine, MoBest *sh)
{
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int sft = kThNT / 2; sft > 0; sft >>= 1) {
        if ((int)threadIdx.x < sft && mo_better(sh[threadIdx.x + sft], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + sft];
        __syncthreads();
    }
    mine = sh[0];
}

__global__ void __launch_bounds__(kThNT) multiotsu_kernel(const double *__restrict__ cP, const double *__restrict__ cS, MoParams p,
                                                         MoBest *__restrict__ part)
{
    __shared__ MoBest sh[kThNT];
    MoBest best;
    best.val = -INFINITY;
    best.key = ~(uint64_t)0;
    const int L = p.K - 1;                      // prefix length, 0 .. 3
    const int M = p.nbins - 2;                  // prefix values: 0 .. M - 1
    int t[3] = {0, 0, 0};
    int64_t rank = (int64_t)blockIdx.x * p.chunk;
    const int64_t rend = min(rank + p.chunk, p.nprefix);
    if (rank < rend && L > 0) {
        // unrank: the L-subset of {0 .. M - 1} with `rank` subsets before it
        int64_t rho = rank;
        int x = 0;
        for (int i = 0; i < L; i++) {
            const int k = L - 1 - i;            // thresholds of the prefix still to come
            if (k == 0) {
                x += (int)rho;
            } else {
                for (;;) {
                    const int64_t c = mo_choose(M - 1 - x, k);
                    if (c > rho || x >= M - 1) break;       // (the second: never for a rank below nprefix)
                    rho -= c;
                    x++;
                }
            }
            t[i] = x;
            x++;
        }
    }
    for (; rank < rend; rank++) {
        double base = 0.0;
        uint64_t key = 0;
        int lo = 0;
        for (int i = 0; i < L; i++) {
            base += mo_term(cP, cS, lo, t[i]);
            key = (key << p.bits) | (uint64_t)t[i];
            lo = t[i] + 1;
        }
        if (p.K > 1) key <<= p.bits;
        for (int u = lo + (int)(blockIdx.y * kThNT + threadIdx.x); u <= p.nbins - 2; u += (int)gridDim.y * kThNT) {
            MoBest c;
            c.val = base + mo_term(cP, cS, lo, u);
            c.val += mo_term(cP, cS, u + 1, p.nbins - 1);
            c.key = key | (uint64_t)u;
            if (mo_better(c, best)) best = c;
        }
        // the next prefix
        int i = L - 1;
        while (i >= 0 && t[i] == M - L + i) i--;
        if (i < 0) break;
        t[i]++;
        for (int j = i + 1; j < L; j++) t[j] = t[j - 1] + 1;
    }
    mo_block_reduce(best, sh);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = best;
}

__global__ void __launch_bounds__(kThNT) multiotsu_final_kernel(const MoBest *__restrict__ part, int64_t nparts, MoBest *__restrict__ out)
{
    __shared__ MoBest sh[kThNT];
    MoBest best;
    best.val = -INFINITY;
    best.key = ~(uint64_t)0;
    for (int64_t k = threadIdx.x; k < nparts; k += kThNT)
        if (mo_better(part[k], best)) best = part[k];
    mo_block_reduce(best, sh);
    if (threadIdx.x == 0) *out = best;
}

// ------------------------------------------------------------------ comparisons
// An integer of any dtype as a key that orders like its value: (not negative, the two's complement bits)
struct IKey {
    uint32_t hi;
    uint64_t lo;
};
__device__ __forceinline__ bool operator<(const IKey &a, const IKey &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ bool operator>(const IKey &a, const IKey &b) { return b < a; }
__device__ __forceinline__ bool operator<=(const IKey &a, const IKey &b) { return !(b < a); }
__device__ __forceinline__ bool operator>=(const IKey &a, const IKey &b) { return !(a < b); }

template <typename C, typename T>
__device__ __forceinline__ C cmp_conv(T v)
{
    if constexpr (std::is_same<C, IKey>::value) {
        IKey k;
        if constexpr (std::is_floating_point<T>::value) {
            k.hi = 0;
            k.lo = 0;                                   // never dispatched
        } else if constexpr (std::is_signed<T>::value) {
            k.hi = v >= 0;
            k.lo = (uint64_t)(int64_t)v;
        } else {
            k.hi = 1;
            k.lo = (uint64_t)v;
        }
        return k;
    } else {
        return (C)v;
    }
}

template <typename C>
__device__ __forceinline__ C cmp_load(const void *p, int64_t i, int dt)
{
    switch (dt) {
    case MI_BOOL: return cmp_conv<C, uint8_t>((uint8_t)(((const uint8_t *)p)[i] != 0));
    case MI_I8:   return cmp_conv<C, int8_t>(((const int8_t *)p)[i]);
    case MI_U8:   return cmp_conv<C, uint8_t>(((const uint8_t *)p)[i]);
    case MI_I16:  return cmp_conv<C, int16_t>(((const int16_t *)p)[i]);
    case MI_U16:  return cmp_conv<C, uint16_t>(((const uint16_t *)p)[i]);
    case MI_I32:  return cmp_conv<C, int32_t>(((const int32_t *)p)[i]);
    case MI_U32:  return cmp_conv<C, uint32_t>(((const uint32_t *)p)[i]);
    case MI_I64:  return cmp_conv<C, int64_t>(((const int64_t *)p)[i]);
    case MI_U64:  return cmp_conv<C, uint64_t>(((const uint64_t *)p)[i]);
    case MI_F32:  return cmp_conv<C, float>(((const float *)p)[i]);
    default:      return cmp_conv<C, double>(((const double *)p)[i]);
    }
}

template <typename C>
__device__ __forceinline__ uint8_t cmp_apply(int op, const C &a, const C &b)
{
    switch (op) {
    case 0:  return a > b;
    case 1:  return a >= b;
    case 2:  return a < b;
    default: return a <= b;
    }
}

template <typename T, int N>
struct alignas(sizeof(T) * N) CmpVec {
    T v[N];
};

// array against a scalar; VEC = 4: four samples per thread from one aligned load, one 4-byte store
template <typename T, typename C, int VEC>
__global__ void __launch_bounds__(kThNT) cmp_scalar_kernel(const T *__restrict__ a, int64_t n, int op, C b, uint8_t *__restrict__ out)
{
    const int64_t groups = (n + VEC - 1) / VEC;
    for (int64_t g = (int64_t)blockIdx.x * kThNT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThNT) {
        const int64_t i = g * VEC;
        if (VEC == 4 && i + 4 <= n) {
            const CmpVec<T, 4> x = *reinterpret_cast<const CmpVec<T, 4> *>(a + i);
            CmpVec<uint8_t, 4> r;
#pragma unroll
            for (int k = 0; k < 4; k++) r.v[k] = cmp_apply<C>(op, cmp_conv<C, T>(x.v[k]), b);
            *reinterpret_cast<CmpVec<uint8_t, 4> *>(out + i) = r;
        } else {
            for (int64_t j = i; j < n && j < i + VEC; j++) out[j] = cmp_apply<C>(op, cmp_conv<C, T>(a[j]), b);
        }
    }
}

template <typename C>
__global__ void __launch_bounds__(kThNT) cmp_array_kernel(const void *__restrict__ a, int adt, const void *__restrict__ b, int bdt, int64_t n, int op,
                                                         uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kThNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThNT)
        out[i] = cmp_apply<C>(op, cmp_load<C>(a, i, adt), cmp_load<C>(b, i, bdt));
}

static bool is_float_dtype(int dt) { return dt == MI_F32 || dt == MI_F64 || dt == MI_F16; }
static bool fits_float32(int dt) { return dt == MI_BOOL || dt == MI_I8 || dt == MI_U8 || dt == MI_I16 || dt == MI_U16 || dt == MI_F32; }

template <typename C>
static int cmp_scalar_launch(const mi_array *a, int op, C b, uint8_t *out, int64_t n, hipStream_t s)
{
    return dispatch_dtype(a->dtype, [&]<typename T0>() -> int {
        typedef typename std::conditional<std::is_same<T0, bool>::value, uint8_t, T0>::type T;      // bool arrays hold 0 and 1
        const bool vec = !((uintptr_t)a->data % (4 * sizeof(T))) && !((uintptr_t)out % 4);
        const int grid = capped_grid(vec ? (n + 3) / 4 : n, kThNT, 1 << 16);
        if (vec) hipLaunchKernelGGL((cmp_scalar_kernel<T, C, 4>), dim3(grid), dim3(kThNT), 0, s, (const T *)a->data, n, op, b, out);
        else hipLaunchKernelGGL((cmp_scalar_kernel<T, C, 1>), dim3(grid), dim3(kThNT), 0, s, (const T *)a->data, n, op, b, out);
        MI_HIP(hipGetLastError());
        note_kernel("mi::cmp_scalar_kernel grid=%d vec=%d (one launch)", grid, vec ? 4 : 1);
        return MI_OK;
    });
}

template <typename C>
static int cmp_array_launch(const mi_array *a, const mi_array *b, int op, uint8_t *out, int64_t n, hipStream_t s)
{
    const int grid = capped_grid(n, kThNT, 1 << 16);
    hipLaunchKernelGGL((cmp_array_kernel<C>), dim3(grid), dim3(kThNT), 0, s, (const void *)a->data, (int)a->dtype, (const void *)b->data, (int)b->dtype, n, op, out);
    MI_HIP(hipGetLastError());
    note_kernel("mi::cmp_array_kernel grid=%d (one launch)", grid);
    return MI_OK;
}

static int read_back(void *host, const void *dev, size_t nbytes, hipStream_t s)
{
    hipError_t e = hipMemcpyAsync(host, dev, nbytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error("HIP error: %s", hipGetErrorString(e));
        return MI_ERR_INTERNAL;
    }
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_threshold(int small_tiles, int force_generic)
{
    g_th_small = small_tiles != 0;
    g_th_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_window_mean_std(const mi_array *image, const int *window, int kind, double k, double r, const mi_array *out0,
                                  const mi_array *out1, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(out0, "out0"))) return rc;
    MI_REQUIRE(kind >= 0 && kind <= 2 && window, MI_ERR_INVALID_ARG, "window_mean_std: kind 0 (mean and deviation), 1 (Niblack) or 2 (Sauvola)");
    MI_REQUIRE((out1 != nullptr) == (kind == 0), MI_ERR_INVALID_ARG, "window_mean_std: a second output for kind 0 only");
    if (out1 && (rc = check_array(out1, "out1"))) return rc;
    const int rank = image->ndim;
    MI_REQUIRE(rank >= 1, MI_ERR_INVALID_ARG, "window_mean_std: arrays of rank 1 to 8");
    MI_REQUIRE(image->dtype != MI_F16, MI_ERR_INVALID_ARG, "window_mean_std: float16 arrays are storage only (the caller converts)");
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "window_mean_std needs a C-contiguous image");
    double nwin = 1.0;
    for (int d = 0; d < rank; d++) {
        MI_REQUIRE(window[d] >= 1 && (window[d] & 1), MI_ERR_INVALID_ARG, "window_mean_std: odd window sizes of at least 1");
        nwin *= (double)window[d];
    }
    MI_REQUIRE(nwin < 2147483648.0, MI_ERR_INVALID_ARG, "window_mean_std: windows of fewer than 2^31 samples");
    for (const mi_array *o : {out0, out1})
        MI_REQUIRE(!o || (o->dtype == MI_F64 && same_shape(o, image) && is_contiguous(o)), MI_ERR_INVALID_ARG,
                   "window_mean_std: C-contiguous float64 outputs of the image's shape");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    const char *ib = (const char *)image->data;
    const int64_t ibytes = total * (int64_t)dtype_size(image->dtype);
    for (const mi_array *o : {out0, out1})
        MI_REQUIRE(!o || !(ib < (const char *)o->data + total * 8 && (const char *)o->data < ib + ibytes), MI_ERR_INVALID_ARG,
                   "window_mean_std: the outputs may not share memory with the image");
    MI_REQUIRE(!out1 || out1->data != out0->data, MI_ERR_INVALID_ARG, "window_mean_std: two outputs, two arrays");
    WinOut o;
    o.kind = kind;
    o.k = k;
    o.r = r;
    o.n = nwin;
    o.o0 = (double *)out0->data;
    o.o1 = out1 ? (double *)out1->data : nullptr;
    hipStream_t s = resolve_stream(stream);
    double maxabs = 0.0;
    switch (image->dtype) {
    case MI_BOOL: maxabs = 1.0; break;
    case MI_I8:   maxabs = 128.0; break;
    case MI_U8:   maxabs = 255.0; break;
    case MI_I16:  maxabs = 32768.0; break;
    case MI_U16:  maxabs = 65535.0; break;
    default: break;
    }
    if (maxabs > 0.0) return win_dispatch<int32_t>(image, window, o, nwin * maxabs < 2147483648.0, s);
    return win_dispatch<double>(image, window, o, true, s);
}

extern "C" int mi_li_sums(const mi_array *image, double threshold, double shift, int64_t shift_int, void *result, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image"))) return rc;
    MI_REQUIRE(result, MI_ERR_INVALID_ARG, "li_sums: no result");
    MI_REQUIRE(image->dtype != MI_F16 && image->dtype != MI_BOOL && image->dtype != MI_U64, MI_ERR_INVALID_ARG,
               "li_sums: float16, bool and uint64 images are converted by the caller");
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "li_sums needs a C-contiguous image");
    const int64_t n = numel(image);
    const bool is_int = !is_float_dtype(image->dtype);
    hipStream_t s = resolve_stream(stream);
    // the number of workgroups is a function of the size alone: the order of the sums, and with it their bits, is fixed
    const int blocks = capped_grid(n, kThNT * 8, 1024);
    void *part = nullptr;
    if ((rc = pool_alloc(&part, (size_t)(blocks + 1) * sizeof(LiPart), s))) return rc;
    LiPart *parts = (LiPart *)part;
    rc = dispatch_dtype(image->dtype, [&]<typename T>() -> int {
        if constexpr (std::is_same<T, bool>::value || std::is_same<T, uint64_t>::value) {
            return MI_ERR_INVALID_ARG;
        } else {
            constexpr bool INT = !std::is_floating_point<T>::value;
            hipLaunchKernelGGL((li_partial_kernel<T, INT>), dim3(blocks), dim3(kThNT), 0, s, (const T *)image->data, n, threshold, shift, shift_int, parts);
            hipLaunchKernelGGL((li_final_kernel<INT>), dim3(1), dim3(kThNT), 0, s, (const LiPart *)parts, blocks, parts + blocks);
            MI_HIP(hipGetLastError());
            return MI_OK;
        }
    });
    if (rc == MI_OK) rc = read_back(result, parts + blocks, sizeof(LiPart), s);
    pool_free(part);
    if (rc == MI_OK) note_kernel("mi::li_partial_kernel<%s> grid=%d + li_final_kernel (two launches, 48 bytes read)", is_int ? "int64" : "float64", blocks);
    return rc;
}

extern "C" int mi_min_adjacent_diff(const mi_array *sorted, double shift, double *result, mi_stream stream)
{
    int rc;
    if ((rc = check_array(sorted, "sorted"))) return rc;
    MI_REQUIRE(result, MI_ERR_INVALID_ARG, "min_adjacent_diff: no result");
    MI_REQUIRE(sorted->dtype != MI_F16 && sorted->dtype != MI_BOOL, MI_ERR_INVALID_ARG, "min_adjacent_diff: float16 and bool arrays are converted by the caller");
    MI_REQUIRE(is_contiguous(sorted), MI_ERR_NOT_CONTIGUOUS, "min_adjacent_diff needs a C-contiguous array");
    const int64_t n = numel(sorted);
    *result = INFINITY;
    if (n < 2) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int blocks = capped_grid(n, kThNT * 8, 1024);
    void *part = nullptr;
    if ((rc = pool_alloc(&part, (size_t)blocks * sizeof(double), s))) return rc;
    rc = dispatch_dtype(sorted->dtype, [&]<typename T>() -> int {
        if constexpr (std::is_same<T, bool>::value) {
            return MI_ERR_INVALID_ARG;
        } else {
            constexpr bool INT = !std::is_floating_point<T>::value;
            hipLaunchKernelGGL((min_gap_kernel<T, INT>), dim3(blocks), dim3(kThNT), 0, s, (const T *)sorted->data, n, shift, (double *)part);
            MI_HIP(hipGetLastError());
            return MI_OK;
        }
    });
    if (rc == MI_OK) {
        std::vector<double> host((size_t)blocks);
        rc = read_back(host.data(), part, host.size() * sizeof(double), s);
        if (rc == MI_OK)
            for (double v : host) *result = std::min(*result, v);
    }
    pool_free(part);
    return rc;
}

extern "C" int mi_multiotsu_search(const double *cum_p, const double *cum_s, int nbins, int classes, int64_t *thresholds, double *best, mi_stream stream)
{
    MI_REQUIRE(cum_p && cum_s && thresholds, MI_ERR_INVALID_ARG, "multiotsu_search: no tables");
    MI_REQUIRE(classes >= 2 && classes <= 5, MI_ERR_INVALID_ARG, "multiotsu_search: 2 to 5 classes");
    MI_REQUIRE(nbins >= classes && nbins <= (1 << 26), MI_ERR_INVALID_ARG, "multiotsu_search: at least as many bins as classes, at most 2^26");
    const int K = classes - 1, L = K - 1;
    // tuples: C(nbins - 1, K); prefixes: C(nbins - 2, L)
    double tuples = 1.0;
    for (int i = 0; i < K; i++) tuples = tuples * (double)(nbins - 1 - i) / (double)(i + 1);
    MI_REQUIRE(tuples <= 17179869184.0 * (1.0 + 1e-12), MI_ERR_INVALID_ARG, "multiotsu_search: more than 2^34 threshold tuples");
    MoParams p;
    p.nbins = nbins;
    p.K = K;
    p.bits = 64 / K;
    MI_REQUIRE(p.bits >= 27 || (nbins >> p.bits) == 0, MI_ERR_INVALID_ARG, "multiotsu_search: too many bins for this number of classes");
    p.nprefix = 1;
    for (int i = 0; i < L; i++) p.nprefix = p.nprefix * (nbins - 2 - i) / (i + 1);       // a binomial at every step: the division is exact
    const int gx = (int)std::min<int64_t>(p.nprefix, 8192);
    p.chunk = (p.nprefix + gx - 1) / gx;
    const int gy = L == 0 ? (int)std::max<int64_t>(1, std::min<int64_t>(64, (nbins + kThNT * 16 - 1) / (kThNT * 16))) : 1;
    hipStream_t s = resolve_stream(stream);
    int rc;
    Scratch tp, ts;
    const size_t tbytes = (size_t)(nbins + 1) * sizeof(double);
    if ((rc = tp.upload(cum_p, tbytes, s)) || (rc = ts.upload(cum_s, tbytes, s))) return rc;
    const int64_t nparts = (int64_t)gx * gy;
    void *part = nullptr;
    if ((rc = pool_alloc(&part, (size_t)(nparts + 1) * sizeof(MoBest), s))) return rc;
    MoBest *parts = (MoBest *)part;
    hipLaunchKernelGGL(multiotsu_kernel, dim3(gx, gy), dim3(kThNT), 0, s, (const double *)tp.ptr, (const double *)ts.ptr, p, parts);
    hipLaunchKernelGGL(multiotsu_final_kernel, dim3(1), dim3(kThNT), 0, s, (const MoBest *)parts, nparts, parts + nparts);
    MoBest got;
    got.val = 0.0;
    got.key = 0;
    const hipError_t e = hipGetLastError();
    rc = e == hipSuccess ? read_back(&got, parts + nparts, sizeof(MoBest), s) : hip_fail(e, "multiotsu_kernel");
    pool_free(part);
    if (rc) return rc;
    const uint64_t mask = p.bits == 64 ? ~(uint64_t)0 : (((uint64_t)1 << p.bits) - 1);
    for (int i = 0; i < K; i++) thresholds[i] = (int64_t)((got.key >> (p.bits * (K - 1 - i))) & mask);
    if (best) *best = got.val;
    note_kernel("mi::multiotsu_kernel grid=%dx%d classes=%d bins=%d prefixes=%lld + multiotsu_final_kernel", gx, gy, classes, nbins, (long long)p.nprefix);
    return MI_OK;
}

extern "C" int mi_compare(int op, const mi_array *a, const mi_array *b, int ctype, double scalar, int scalar_hi, uint64_t scalar_lo,
                          const mi_array *out, mi_stream stream)
{
    int rc;
    if ((rc = check_array(a, "a")) || (rc = check_array(out, "out"))) return rc;
    if (b && (rc = check_array(b, "b"))) return rc;
    MI_REQUIRE(op >= 0 && op <= 3, MI_ERR_INVALID_ARG, "compare: op 0 (>), 1 (>=), 2 (<) or 3 (<=)");
    MI_REQUIRE(ctype >= 0 && ctype <= 2, MI_ERR_INVALID_ARG, "compare: common type 0 (integer), 1 (float32) or 2 (float64)");
    MI_REQUIRE(scalar_hi >= 0 && scalar_hi <= 2, MI_ERR_INVALID_ARG, "compare: the integer scalar's high word is 0, 1 or 2");
    MI_REQUIRE(a->dtype != MI_F16 && (!b || b->dtype != MI_F16), MI_ERR_INVALID_ARG, "compare: float16 arrays are storage only (the caller converts)");
    MI_REQUIRE(out->dtype == MI_BOOL && same_shape(out, a) && is_contiguous(out), MI_ERR_INVALID_ARG, "compare: a C-contiguous bool output of the operand's shape");
    MI_REQUIRE(is_contiguous(a) && (!b || (is_contiguous(b) && same_shape(a, b))), MI_ERR_NOT_CONTIGUOUS, "compare: C-contiguous operands of one shape");
    for (const mi_array *x : {a, b}) {
        if (!x) continue;
        MI_REQUIRE(ctype != 0 || !is_float_dtype(x->dtype), MI_ERR_INVALID_ARG, "compare: the integer comparison takes integer and bool operands");
        MI_REQUIRE(ctype != 1 || fits_float32(x->dtype), MI_ERR_INVALID_ARG, "compare: the float32 comparison takes operands float32 holds exactly");
    }
    const int64_t n = numel(a);
    if (n == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    uint8_t *o = (uint8_t *)out->data;
    if (b) {
        if (ctype == 0) return cmp_array_launch<IKey>(a, b, op, o, n, s);
        if (ctype == 1) return cmp_array_launch<float>(a, b, op, o, n, s);
        return cmp_array_launch<double>(a, b, op, o, n, s);
    }
    if (ctype == 0) {
        IKey key;
        key.hi = (uint32_t)scalar_hi;
        key.lo = scalar_lo;
        return cmp_scalar_launch<IKey>(a, op, key, o, n, s);
    }
    if (ctype == 1) return cmp_scalar_launch<float>(a, op, (float)scalar, o, n, s);
    return cmp_scalar_launch<double>(a, op, scalar, o, n, s);
}
