// regionprops.hip -- what callers do next with a label image: bound the regions (scipy.ndimage.find_objects), describe them
// (skimage.measure.regionprops / regionprops_table; reference cupyimg/skimage/measure/_regionprops.py, _moments.py) and drop
// the small ones (skimage.morphology.remove_small_objects / remove_small_holes; reference morphology/misc.py:51-245).
//
// Three rules hold for every kernel of this file:
//   * no workgroup waits on another one inside a kernel: every dependency between workgroups is a launch boundary
//     (extent pass | centres | moment pass | finish);
//   * the number of launches does not depend on the number of regions: a table row per label, never a launch per label;
//   * every table row a kernel stores to is compared with the table's size first, whatever the label says: labels <= 0 and
//     labels above max_label belong to no region.
// Work blocks and outputs come from the pool uninitialised: the entry points zero (or fill) what they accumulate into.
//
// Tables (row r = label r + 1, R = max_label rows):
//   ext      uint64 (R, 1 + 3 nd): voxel count | smallest index per axis | largest index + 1 per axis | sum of indices per axis
//   centres  float64 (R, 2, nd):   bounding-box origin | centre of the central moments in box coordinates
//   moments  float64 (R, 4^nd):    M[p][q][r] = sum w dz^p dy^q dx^r about a centre (raw: the box origin; central: the centroid)
//   derived  float64 (R, stride):  the columns of rp_finish_kernel, layout in RpCols
//
// Atomic budget (that of meas_kernel, measure.hip): a wave covers 64 consecutive voxels; runs of equal labels inside the wave
// are reduced by shuffles and only the run's head lane issues atomics -- to per-workgroup copies in LDS below a slot limit
// (then one global atomic per workgroup and slot), straight to global memory above it or after mi_debug_set_regionprops(1).
// The extent pass adds, minimises and maximises integers: its result has no order to depend on.  The moment pass adds doubles:
// exact (any order) while every term and partial sum is an integer below 2^53, else the last bits depend on arrival order.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.hpp"

namespace mi {

static Knob g_rp_global{0};
static std::atomic<int> g_rp_launches{0};

constexpr int kRpLdsExt = 4096;          // uint64 accumulators of the extent pass a workgroup keeps in LDS (32 KiB)
constexpr int kRpLdsMom = 4096;          // double accumulators of the moment pass a workgroup keeps in LDS (32 KiB)
constexpr int64_t kRpMaxRows = 2147483647LL;

#define RP_LAUNCH(kernel, grid, block, stream, ...)                                         \
    do {                                                                                    \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3((unsigned)(block)), 0, stream, __VA_ARGS__); \
        g_rp_launches.fetch_add(1, std::memory_order_relaxed);                              \
    } while (0)

struct RpGeom {
    int ndim;
    int64_t shape[MI_MAX_NDIM];
};

// layout of a row of the derived table, a function of the rank alone (the Python layer computes the same offsets)
struct RpCols {
    int bbox_area, extent, eq_diam, centroid, local_centroid, normalized, hu, inertia, eigvals, major, minor, ecc, orientation, stride;
    __host__ __device__ explicit RpCols(int nd)
    {
        int t = 1;
        for (int d = 0; d < nd; d++) t *= 4;
        bbox_area = 0; extent = 1; eq_diam = 2;
        centroid = 3;
        local_centroid = centroid + nd;
        normalized = local_centroid + nd;
        hu = normalized + t;
        inertia = hu + 7;
        eigvals = inertia + nd * nd;
        major = eigvals + nd;
        minor = major + 1;
        ecc = minor + 1;
        orientation = ecc + 1;
        stride = orientation + 1;
    }
};

struct RpAdd { template <typename V> __device__ V operator()(V a, V b) const { return a + b; } };
struct RpMin { template <typename V> __device__ V operator()(V a, V b) const { return a < b ? a : b; } };
struct RpMax { template <typename V> __device__ V operator()(V a, V b) const { return a > b ? a : b; } };

// segmented reduction inside the wave: after it the first lane of a run holds the run's total; `end` = last lane of the run
template <typename V, typename Op>
__device__ __forceinline__ V rp_run_reduce(V v, int lane, int end, Op op)
{
    for (int d = 1; d < 64; d <<= 1) {
        const V o = __shfl_down(v, d, 64);
        if (lane + d <= end) v = op(v, o);
    }
    return v;
}

static int rp_grid(int64_t n)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)device_cus() * 16));
}

// ------------------------------------------------------------------ pass 1: extents
__global__ void __launch_bounds__(256) rp_init_kernel(unsigned long long *ext, int64_t slots, int W, int nd)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < slots; k += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(k % W);
        ext[k] = (c >= 1 && c <= nd) ? ~0ull : 0ull;
    }
}

template <typename L>
__global__ void __launch_bounds__(256) rp_extent_kernel(const L *__restrict__ lab, int64_t n, RpGeom g, int64_t R, unsigned long long *ext,
                                                        int use_lds)
{
    __shared__ unsigned long long lds[kRpLdsExt];
    const int nd = g.ndim, W = 1 + 3 * nd;
    const int lane = threadIdx.x & 63;
    const int nslot = use_lds ? (int)R * W : 0;          // use_lds: R * W <= kRpLdsExt
    for (int k = threadIdx.x; k < nslot; k += blockDim.x) {
        const int c = k % W;
        lds[k] = (c >= 1 && c <= nd) ? ~0ull : 0ull;
    }
    if (use_lds) __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        long long key = -1;
        if (i < n) {
            const long long v = (long long)lab[i];
            if (v >= 1 && v <= R) key = v - 1;
        }
        const long long nxt = __shfl_down(key, 1, 64);
        const long long prv = __shfl_up(key, 1, 64);
        const unsigned long long ends = __ballot(lane == 63 || nxt != key);
        const int end = __ffsll((long long)(ends & (~0ull << lane))) - 1;
        const bool issue = (lane == 0 || prv != key) && key >= 0;
        // two spellings, so that each address space gets its own atomic instruction (as meas_kernel does)
        unsigned long long *ldst = lds + (issue && use_lds ? key * W : 0);
        unsigned long long *gdst = ext + (issue ? key * W : 0);
        if (issue) {
            const unsigned long long c = (unsigned long long)(end - lane + 1);
            if (use_lds) atomicAdd(&ldst[0], c);
            else atomicAdd(&gdst[0], c);
        }
        int64_t rem = i < n ? i : 0;
        for (int d = nd - 1; d >= 0; d--) {
            const int64_t q = rem / g.shape[d];
            const unsigned long long c = (unsigned long long)(rem - q * g.shape[d]);
            rem = q;
            const unsigned long long lo = rp_run_reduce(c, lane, end, RpMin());
            const unsigned long long hi = rp_run_reduce(c, lane, end, RpMax());
            const unsigned long long sm = rp_run_reduce(c, lane, end, RpAdd());
            if (issue && use_lds) {
                atomicMin(&ldst[1 + d], lo);
                atomicMax(&ldst[1 + nd + d], hi + 1ull);
                atomicAdd(&ldst[1 + 2 * nd + d], sm);
            } else if (issue) {
                atomicMin(&gdst[1 + d], lo);
                atomicMax(&gdst[1 + nd + d], hi + 1ull);
                atomicAdd(&gdst[1 + 2 * nd + d], sm);
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < nslot; k += blockDim.x) {
            const int row = k / W, c = k - row * W;
            if (lds[row * W] == 0ull) continue;                     // this workgroup saw no voxel of the label
            if (c == 0 || c > 2 * nd) atomicAdd(&ext[k], lds[k]);
            else if (c <= nd) atomicMin(&ext[k], lds[k]);
            else atomicMax(&ext[k], lds[k]);
        }
    }
}

// ------------------------------------------------------------------ centres
// origin = the bounding box's first index; centre = the local centroid the reference passes to moments_central:
// M[1, 0, ..] / M[0, 0, ..] of the raw table about the origin -- unweighted the quotient of two exact integers
// (sum - count * origin) / count, weighted the quotient of two entries of the weighted raw table `wraw`
__global__ void __launch_bounds__(256) rp_centres_kernel(const unsigned long long *__restrict__ ext, int64_t R, int nd,
                                                         const double *__restrict__ wraw, int T, double *centres)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int W = 1 + 3 * nd;
    const unsigned long long cnt = ext[r * W];
    int stride = T;
    for (int d = 0; d < nd; d++) {
        stride /= 4;                                                  // the entry with power 1 on axis d alone
        double o = 0.0, c = 0.0;
        if (cnt) {
            const long long mn = (long long)ext[r * W + 1 + d];
            o = (double)mn;
            if (wraw) c = wraw[r * T + stride] / wraw[r * T];
            else c = (double)((long long)ext[r * W + 1 + 2 * nd + d] - (long long)cnt * mn) / (double)(long long)cnt;
        }
        centres[(r * 2 + 0) * nd + d] = o;
        centres[(r * 2 + 1) * nd + d] = c;
    }
}

// ------------------------------------------------------------------ pass 2: moments
// The unit of work is a run: a maximal stretch of equal labels inside one row inside one wave (a wave spans several rows when
// the row is shorter than 64).  The run's four sums over w dx^r come from a segmented shuffle reduction; the head lane
// multiplies them by dy^q (and dz^p) and issues the 4^ND adds.  out[0]: about the box origin; out[1]: about centres[.][1].
template <typename L, int ND>
__global__ void __launch_bounds__(256) rp_moments_kernel(const L *__restrict__ lab, const void *__restrict__ inten, int idt, int64_t n,
                                                         RpGeom g, int64_t R, const double *__restrict__ centres, double *out0,
                                                         double *out1, int use_lds)
{
    constexpr int T = ND == 2 ? 16 : 64;
    __shared__ double lds[kRpLdsMom];
    const int lane = threadIdx.x & 63;
    const int njobs = (out0 ? 1 : 0) + (out1 ? 1 : 0);
    const int nslot = use_lds ? (int)R * T * njobs : 0;               // use_lds: R * T * njobs <= kRpLdsMom
    for (int k = threadIdx.x; k < nslot; k += blockDim.x) lds[k] = 0.0;
    if (use_lds) __syncthreads();
    const int64_t nx = g.shape[ND - 1], ny = g.shape[ND - 2];
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        long long key = -1;
        if (i < n) {
            const long long v = (long long)lab[i];
            if (v >= 1 && v <= R) key = v - 1;
        }
        const int64_t ii = i < n ? i : 0;
        const int64_t row = ii / nx;
        const int64_t x = ii - row * nx;
        const int64_t z = ND == 3 ? row / ny : 0;
        const int64_t y = row - z * ny;
        const long long prv = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || prv != key || x == 0;
        const unsigned long long heads = __ballot(head);
        // last lane of this lane's run: the lane before the next head above this lane
        const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
        const int end = above ? __ffsll((long long)above) - 2 : 63;
        const bool issue = head && key >= 0;
        const double w = key >= 0 ? (inten ? load_as_f64(inten, ii, idt) : 1.0) : 0.0;
        int slot = 0;
#pragma unroll 1
        for (int job = 0; job < 2; job++) {
            double *out = job ? out1 : out0;
            if (!out) continue;
            const double *cz = centres + (key >= 0 ? key * 2 * ND : 0);
            // box coordinates are exact integers in double; the centre is subtracted in double, as the reference does
            const double dx = key >= 0 ? ((double)x - cz[ND - 1]) - (job ? cz[ND + ND - 1] : 0.0) : 0.0;
            const double wx1 = w * dx, dx2 = dx * dx;
            const double wx2 = w * dx2, wx3 = w * (dx2 * dx);
            double s[4];
            s[0] = rp_run_reduce(w, lane, end, RpAdd());
            s[1] = rp_run_reduce(wx1, lane, end, RpAdd());
            s[2] = rp_run_reduce(wx2, lane, end, RpAdd());
            s[3] = rp_run_reduce(wx3, lane, end, RpAdd());
            if (issue) {
                double py[4], pz[4];
                const double dy = ((double)y - cz[ND - 2]) - (job ? cz[ND + ND - 2] : 0.0);
                py[0] = 1.0; py[1] = dy; py[2] = dy * dy; py[3] = py[2] * dy;
                pz[0] = 1.0; pz[1] = pz[2] = pz[3] = 0.0;
                if constexpr (ND == 3) {
                    const double dz = ((double)z - cz[0]) - (job ? cz[ND] : 0.0);
                    pz[1] = dz; pz[2] = dz * dz; pz[3] = pz[2] * dz;
                }
                // two spellings, so that each address space gets its own atomic instruction (as meas_kernel does)
                double *ldst = lds + (use_lds ? ((int64_t)slot * R + key) * T : 0);
                double *gdst = out + key * T;
#pragma unroll
                for (int p = 0; p < (ND == 3 ? 4 : 1); p++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            double t = s[r] * py[q];
                            if constexpr (ND == 3) t = t * pz[p];
                            if (use_lds) atomicAdd(&ldst[(p * 4 + q) * 4 + r], t);
                            else atomicAdd(&gdst[(p * 4 + q) * 4 + r], t);
                        }
            }
            slot++;
        }
    }
    if (use_lds) {
        __syncthreads();
        const int per = (int)R * T;
        for (int k = threadIdx.x; k < nslot; k += blockDim.x) {
            const double v = lds[k];
            if (v == 0.0) continue;                                   // adding +0.0 changes nothing (the tables start at +0.0)
            double *out = out0 ? (k < per ? out0 : out1) : out1;
            atomicAdd(&out[k < per ? k : k - per], v);
        }
    }
}

// ------------------------------------------------------------------ derived columns
// eigenvalues of a symmetric 3 x 3 matrix, decreasing: cyclic Jacobi in Rutishauser's form (the solver of ridges.hip for
// float64, N = 3, written out a second time so that ridges.hip and its helpers sqrt_t / rg_abs stay as they are); 8 sweeps
// at most
__device__ __forceinline__ void rp_eig3(const double *m, double *lam)
{
    double a[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a[r][c] = m[r * 3 + c];
    double d[3], b[3], z[3];
    for (int i = 0; i < 3; i++) d[i] = b[i] = a[i][i];
#pragma unroll 1
    for (int sw = 0; sw < 8; sw++) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off == 0.0) break;
        for (int i = 0; i < 3; i++) z[i] = 0.0;
#pragma unroll
        for (int p = 0; p < 2; p++) {
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double apq = a[p][q];
                if (apq != 0.0) {
                    const double h = d[q] - d[p];
                    const double theta = (0.5 * h) / apq;
                    const double th2 = theta * theta;
                    double t;
                    if (th2 <= std::numeric_limits<double>::max()) {
                        t = 1.0 / (fabs(theta) + sqrt(th2 + 1.0));
                        if (theta < 0.0) t = -t;
                    } else {
                        t = apq / h;
                    }
                    const double c = 1.0 / sqrt(t * t + 1.0);
                    const double s = t * c;
                    const double tau = s / (1.0 + c);
                    const double hh = t * apq;
                    z[p] -= hh; z[q] += hh;
                    d[p] -= hh; d[q] += hh;
                    a[p][q] = 0.0;
                    const int r = 3 - p - q;                          // the third index
                    double &arp = r < p ? a[r][p] : a[p][r];
                    double &arq = r < q ? a[r][q] : a[q][r];
                    const double gg = arp, kk = arq;
                    arp = gg - s * (kk + gg * tau);
                    arq = kk + s * (gg - kk * tau);
                }
            }
        }
        for (int i = 0; i < 3; i++) {
            b[i] += z[i];
            d[i] = b[i];
        }
    }
    for (int pass = 0; pass < 2; pass++)
        for (int j = 0; j < 2 - pass; j++)
            if (d[j] < d[j + 1]) { const double t = d[j]; d[j] = d[j + 1]; d[j + 1] = t; }
    for (int i = 0; i < 3; i++) lam[i] = d[i];
}

// One thread per region; the reference's operation order (_regionprops.py, _moments.py).  raw: the WEIGHTED raw table (null
// for the unweighted columns, whose centroids are quotients of the extent table's integers); central: the central table the
// normalised moments, the Hu set and the inertia tensor come from; null: the row is the short one, `stride` = RpCols::normalized
// doubles (bbox_area .. local_centroid), so that a table of areas, boxes and centroids costs 72 bytes a label and not 768.
template <int ND>
__global__ void __launch_bounds__(256) rp_finish_kernel(const unsigned long long *__restrict__ ext, int64_t R, const double *__restrict__ raw,
                                                        const double *__restrict__ central, double *out, int stride_out)
{
    constexpr int T = ND == 2 ? 16 : 64;
    constexpr int W = 1 + 3 * ND;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const RpCols C(ND);
    double *o = out + r * stride_out;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const unsigned long long *e = ext + r * W;
    const long long cnt = (long long)e[0];
    if (cnt == 0) {
        for (int k = 0; k < stride_out; k++) o[k] = nan;
        return;
    }
    long long box = 1;
    for (int d = 0; d < ND; d++) box *= (long long)e[1 + ND + d] - (long long)e[1 + d];
    o[C.bbox_area] = (double)box;
    o[C.extent] = (double)cnt / (double)box;
    const double PI = 3.141592653589793;
    if (ND == 2) o[C.eq_diam] = sqrt((double)(4 * cnt) / PI);
    else o[C.eq_diam] = pow((double)(2 * ND * cnt) / PI, 1.0 / ND);
    int stride = T;
    for (int d = 0; d < ND; d++) {
        stride /= 4;
        const long long mn = (long long)e[1 + d];
        if (raw) {
            const double lc = raw[r * T + stride] / raw[r * T];
            o[C.local_centroid + d] = lc;
            o[C.centroid + d] = lc + (double)mn;
        } else {
            const long long sm = (long long)e[1 + 2 * ND + d];
            o[C.local_centroid + d] = (double)(sm - cnt * mn) / (double)cnt;
            o[C.centroid + d] = (double)sm / (double)cnt;
        }
    }
    if (!central) return;                   // the short row ends here
    const double *mu = central + r * T;
    const double mu0 = mu[0];
    // moments_normalized: nu[p] = mu[p] / mu0 ** (sum(p) / ndim + 1), NaN below order 2
    double *nu = o + C.normalized;
    for (int k = 0; k < T; k++) {
        const int order = (k & 3) + ((k >> 2) & 3) + ((k >> 4) & 3);
        nu[k] = order < 2 ? nan : mu[k] / pow(mu0, (double)order / (double)ND + 1.0);
    }
    for (int k = 0; k < 7; k++) o[C.hu + k] = nan;
    o[C.ecc] = nan;
    o[C.orientation] = nan;
    double lam[3] = {0.0, 0.0, 0.0};
    double *it = o + C.inertia;
    if constexpr (ND == 2) {
        // Hu's seven invariants, the operation order of skimage's moments_hu
        const double n20 = nu[2 * 4 + 0], n02 = nu[0 * 4 + 2], n11 = nu[1 * 4 + 1];
        const double n30 = nu[3 * 4 + 0], n12 = nu[1 * 4 + 2], n21 = nu[2 * 4 + 1], n03 = nu[0 * 4 + 3];
        double t0 = n30 + n12;
        double t1 = n21 + n03;
        double q0 = t0 * t0;
        double q1 = t1 * t1;
        const double n4 = 4 * n11;
        const double s = n20 + n02;
        const double d = n20 - n02;
        double *hu = o + C.hu;
        hu[0] = s;
        hu[1] = d * d + n4 * n11;
        hu[3] = q0 + q1;
        hu[5] = d * (q0 - q1) + n4 * t0 * t1;
        t0 *= q0 - 3 * q1;
        t1 *= 3 * q0 - q1;
        q0 = n30 - 3 * n12;
        q1 = 3 * n21 - n03;
        hu[2] = q0 * q0 + q1 * q1;
        hu[4] = q0 * t0 + q1 * t1;
        hu[6] = q1 * t0 - q0 * t1;
        // inertia tensor: diag (sum of the second moments - that of the axis) / mu0, off-diagonal -mu11 / mu0
        const double m20 = mu[2 * 4 + 0], m02 = mu[0 * 4 + 2], m11 = mu[1 * 4 + 1];
        const double sum2 = m20 + m02;
        const double a = (sum2 - m20) / mu0, b = -m11 / mu0, c = (sum2 - m02) / mu0;
        it[0] = a; it[1] = b; it[2] = b; it[3] = c;
        // 2 x 2 eigenvalues in closed form (the one of ridges.hip)
        double tmp1 = b * b;
        tmp1 = tmp1 * 4.0;
        double tmp2 = a - c;
        tmp2 = tmp2 * tmp2;
        tmp2 = tmp2 + tmp1;
        tmp2 = sqrt(tmp2);
        tmp2 = tmp2 / 2.0;
        tmp1 = a + c;
        tmp1 = tmp1 / 2.0;
        lam[0] = tmp1 + tmp2;
        lam[1] = tmp1 - tmp2;
        if (a - c == 0.0) o[C.orientation] = b < 0.0 ? -PI / 4.0 : PI / 4.0;
        else o[C.orientation] = 0.5 * atan2(-2 * b, c - a);
    } else {
        const double m200 = mu[2 * 16], m020 = mu[2 * 4], m002 = mu[2];
        const double sum2 = (m200 + m020) + m002;
        it[0] = (sum2 - m200) / mu0;
        it[4] = (sum2 - m020) / mu0;
        it[8] = (sum2 - m002) / mu0;
        it[1] = it[3] = -mu[16 + 4] / mu0;
        it[2] = it[6] = -mu[16 + 1] / mu0;
        it[5] = it[7] = -mu[4 + 1] / mu0;
        rp_eig3(it, lam);
    }
    for (int d = 0; d < ND; d++) {
        if (lam[d] < 0.0) lam[d] = 0.0;                               // numpy.clip(eigvals, 0, None): NaN stays
        o[C.eigvals + d] = lam[d];
    }
    o[C.major] = 4 * sqrt(lam[0]);
    o[C.minor] = 4 * sqrt(lam[ND - 1]);
    if constexpr (ND == 2) o[C.ecc] = lam[0] == 0.0 ? 0.0 : sqrt(1 - lam[1] / lam[0]);
}

// ------------------------------------------------------------------ keep / crop
__device__ __forceinline__ unsigned long long rp_load_bits(const void *p, int64_t i, int size)
{
    switch (size) {
    case 1: return ((const uint8_t *)p)[i];
    case 2: return ((const uint16_t *)p)[i];
    case 4: return ((const uint32_t *)p)[i];
    default: return ((const uint64_t *)p)[i];
    }
}

__device__ __forceinline__ void rp_store_bits(void *p, int64_t i, int size, unsigned long long v)
{
    switch (size) {
    case 1: ((uint8_t *)p)[i] = (uint8_t)v; break;
    case 2: ((uint16_t *)p)[i] = (uint16_t)v; break;
    case 4: ((uint32_t *)p)[i] = (uint32_t)v; break;
    default: ((uint64_t *)p)[i] = v; break;
    }
}

// mode 0: out = src where count[label] >= min_size, else 0 (src and out of one element size)
// mode 1: out = (src == 0) as 0 / 1 (logical_not; no labels)
// mode 2: out = !(count[label] >= min_size) as 0 / 1 (the closing logical_not of remove_small_holes fused into the keep)
template <typename L>
__global__ void __launch_bounds__(256) rp_keep_kernel(const L *__restrict__ lab, const void *__restrict__ src, int ssize, void *out,
                                                      int osize, int64_t n, const unsigned long long *__restrict__ ext, int W, int64_t R,
                                                      unsigned long long min_size, int mode)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (mode == 1) {
            rp_store_bits(out, i, osize, rp_load_bits(src, i, ssize) == 0ull ? 1ull : 0ull);
            continue;
        }
        const long long v = (long long)lab[i];
        const bool keep = v >= 1 && v <= R && ext[(v - 1) * W] >= min_size;
        if (mode == 0) rp_store_bits(out, i, osize, keep ? rp_load_bits(src, i, ssize) : 0ull);
        else rp_store_bits(out, i, osize, keep ? 0ull : 1ull);
    }
}

struct RpBox {
    int ndim;
    int64_t origin[3], box[3], shape[3];
};

// out (the box, C-contiguous) = label_image[slice] == label (bool), or intensity[slice] * that mask (the intensity's dtype)
template <typename L>
__global__ void __launch_bounds__(256) rp_crop_kernel(const L *__restrict__ lab, const void *__restrict__ inten, int isize, long long label,
                                                      RpBox b, int64_t nbox, void *out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nbox; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t rem = k, src = 0, mul = 1;
        for (int d = b.ndim - 1; d >= 0; d--) {
            const int64_t q = rem / b.box[d];
            src += (b.origin[d] + (rem - q * b.box[d])) * mul;
            mul *= b.shape[d];
            rem = q;
        }
        const bool in = (long long)lab[src] == label;
        if (inten) rp_store_bits(out, k, isize, in ? rp_load_bits(inten, src, isize) : 0ull);
        else ((uint8_t *)out)[k] = in ? 1 : 0;
    }
}

// ------------------------------------------------------------------ host side
static int rp_check_labels(const mi_array *labels, int min_rank, int max_rank)
{
    int rc = check_array(labels, "labels");
    if (rc) return rc;
    MI_REQUIRE(labels->dtype == MI_I32 || labels->dtype == MI_I64, MI_ERR_INVALID_ARG, "labels must be int32 or int64");
    MI_REQUIRE(labels->ndim >= min_rank && labels->ndim <= max_rank, MI_ERR_INVALID_ARG, "labels: rank out of range for this entry point");
    MI_REQUIRE(is_contiguous(labels), MI_ERR_NOT_CONTIGUOUS, "labels must be C-contiguous");
    return MI_OK;
}

// ext: uint64 / int64 (R, 1 + 3 nd), C-contiguous
static int rp_check_ext(const mi_array *ext, int nd, int64_t *R)
{
    int rc = check_array(ext, "extents");
    if (rc) return rc;
    MI_REQUIRE((ext->dtype == MI_I64 || ext->dtype == MI_U64) && ext->ndim == 2 && ext->shape[1] == 1 + 3 * nd && is_contiguous(ext),
               MI_ERR_INVALID_ARG, "the extent table is a C-contiguous (max_label, 1 + 3 ndim) int64 array");
    MI_REQUIRE(ext->shape[0] >= 1 && ext->shape[0] <= kRpMaxRows && ext->shape[0] * ext->shape[1] <= kRpMaxRows, MI_ERR_INVALID_ARG,
               "the extent table holds 1 .. 2^31 - 1 entries");
    MI_REQUIRE(ext->data, MI_ERR_INVALID_ARG, "null data pointer");
    *R = ext->shape[0];
    return MI_OK;
}

static int rp_check_table(const mi_array *t, int64_t R, int64_t cols, const char *msg)
{
    int rc = check_array(t, "table");
    if (rc) return rc;
    MI_REQUIRE(t->dtype == MI_F64 && numel(t) == R * cols && is_contiguous(t) && t->data, MI_ERR_INVALID_ARG, msg);
    return MI_OK;
}

static RpGeom rp_geom(const mi_array *a)
{
    RpGeom g = {};
    g.ndim = a->ndim;
    for (int d = 0; d < a->ndim; d++) g.shape[d] = a->shape[d];
    return g;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_regionprops(int force_global)
{
    g_rp_global = force_global != 0;
    return MI_OK;
}

extern "C" int mi_debug_regionprops_launches(void) { return g_rp_launches.load(std::memory_order_relaxed); }

extern "C" int mi_rp_extent(const mi_array *labels, const mi_array *ext, mi_stream stream)
{
    int rc = rp_check_labels(labels, 1, MI_MAX_NDIM);
    if (rc) return rc;
    int64_t R = 0;
    if ((rc = rp_check_ext(ext, labels->ndim, &R))) return rc;
    const int64_t n = numel(labels);
    MI_REQUIRE(n == 0 || labels->data, MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    const int nd = labels->ndim, W = 1 + 3 * nd;
    unsigned long long *e = (unsigned long long *)ext->data;
    dim3 grid;
    grid_for(R * W, 256, &grid);
    RP_LAUNCH(rp_init_kernel, grid.x, 256, s, e, R * W, W, nd);
    const int use_lds = !g_rp_global && R * W <= kRpLdsExt;
    if (n > 0) {
        const RpGeom g = rp_geom(labels);
        if (labels->dtype == MI_I64) RP_LAUNCH(rp_extent_kernel<int64_t>, rp_grid(n), 256, s, (const int64_t *)labels->data, n, g, R, e, use_lds);
        else RP_LAUNCH(rp_extent_kernel<int32_t>, rp_grid(n), 256, s, (const int32_t *)labels->data, n, g, R, e, use_lds);
    }
    MI_HIP(hipGetLastError());
    note_kernel("mi::rp_extent_kernel grid=%d (%lld rows x %d, %s atomics)", rp_grid(n), (long long)R, W, use_lds ? "LDS" : "global");
    return MI_OK;
}

extern "C" int mi_rp_moments(const mi_array *labels, const mi_array *intensity, const mi_array *ext, const mi_array *raw,
                             const mi_array *central, const mi_array *centres, mi_stream stream)
{
    int rc = rp_check_labels(labels, 2, 3);
    if (rc) return rc;
    const int nd = labels->ndim, T = nd == 2 ? 16 : 64;
    int64_t R = 0;
    if ((rc = rp_check_ext(ext, nd, &R))) return rc;
    MI_REQUIRE(raw || central, MI_ERR_INVALID_ARG, "mi_rp_moments: no table to accumulate");
    if (raw && (rc = rp_check_table(raw, R, T, "the raw table is a C-contiguous (max_label, 4^ndim) float64 array"))) return rc;
    if (central && (rc = rp_check_table(central, R, T, "the central table is a C-contiguous (max_label, 4^ndim) float64 array"))) return rc;
    if ((rc = rp_check_table(centres, R, 2 * nd, "the centre table is a C-contiguous (max_label, 2, ndim) float64 array"))) return rc;
    MI_REQUIRE(R * T <= kRpMaxRows, MI_ERR_INVALID_ARG, "the moment tables hold at most 2^31 - 1 entries");
    int idt = 0;
    if (intensity) {
        if ((rc = check_array(intensity, "intensity"))) return rc;
        MI_REQUIRE(intensity->dtype != MI_F16, MI_ERR_INVALID_ARG, "float16 intensity: convert to float32 first");
        MI_REQUIRE(same_shape(intensity, labels) && is_contiguous(intensity), MI_ERR_INVALID_ARG,
                   "the intensity image is C-contiguous of the labels' shape");
        MI_REQUIRE(!central || raw, MI_ERR_INVALID_ARG, "weighted central moments are taken about the weighted raw table's centroid: pass both");
        idt = intensity->dtype;
    }
    const int64_t n = numel(labels);
    MI_REQUIRE(n == 0 || (labels->data && (!intensity || intensity->data)), MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    const size_t tbytes = (size_t)R * T * sizeof(double);
    if (raw) MI_HIP(hipMemsetAsync(raw->data, 0, tbytes, s));
    if (central) MI_HIP(hipMemsetAsync(central->data, 0, tbytes, s));
    const unsigned long long *e = (const unsigned long long *)ext->data;
    double *c = (double *)centres->data;
    double *r0 = raw ? (double *)raw->data : nullptr, *r1 = central ? (double *)central->data : nullptr;
    const void *w = intensity ? intensity->data : nullptr;
    const RpGeom g = rp_geom(labels);
    const int64_t cgrid = (R + 255) / 256;
    int sweeps = 0;
    auto sweep = [&](double *o0, double *o1) {
        if (n == 0) return;
        const int njobs = (o0 ? 1 : 0) + (o1 ? 1 : 0);
        const int use_lds = !g_rp_global && R * T * njobs <= kRpLdsMom;
        const bool l64 = labels->dtype == MI_I64;
        if (nd == 2 && l64) RP_LAUNCH((rp_moments_kernel<int64_t, 2>), rp_grid(n), 256, s, (const int64_t *)labels->data, w, idt, n, g, R, (const double *)c, o0, o1, use_lds);
        else if (nd == 2) RP_LAUNCH((rp_moments_kernel<int32_t, 2>), rp_grid(n), 256, s, (const int32_t *)labels->data, w, idt, n, g, R, (const double *)c, o0, o1, use_lds);
        else if (l64) RP_LAUNCH((rp_moments_kernel<int64_t, 3>), rp_grid(n), 256, s, (const int64_t *)labels->data, w, idt, n, g, R, (const double *)c, o0, o1, use_lds);
        else RP_LAUNCH((rp_moments_kernel<int32_t, 3>), rp_grid(n), 256, s, (const int32_t *)labels->data, w, idt, n, g, R, (const double *)c, o0, o1, use_lds);
        sweeps++;
    };
    RP_LAUNCH(rp_centres_kernel, cgrid, 256, s, e, R, nd, (const double *)nullptr, T, c);
    if (!intensity) {
        sweep(r0, r1);                  // one sweep serves both tables: the centroid is known from the extent table
    } else {
        sweep(r0, nullptr);
        if (central) {
            RP_LAUNCH(rp_centres_kernel, cgrid, 256, s, e, R, nd, (const double *)r0, T, c);
            sweep(nullptr, r1);
        }
    }
    MI_HIP(hipGetLastError());
    note_kernel("mi::rp_moments_kernel<%d> grid=%d (%lld rows x %d%s%s, %s, %d sweep%s, %s atomics)", nd, rp_grid(n), (long long)R, T,
                raw ? " raw" : "", central ? " central" : "", intensity ? "weighted" : "unweighted", sweeps, sweeps == 1 ? "" : "s",
                (!g_rp_global && R * T * ((!intensity && raw && central) ? 2 : 1) <= kRpLdsMom) ? "LDS" : "global");
    return MI_OK;
}

extern "C" int mi_rp_finish(const mi_array *ext, int ndim, const mi_array *raw, const mi_array *central, const mi_array *out, mi_stream stream)
{
    MI_REQUIRE(ndim == 2 || ndim == 3, MI_ERR_INVALID_ARG, "mi_rp_finish: ranks 2 and 3");
    int64_t R = 0;
    int rc = rp_check_ext(ext, ndim, &R);
    if (rc) return rc;
    const int T = ndim == 2 ? 16 : 64;
    const RpCols C(ndim);
    if (raw && (rc = rp_check_table(raw, R, T, "the raw table is a C-contiguous (max_label, 4^ndim) float64 array"))) return rc;
    if (central && (rc = rp_check_table(central, R, T, "the central table is a C-contiguous (max_label, 4^ndim) float64 array"))) return rc;
    const int stride = central ? C.stride : C.normalized;
    if ((rc = rp_check_table(out, R, stride, "the derived table is a C-contiguous (max_label, stride) float64 array: the full row with a central table, the short one without"))) return rc;
    hipStream_t s = resolve_stream(stream);
    const unsigned long long *e = (const unsigned long long *)ext->data;
    const double *r0 = raw ? (const double *)raw->data : nullptr, *r1 = central ? (const double *)central->data : nullptr;
    if (ndim == 2) RP_LAUNCH(rp_finish_kernel<2>, (R + 255) / 256, 256, s, e, R, r0, r1, (double *)out->data, stride);
    else RP_LAUNCH(rp_finish_kernel<3>, (R + 255) / 256, 256, s, e, R, r0, r1, (double *)out->data, stride);
    MI_HIP(hipGetLastError());
    note_kernel("mi::rp_finish_kernel<%d> (%lld rows x %d columns)", ndim, (long long)R, stride);
    return MI_OK;
}

extern "C" int mi_rp_keep(const mi_array *labels, const mi_array *src, const mi_array *ext, int64_t min_size, int mode, const mi_array *out,
                          mi_stream stream)
{
    MI_REQUIRE(mode >= 0 && mode <= 2, MI_ERR_INVALID_ARG, "mi_rp_keep: mode 0 (keep), 1 (logical not), 2 (keep, negated)");
    int rc;
    if ((rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "the output must be C-contiguous");
    const int64_t n = numel(out);
    int64_t R = 0;
    int W = 0;
    if (mode != 1) {
        if ((rc = rp_check_labels(labels, 0, MI_MAX_NDIM))) return rc;
        MI_REQUIRE(numel(labels) == n, MI_ERR_INVALID_ARG, "labels and output differ in size");
        if ((rc = check_array(ext, "extents"))) return rc;
        MI_REQUIRE((ext->dtype == MI_I64 || ext->dtype == MI_U64) && ext->ndim == 2 && is_contiguous(ext) && ext->shape[0] >= 1 &&
                   ext->shape[1] >= 1 && ext->data, MI_ERR_INVALID_ARG, "the extent table is a C-contiguous (max_label, columns) int64 array");
        R = ext->shape[0];
        W = (int)ext->shape[1];
        MI_REQUIRE(min_size >= 0, MI_ERR_INVALID_ARG, "min_size cannot be negative");
    }
    if (mode != 2) {
        if ((rc = check_array(src, "src"))) return rc;
        MI_REQUIRE(is_contiguous(src) && numel(src) == n, MI_ERR_INVALID_ARG, "the source is C-contiguous of the output's size");
        MI_REQUIRE(mode == 1 || dtype_size(src->dtype) == dtype_size(out->dtype), MI_ERR_INVALID_ARG, "source and output differ in element size");
    }
    if (n == 0) return MI_OK;
    MI_REQUIRE(out->data && (mode == 1 || labels->data) && (mode == 2 || src->data), MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    dim3 grid;
    grid_for(n, 256, &grid);
    const void *sp = mode == 2 ? nullptr : src->data;
    const int ssize = mode == 2 ? 1 : (int)dtype_size(src->dtype), osize = (int)dtype_size(out->dtype);
    const unsigned long long *e = mode == 1 ? nullptr : (const unsigned long long *)ext->data;
    if (mode != 1 && labels->dtype == MI_I64)
        RP_LAUNCH(rp_keep_kernel<int64_t>, grid.x, 256, s, (const int64_t *)labels->data, sp, ssize, out->data, osize, n, e, W, R,
                  (unsigned long long)min_size, mode);
    else
        RP_LAUNCH(rp_keep_kernel<int32_t>, grid.x, 256, s, mode == 1 ? nullptr : (const int32_t *)labels->data, sp, ssize, out->data, osize, n, e,
                  W, R, (unsigned long long)min_size, mode);
    MI_HIP(hipGetLastError());
    note_kernel("mi::rp_keep_kernel grid=%d mode=%d", (int)grid.x, mode);
    return MI_OK;
}

extern "C" int mi_rp_crop(const mi_array *labels, const mi_array *intensity, int64_t label, const int64_t *origin, const mi_array *out,
                          mi_stream stream)
{
    int rc = rp_check_labels(labels, 1, 3);
    if (rc) return rc;
    if ((rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(origin, MI_ERR_INVALID_ARG, "mi_rp_crop: no origin");
    MI_REQUIRE(out->ndim == labels->ndim && is_contiguous(out), MI_ERR_INVALID_ARG, "the output is a C-contiguous box of the labels' rank");
    RpBox b = {};
    b.ndim = labels->ndim;
    for (int d = 0; d < b.ndim; d++) {
        b.origin[d] = origin[d];
        b.box[d] = out->shape[d];
        b.shape[d] = labels->shape[d];
        MI_REQUIRE(origin[d] >= 0 && out->shape[d] >= 0 && origin[d] + out->shape[d] <= labels->shape[d], MI_ERR_INVALID_ARG,
                   "the box leaves the label image");
    }
    int isize = 1;
    if (intensity) {
        if ((rc = check_array(intensity, "intensity"))) return rc;
        MI_REQUIRE(same_shape(intensity, labels) && is_contiguous(intensity) && intensity->dtype == out->dtype, MI_ERR_INVALID_ARG,
                   "the intensity image is C-contiguous, of the labels' shape and of the output's dtype");
        isize = (int)dtype_size(intensity->dtype);
    } else {
        MI_REQUIRE(out->dtype == MI_BOOL, MI_ERR_INVALID_ARG, "the region's image is a bool array");
    }
    const int64_t nbox = numel(out);
    if (nbox == 0) return MI_OK;
    MI_REQUIRE(labels->data && out->data && (!intensity || intensity->data), MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    dim3 grid;
    grid_for(nbox, 256, &grid);
    const void *ip = intensity ? intensity->data : nullptr;
    if (labels->dtype == MI_I64) RP_LAUNCH(rp_crop_kernel<int64_t>, grid.x, 256, s, (const int64_t *)labels->data, ip, isize, (long long)label, b, nbox, out->data);
    else RP_LAUNCH(rp_crop_kernel<int32_t>, grid.x, 256, s, (const int32_t *)labels->data, ip, isize, (long long)label, b, nbox, out->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::rp_crop_kernel grid=%d (%lld voxels%s)", (int)grid.x, (long long)nbox, intensity ? ", intensity" : "");
    return MI_OK;
}
