// Labelled reductions (scipy.ndimage.measurements; reference cupyimg/scipy/ndimage/measurements.py:316-1464): sum, mean,
// variance, extrema and their positions, center_of_mass and histogram per label, in float64 (sums) or on order-preserving
// integer keys (extrema).
//
// Index -> slot.  `index` (K int64 values on the device) names the regions.  When its range imax - imin is small (the usual
// arange(1, n + 1) after label) a lookup table lut[v - imin] = smallest k with index[k] == v is built on the device (one
// atomicMin scatter); otherwise the caller passes index sorted and unique and each voxel binary-searches it.  Without an
// index every voxel with label > 0 (labels given; label != 0 for uint64 labels the caller passed as int64) or every voxel
// (no labels) falls in slot 0.
//
// Atomic budget (reduce on chip first, one atomic per destination and workgroup).  A wave covers 64 consecutive voxels; runs of equal slots inside
// the wave are first reduced by shuffles (segmented doubling), and only each run's head lane issues an atomic.  With few
// slots (<= kLdsSlots; center_of_mass: slots x axes <= kLdsCom) the atomics go to per-workgroup copies in LDS and one global atomic per (workgroup, slot) follows;
// with many (a label image of millions of regions) the run heads go straight to global memory.  Float results therefore
// depend on atomic arrival order in their last bits; integer inputs sum exactly below 2**53.
#include <cmath>
#include <string>
#include <vector>
#include "common.hpp"

namespace mi {

constexpr int kLdsSlots = 1024;
constexpr int kLdsCom = 2048;             // LDS accumulators of center_of_mass: slots x axes

enum MeasOp { M_SUMS = 0, M_SSD = 1, M_EXT = 2, M_POS = 3, M_COM = 4, M_HIST = 5 };
enum SlotMode { S_ALL = 0, S_POSITIVE = 1, S_LUT = 2, S_SEARCH = 3, S_NONZERO = 4 };

struct SlotMap {
    int mode;
    int nslot;
    int64_t imin, imax;
    const int *lut;             // S_LUT: imax - imin + 1 entries, >= nslot where the value is absent
    const int64_t *sorted;      // S_SEARCH: nslot sorted unique values
};

struct MeasAcc {
    unsigned long long *cnt;    // M_SUMS
    double *sum;                // M_SUMS, M_COM (sum of values)
    double *ssd;                // M_SSD
    const double *mean;         // M_SSD (per slot)
    unsigned long long *kmin, *kmax;            // M_EXT; read by M_POS
    unsigned long long *pmin, *pmax_first;      // M_POS: smallest index at the extreme
    long long *pmax_last;                       // M_POS: largest NaN index (maximum of a region holding NaN)
    double *com;                // M_COM: nslot x ndim
    unsigned long long *hist;   // M_HIST: nslot x (bins + 1)
    const double *edges;        // M_HIST: bins + 1 float64 edges
    int bins;                   // M_HIST: per slot bins + 1 counters, the last one for values outside the edges
    int ndim;
    int64_t shape[MI_MAX_NDIM];
};

template <typename T> struct is_float_t { static constexpr bool value = std::is_floating_point<T>::value; };

// order-preserving 64-bit key; NaN above everything (maximum: any NaN wins; minimum: NaN only if nothing else).  -0.0 and
// +0.0 share +0.0's key, as they compare equal in SciPy: the first of them in C order is the extreme's position.
template <typename T>
__device__ __forceinline__ unsigned long long to_key(T v)
{
    if constexpr (std::is_floating_point<T>::value) {
        const double d = (double)v;
        if (d != d) return ~0ull;
        const unsigned long long b = d == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(d);
        return (b >> 63) ? ~b : (b | (1ull << 63));
    } else if constexpr (std::is_same<T, uint64_t>::value) {
        return v;
    } else if constexpr (std::is_same<T, bool>::value) {
        return v ? 1ull : 0ull;
    } else {
        return (unsigned long long)(int64_t)v ^ (1ull << 63);
    }
}

template <typename T>
__device__ __forceinline__ T from_key(unsigned long long k)
{
    if constexpr (std::is_floating_point<T>::value) {
        if (k == ~0ull) return (T)NAN;
        const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
        return (T)__longlong_as_double((long long)b);
    } else if constexpr (std::is_same<T, uint64_t>::value) {
        return k;
    } else if constexpr (std::is_same<T, bool>::value) {
        return k != 0;
    } else {
        return (T)(int64_t)(k ^ (1ull << 63));
    }
}

template <typename L>
__device__ __forceinline__ int slot_of(const L *__restrict__ lab, int64_t i, const SlotMap &m)
{
    if (m.mode == S_ALL) return 0;
    const int64_t v = (int64_t)lab[i];
    if (m.mode == S_POSITIVE) return v > 0 ? 0 : -1;
    if (m.mode == S_NONZERO) return v != 0 ? 0 : -1;
    if (v < m.imin || v > m.imax) return -1;
    if (m.mode == S_LUT) {
        const int s = m.lut[v - m.imin];
        return s < m.nslot ? s : -1;
    }
    int lo = 0, hi = m.nslot - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int64_t u = m.sorted[mid];
        if (u == v) return mid;
        if (u < v) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// segmented reduction of a run of equal keys inside the wave: after it the run's first lane holds the run's total.
// `end` = last lane of this lane's run.
template <typename V, typename Op>
__device__ __forceinline__ V run_reduce(V v, int lane, int end, Op op)
{
    for (int d = 1; d < 64; d <<= 1) {
        const V o = __shfl_down(v, d, 64);
        if (lane + d <= end) v = op(v, o);
    }
    return v;
}

struct AddOp { template <typename V> __device__ V operator()(V a, V b) const { return a + b; } };
struct MinOp { template <typename V> __device__ V operator()(V a, V b) const { return a < b ? a : b; } };
struct MaxOp { template <typename V> __device__ V operator()(V a, V b) const { return a > b ? a : b; } };

// scipy.ndimage.histogram = numpy.histogram(values, linspace(min, max, bins + 1)) with these explicit float64 edges:
// bin k holds e[k] <= v < e[k + 1], the last bin is closed (e[n - 1] <= v <= e[n]); values outside [e[0], e[n]] and NaN
// are not counted (returned as n: the slot's "outside" counter).  Every dtype compares in double, as NumPy does against
// float64 edges (exact for every value below 2**53; float32 data converts exactly).
__device__ __forceinline__ int hist_bin(double v, const double *__restrict__ e, int n)
{
    if (!(v >= e[0] && v <= e[n])) return n;
    if (v >= e[n - 1]) return n - 1;
    int lo = 0, hi = n - 2;              // largest k <= n - 2 with e[k] <= v (then v < e[k + 1])
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (e[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T, typename L, int OP>
__global__ void __launch_bounds__(256) meas_kernel(const T *__restrict__ x, const L *__restrict__ lab, int64_t n, SlotMap m,
                                                   MeasAcc acc, int use_lds)
{
    __shared__ double lsum[kLdsSlots];
    __shared__ unsigned long long lcnt[OP == M_COM ? 1 : kLdsSlots];
    __shared__ double lcom[OP == M_COM ? kLdsCom : 1];
    const int lane = threadIdx.x & 63;
    if (use_lds) {
        for (int k = threadIdx.x; k < m.nslot; k += blockDim.x) {
            lsum[k] = 0.0;
            if constexpr (OP != M_COM) lcnt[k] = (OP == M_EXT) ? ~0ull : 0ull;
        }
        if constexpr (OP == M_COM)
            for (int k = threadIdx.x; k < m.nslot * acc.ndim; k += blockDim.x) lcom[k] = 0.0;
        __syncthreads();
    }
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        const int s = i < n ? slot_of(lab, i, m) : -1;
        const T v = i < n ? x[i] : T(0);
        int key = s;
        if constexpr (OP == M_HIST) {
            if (s >= 0) {
                key = s * (acc.bins + 1) + hist_bin((double)v, acc.edges, acc.bins);
            }
        }
        // runs of equal keys inside the wave
        const int nxt = __shfl_down(key, 1, 64);
        const int prv = __shfl_up(key, 1, 64);
        const unsigned long long ends = __ballot(lane == 63 || nxt != key);
        const int end = __ffsll((long long)(ends & (~0ull << lane))) - 1;
        const bool head = lane == 0 || prv != key;
        if constexpr (OP == M_SUMS) {
            const double sv = run_reduce((double)v, lane, end, AddOp());
            const unsigned long long c = (unsigned long long)(end - lane + 1);
            if (head && key >= 0) {
                if (use_lds) { atomicAdd(&lsum[key], sv); atomicAdd(&lcnt[key], c); }
                else { atomicAdd(&acc.sum[key], sv); atomicAdd(&acc.cnt[key], c); }
            }
        } else if constexpr (OP == M_SSD) {
            const double d = key >= 0 ? (double)v - acc.mean[key] : 0.0;
            const double sv = run_reduce(d * d, lane, end, AddOp());
            if (head && key >= 0) {
                if (use_lds) atomicAdd(&lsum[key], sv);
                else atomicAdd(&acc.ssd[key], sv);
            }
        } else if constexpr (OP == M_EXT) {
            const unsigned long long kv = to_key(v);
            const unsigned long long lo = run_reduce(kv, lane, end, MinOp());
            const unsigned long long hi = run_reduce(kv, lane, end, MaxOp());
            if (head && key >= 0) {
                if (use_lds) { atomicMin(&lcnt[key], lo); atomicMax((unsigned long long *)&lsum[key], hi); }
                else { atomicMin(&acc.kmin[key], lo); atomicMax(&acc.kmax[key], hi); }
            }
        } else if constexpr (OP == M_POS) {
            // extremes are settled (previous launch); positions are rare hits: plain per-lane atomics
            if (key >= 0) {
                const unsigned long long kv = to_key(v);
                if (kv == acc.kmin[key]) atomicMin(&acc.pmin[key], (unsigned long long)i);
                if (kv == acc.kmax[key]) {
                    if (is_float_t<T>::value && kv == ~0ull) atomicMax(&acc.pmax_last[key], (long long)i);
                    else atomicMin(&acc.pmax_first[key], (unsigned long long)i);
                }
            }
        } else if constexpr (OP == M_COM) {
            const double dv = (double)v;
            const double sv = run_reduce(dv, lane, end, AddOp());
            if (head && key >= 0) {
                if (use_lds) atomicAdd(&lsum[key], sv);
                else atomicAdd(&acc.sum[key], sv);
            }
            int64_t rem = i;
            for (int d = acc.ndim - 1; d >= 0; d--) {
                const int64_t q = rem / acc.shape[d];
                const double c = (double)(rem - q * acc.shape[d]);
                rem = q;
                const double w = run_reduce(dv * c, lane, end, AddOp());
                if (head && key >= 0) {
                    if (use_lds) atomicAdd(&lcom[key * acc.ndim + d], w);
                    else atomicAdd(&acc.com[(int64_t)key * acc.ndim + d], w);
                }
            }
        } else {   // M_HIST
            const unsigned long long c = (unsigned long long)(end - lane + 1);
            if (head && key >= 0) atomicAdd(&acc.hist[key], c);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < m.nslot; k += blockDim.x) {
            if constexpr (OP == M_SUMS) {
                if (lcnt[k]) { atomicAdd(&acc.sum[k], lsum[k]); atomicAdd(&acc.cnt[k], lcnt[k]); }
            } else if constexpr (OP == M_SSD) {
                if (lsum[k] != 0.0) atomicAdd(&acc.ssd[k], lsum[k]);
            } else if constexpr (OP == M_EXT) {
                const unsigned long long hi = *(unsigned long long *)&lsum[k];
                if (lcnt[k] <= hi) { atomicMin(&acc.kmin[k], lcnt[k]); atomicMax(&acc.kmax[k], hi); }
            } else if constexpr (OP == M_COM) {
                if (lsum[k] != 0.0) atomicAdd(&acc.sum[k], lsum[k]);
                for (int d = 0; d < acc.ndim; d++)
                    if (lcom[k * acc.ndim + d] != 0.0) atomicAdd(&acc.com[(int64_t)k * acc.ndim + d], lcom[k * acc.ndim + d]);
            }
        }
    }
}

// lut[v - imin] = smallest k with index[k] == v
__global__ void __launch_bounds__(256) meas_lut_kernel(const int64_t *__restrict__ index, int K, int64_t imin, int *lut)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) atomicMin(&lut[index[k] - imin], k);
}

// slot of every requested index value (rep[k]); -1 where the value is absent (cannot happen for the LUT path)
__global__ void __launch_bounds__(256) meas_rep_kernel(const int64_t *__restrict__ index, int K, SlotMap m, int *rep)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    if (m.mode == S_LUT) rep[k] = m.lut[index[k] - m.imin];
    else rep[k] = k;
}

__global__ void __launch_bounds__(256) meas_mean_kernel(MeasAcc acc, int nslot, double *mean)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nslot) mean[k] = acc.sum[k] / (double)acc.cnt[k];
}

// per requested index k: out(k, ...) from the accumulators of slot rep[k]
template <typename T>
__global__ void __launch_bounds__(256) meas_finalize_kernel(int op, MeasAcc acc, const int *__restrict__ rep, int K,
                                                            double *outd, T *outv, int64_t *outp)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int s = rep[k];
    switch (op) {
    case 0: outd[k] = acc.sum[s]; break;                                        // sum
    case 1: outd[k] = acc.sum[s] / (double)acc.cnt[s]; break;                   // mean (NaN where absent)
    case 2: outd[k] = acc.ssd[s] / (double)acc.cnt[s]; break;                   // variance
    case 3: outd[k] = sqrt(acc.ssd[s] / (double)acc.cnt[s]); break;             // standard deviation
    case 4: {                                                                   // extrema (+ positions)
        const bool present = acc.kmin[s] <= acc.kmax[s];
        outv[2 * k] = present ? from_key<T>(acc.kmin[s]) : T(0);
        outv[2 * k + 1] = present ? from_key<T>(acc.kmax[s]) : T(0);
        if (outp) {             // -1: no voxel carries the value; 0 where it does when no position pass ran (pmin null)
            const bool last = is_float_t<T>::value && acc.kmax[s] == ~0ull;
            outp[2 * k] = !present ? -1 : acc.pmin ? (int64_t)acc.pmin[s] : 0;
            outp[2 * k + 1] = !present ? -1 : !acc.pmin ? 0 : last ? (int64_t)acc.pmax_last[s] : (int64_t)acc.pmax_first[s];
        }
        break;
    }
    case 5:                                                                     // center of mass
        for (int d = 0; d < acc.ndim; d++) outd[(int64_t)k * acc.ndim + d] = acc.com[(int64_t)s * acc.ndim + d] / acc.sum[s];
        break;
    case 6:                                                                     // histogram
        for (int b = 0; b <= acc.bins; b++) outp[(int64_t)k * (acc.bins + 1) + b] = (int64_t)acc.hist[(int64_t)s * (acc.bins + 1) + b];
        break;
    }
}

static int meas_grid(int64_t n)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)device_cus() * 16));
}

static const char *const kOpName[] = {"M_SUMS", "M_SSD", "M_EXT", "M_POS", "M_COM", "M_HIST"};
static const char *const kSlotName[] = {"all", "positive", "lut", "search", "nonzero"};

// appends "<kernel and route>" to `what` (the name mi_debug_last_kernel reports for the call)
template <typename T, typename L, int OP>
static void launch_meas(const mi_array *in, const mi_array *lab, int64_t n, const SlotMap &m, const MeasAcc &acc, hipStream_t s,
                        std::string &what)
{
    // lsum holds kLdsSlots values; center_of_mass also needs slots x axes <= kLdsCom for lcom
    const int use_lds = ((OP == M_SUMS || OP == M_SSD || OP == M_EXT) && m.nslot <= kLdsSlots) ||
                        (OP == M_COM && m.nslot <= kLdsSlots && m.nslot * std::max(in->ndim, 1) <= kLdsCom);
    hipLaunchKernelGGL((meas_kernel<T, L, OP>), dim3(meas_grid(n)), dim3(256), 0, s, (const T *)in->data,
                       lab ? (const L *)lab->data : nullptr, n, m, acc, use_lds);
    char buf[160];
    snprintf(buf, sizeof buf, "%smi::meas_kernel<%s> grid=%d (%d slots, %s, %s atomics)", what.empty() ? "" : " + ", kOpName[OP],
             meas_grid(n), m.nslot, kSlotName[m.mode], use_lds ? "LDS" : "global");
    what += buf;
}

template <typename T, typename L>
static int run_ops(int op, const mi_array *in, const mi_array *lab, int64_t n, const SlotMap &m, MeasAcc &acc, double *mean_ws,
                   hipStream_t s)
{
    std::string what;
    switch (op) {
    case 0: case 1:
        launch_meas<T, L, M_SUMS>(in, lab, n, m, acc, s, what);
        break;
    case 2: case 3:
        launch_meas<T, L, M_SUMS>(in, lab, n, m, acc, s, what);
        hipLaunchKernelGGL(meas_mean_kernel, dim3((m.nslot + 255) / 256), dim3(256), 0, s, acc, m.nslot, mean_ws);
        acc.mean = mean_ws;
        launch_meas<T, L, M_SSD>(in, lab, n, m, acc, s, what);             // two passes, as SciPy's _stats(centered=True)
        break;
    case 4:
        launch_meas<T, L, M_EXT>(in, lab, n, m, acc, s, what);
        if (acc.pmin) launch_meas<T, L, M_POS>(in, lab, n, m, acc, s, what);
        break;
    case 5:
        launch_meas<T, L, M_COM>(in, lab, n, m, acc, s, what);
        break;
    case 6:
        launch_meas<T, L, M_HIST>(in, lab, n, m, acc, s, what);
        break;
    }
    MI_HIP(hipGetLastError());
    note_kernel("%s", what.c_str());
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_labeled_reduce(int op, const mi_array *in, const mi_array *labels, const mi_array *index, int64_t imin, int64_t imax,
                      int sorted_index, const double *edges, int bins, const mi_array *out, const mi_array *out_pos,
                      mi_stream stream)
{
    int rc;
    if ((rc = check_array(in, "input")) || (rc = check_array(out, "output"))) return rc;
    const int flags = op & ~0xff;
    op &= 0xff;
    MI_REQUIRE(op >= 0 && op <= 6 && (flags & ~(MI_REDUCE_NONZERO | MI_REDUCE_PRESENCE)) == 0, MI_ERR_INVALID_ARG,
               "unknown labelled reduction");
    MI_REQUIRE(!(flags & MI_REDUCE_PRESENCE) || (op == 4 && out_pos), MI_ERR_INVALID_ARG,
               "MI_REDUCE_PRESENCE: extrema with out_pos");
    MI_REQUIRE(is_contiguous(in) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "mi_labeled_reduce needs C-contiguous arrays");
    MI_REQUIRE(in->dtype != MI_F16, MI_ERR_INVALID_ARG, "float16 input: convert to float32 first");
    if (labels) {
        if ((rc = check_array(labels, "labels"))) return rc;
        MI_REQUIRE(same_shape(in, labels) && is_contiguous(labels), MI_ERR_INVALID_ARG, "labels must be C-contiguous of the input's shape");
        MI_REQUIRE(labels->dtype == MI_I32 || labels->dtype == MI_I64, MI_ERR_INVALID_ARG, "labels must be int32 or int64");
    }
    int K = 1;
    if (index) {
        if ((rc = check_array(index, "index"))) return rc;
        MI_REQUIRE(labels && index->dtype == MI_I64 && index->ndim == 1 && is_contiguous(index), MI_ERR_INVALID_ARG,
                   "index must be a 1-D int64 array (and needs labels)");
        MI_REQUIRE(index->shape[0] >= 1 && index->shape[0] < (1 << 30), MI_ERR_INVALID_ARG, "index: 1 .. 2**30 values");
        K = (int)index->shape[0];
        MI_REQUIRE(imin <= imax && (sorted_index || (uint64_t)imax - (uint64_t)imin < ((uint64_t)1 << 30)), MI_ERR_INVALID_ARG,
                   "index range: a lookup table covers at most 2**30 values (pass the index sorted and unique)");
    }
    MI_REQUIRE(op != 6 || (edges && bins >= 1), MI_ERR_INVALID_ARG, "histogram needs bins and edges");
    const int outer = op == 4 ? 2 : op == 5 ? in->ndim : op == 6 ? bins + 1 : 1;
    MI_REQUIRE(numel(out) == (int64_t)K * outer, MI_ERR_INVALID_ARG, "output size");
    const int want = op == 4 ? in->dtype : op == 6 ? MI_I64 : MI_F64;
    MI_REQUIRE(out->dtype == want, MI_ERR_INVALID_ARG, "output dtype: the input's for extrema, int64 for histograms, float64 otherwise");
    MI_REQUIRE(op != 6 || (int64_t)K * (bins + 1) < ((int64_t)1 << 31), MI_ERR_INVALID_ARG, "histogram: too many index values x bins");
    if (out_pos) {
        MI_REQUIRE(op == 4 && out_pos->dtype == MI_I64 && numel(out_pos) == (int64_t)K * 2 && is_contiguous(out_pos), MI_ERR_INVALID_ARG,
                   "positions: int64 (K, 2)");
    }
    const int64_t n = numel(in);
    hipStream_t s = resolve_stream(stream);

    SlotMap m{};
    m.nslot = K;
    m.imin = imin;
    m.imax = imax;
    m.mode = !labels ? S_ALL : !index ? ((flags & MI_REDUCE_NONZERO) ? S_NONZERO : S_POSITIVE) : sorted_index ? S_SEARCH : S_LUT;
    const int64_t lutn = m.mode == S_LUT ? imax - imin + 1 : 0;
    const int nd = in->ndim;
    // workspace: lut | rep | cnt | sum | ssd | mean | kmin | kmax | pmin | pmaxf | pmaxl | com | hist | edges
    const size_t S = (size_t)K;
    const size_t bytes = (size_t)lutn * 4 + S * 4 + S * 8 * 10 + S * 8 * (size_t)std::max(nd, 1) + (op == 6 ? S * 8 * (bins + 1) + 8 * (bins + 1) : 0) + 64;
    void *ws = nullptr;
    if ((rc = pool_alloc(&ws, bytes, s))) return rc;
    char *w = (char *)ws;
    int *lut = (int *)w; w += lutn * 4;
    int *rep = (int *)w; w += S * 4;
    w = (char *)(((uintptr_t)w + 7) & ~(uintptr_t)7);
    char *acc0 = w;
    MeasAcc acc{};
    acc.cnt = (unsigned long long *)w; w += S * 8;
    acc.sum = (double *)w; w += S * 8;
    acc.ssd = (double *)w; w += S * 8;
    double *mean_ws = (double *)w; w += S * 8;
    char *zero_end = w;
    acc.kmin = (unsigned long long *)w; w += S * 8;
    acc.pmin = (unsigned long long *)w; w += S * 8;
    acc.pmax_first = (unsigned long long *)w; w += S * 8;
    char *ones_end = w;
    acc.kmax = (unsigned long long *)w; w += S * 8;
    acc.pmax_last = (long long *)w; w += S * 8;
    char *acc_end2 = w;
    acc.com = (double *)w; w += S * 8 * std::max(nd, 1);
    acc.hist = (unsigned long long *)w; if (op == 6) w += S * 8 * (bins + 1);
    double *dedges = (double *)w;
    char *zero2_end = w;
    acc.ndim = nd;
    for (int d = 0; d < nd; d++) acc.shape[d] = in->shape[d];
    acc.bins = bins;
    acc.edges = dedges;
    if (!out_pos || (flags & MI_REDUCE_PRESENCE)) { acc.pmin = nullptr; }      // no M_POS pass

    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(acc0, 0, zero_end - acc0, s);
    if (e == hipSuccess) e = hipMemsetAsync(zero_end, 0xff, ones_end - zero_end, s);                 // kmin, pmin, pmax_first
    if (e == hipSuccess) e = hipMemsetAsync(acc.kmax, 0, S * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(acc.pmax_last, 0xff, S * 8, s);                          // -1
    if (e == hipSuccess) e = hipMemsetAsync(acc_end2, 0, zero2_end - acc_end2, s);
    if (e == hipSuccess && op == 6) e = hipMemcpyAsync(dedges, edges, 8 * (size_t)(bins + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && m.mode == S_LUT) e = hipMemsetAsync(lut, 0x7f, (size_t)lutn * 4, s);
    if (e != hipSuccess) { pool_free(ws); set_error("HIP error: %s", hipGetErrorString(e)); return MI_ERR_INTERNAL; }
    const int64_t *idx = index ? (const int64_t *)index->data : nullptr;
    if (m.mode == S_LUT) {
        hipLaunchKernelGGL(meas_lut_kernel, dim3((K + 255) / 256), dim3(256), 0, s, idx, K, imin, lut);
        m.lut = lut;
    }
    if (m.mode == S_SEARCH) m.sorted = idx;
    if (m.mode == S_LUT) hipLaunchKernelGGL(meas_rep_kernel, dim3((K + 255) / 256), dim3(256), 0, s, idx, K, m, rep);
    else e = hipMemsetAsync(rep, 0, S * 4, s);          // S_ALL / S_POSITIVE / S_NONZERO: one slot; S_SEARCH: identity, set below
    if (m.mode == S_SEARCH) hipLaunchKernelGGL(meas_rep_kernel, dim3((K + 255) / 256), dim3(256), 0, s, idx, K, m, rep);

    if (n > 0) {
        rc = dispatch_dtype(in->dtype, [&]<typename T>() -> int {
            if (labels && labels->dtype == MI_I64) return run_ops<T, int64_t>(op, in, labels, n, m, acc, mean_ws, s);
            return run_ops<T, int32_t>(op, in, labels, n, m, acc, mean_ws, s);
        });
    } else if (op == 2 || op == 3) {
        hipLaunchKernelGGL(meas_mean_kernel, dim3((K + 255) / 256), dim3(256), 0, s, acc, K, mean_ws);
    }
    if (rc == MI_OK) {
        rc = dispatch_dtype(op == 4 ? in->dtype : MI_F64, [&]<typename T>() -> int {
            hipLaunchKernelGGL((meas_finalize_kernel<T>), dim3((K + 255) / 256), dim3(256), 0, s, op, acc, (const int *)rep, K,
                               (double *)out->data, (T *)out->data, op == 6 ? (int64_t *)out->data : out_pos ? (int64_t *)out_pos->data : nullptr);
            MI_HIP(hipGetLastError());
            return MI_OK;
        });
    }
    pool_free(ws);
    if (e != hipSuccess) { set_error("HIP error: %s", hipGetErrorString(e)); return MI_ERR_INTERNAL; }
    return rc;
}

}  // extern "C"
