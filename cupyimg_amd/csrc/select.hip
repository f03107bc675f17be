// select.hip -- results whose size depends on the data: stream compaction (count_nonzero, flatnonzero, nonzero, argwhere),
// flat gather (take), a stable LSD radix sort of (key, index) pairs (argsort, sort), the peak candidates of
// skimage.feature.peak_local_max (cupyimg/skimage/feature/peak.py:20-71) and the greedy spacing of ensure_spacing /
// corner_peaks (cupyimg/skimage/_shared/coord.py, corner.py:929-945) on the device.
//
// Two rules hold for every kernel of this file:
//   * no workgroup waits on another one inside a kernel: every dependency between workgroups is a launch boundary (per-tile
//     counts | scan | scatter; per-workgroup digit histogram | scan | scatter);
//   * where an element lands never depends on the order in which waves arrive: positions come from __ballot / __popcll
//     within a wave (wave64), the waves of a workgroup taken in order through LDS, and the scanned per-tile table.  The one
//     atomic of the file adds integers into a counter (the number of voxels equal to their filtered maximum), whose value
//     does not depend on the order either.
// Every index a kernel stores to is compared with the size of its destination first, whatever the (pooled, possibly dirty)
// tables say.
//
// Tiles: a workgroup of 256 threads owns kSelChunks (compaction) or >= kSortChunks (sort) consecutive chunks of 256 elements;
// the scan handles 1024 table entries per workgroup and level.  After mi_debug_set_select(1) a tile is 64 elements (one wave)
// and a scan block 64 entries, so that an array of a few thousand elements spans many tiles and several scan levels.
#include "common.hpp"

#include <algorithm>
#include <vector>

namespace mi {

static Knob g_sel_small{0};
static std::atomic<int> g_sel_launches{0};

constexpr int kSelChunks = 8;
constexpr int kSortChunks = 16;
constexpr int64_t kSelMaxN = 2147483647LL;
constexpr int kHdrBytes = 64;         // work block: uint64 total, uint64 n_equal, padding; then the tables

#define SEL_LAUNCH(kernel, grid, block, stream, ...)                                        \
    do {                                                                                    \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3((unsigned)(block)), 0, stream, __VA_ARGS__); \
        g_sel_launches.fetch_add(1, std::memory_order_relaxed);                             \
    } while (0)

struct SelGeom {
    int block, chunks, scan_block;
    int64_t tile, ntiles;
};

static SelGeom sel_geom(int64_t n)
{
    SelGeom g;
    const bool small = g_sel_small && n <= (1 << 20);
    g.block = small ? 64 : 256;
    g.chunks = small ? 1 : kSelChunks;
    g.scan_block = small ? 64 : 1024;
    g.tile = (int64_t)g.block * g.chunks;
    g.ntiles = std::max<int64_t>(1, (n + g.tile - 1) / g.tile);
    return g;
}

// entries of the scratch the scan of n entries needs (the block sums of every level)
static int64_t scan_scratch_entries(int64_t n, int S)
{
    int64_t total = 0;
    for (;;) {
        const int64_t nb = (n + S - 1) / S;
        total += nb;
        if (nb <= 1) return total;
        n = nb;
    }
}

static const char *dtype_name(int dt)
{
    static const char *names[] = {"bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64",
                                  "float16"};
    return dt >= 0 && dt <= MI_F16 ? names[dt] : "?";
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    return (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// ------------------------------------------------------------------ exclusive scan of a uint32 table, in place
// scan_block_kernel: workgroup b scans entries [b S, (b + 1) S) and leaves their sum in sums[b]; the sums are scanned by the
// next level (a launch of its own) and scan_add_kernel adds them back.
__global__ void scan_block_kernel(uint32_t *data, int64_t n, int S, uint32_t *sums, unsigned long long *total)
{
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t lo = (int64_t)blockIdx.x * S;
    const int64_t hi = lo + S < n ? lo + S : n;
    uint32_t carry = 0;
    for (int64_t c = lo; c < hi; c += blockDim.x) {
        const int64_t i = c + threadIdx.x;
        const uint32_t v = i < hi ? data[i] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        uint32_t before = carry, all = 0;
        for (int k = 0; k < nw; k++) {
            if (k < w) before += s_wave[k];
            all += s_wave[k];
        }
        if (i < hi) data[i] = before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = carry;
        if (total) *total = carry;
    }
}

__global__ void scan_add_kernel(uint32_t *data, int64_t n, int S, const uint32_t *sums)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) data[i] += sums[i / S];
}

static void scan_u32(uint32_t *data, int64_t n, int S, uint32_t *scratch, unsigned long long *total, hipStream_t s)
{
    const int64_t nb = (n + S - 1) / S;
    SEL_LAUNCH(scan_block_kernel, nb, std::min(S, 256), s, data, n, S, scratch, nb == 1 ? total : nullptr);
    if (nb > 1) {
        scan_u32(scratch, nb, S, scratch + nb, total, s);
        dim3 grid;
        grid_for(n, 256, &grid);
        SEL_LAUNCH(scan_add_kernel, grid.x, 256, s, data, n, S, (const uint32_t *)scratch);
    }
}

// ------------------------------------------------------------------ predicates
template <typename T>
struct NonzeroPred {
    static constexpr bool kCountsEqual = false;
    const T *a;
    __device__ bool operator()(int64_t i, bool &) const { return a[i] != (T)0; }      // NaN != 0, -0.0 == 0
};

template <typename T>
struct PeakPred {
    static constexpr bool kCountsEqual = true;
    const T *image, *image_max;      // image_max == nullptr: image > threshold alone
    double threshold;
    int ndim, any_border;
    int64_t shape[MI_MAX_NDIM], border[MI_MAX_NDIM];
    __device__ bool operator()(int64_t i, bool &equal) const
    {
        const T v = image[i];
        bool ok;
        if constexpr (std::is_floating_point<T>::value) ok = v > (T)threshold;      // the scalar is weak: compared in the image's dtype
        else ok = (double)v > threshold;
        if (image_max) {
            equal = v == image_max[i];
            ok = ok && equal;
        }
        if (ok && any_border) {
            int64_t r = i;
            for (int d = ndim - 1; d >= 0; d--) {
                const int64_t c = r % shape[d];
                r /= shape[d];
                if (c < border[d] || c >= shape[d] - border[d]) ok = false;
            }
        }
        return ok;
    }
};

// where the k-th selected element (flat index i) goes
struct SelWriter {
    int64_t *idx;          // layout 0: idx[k] = i; 1: idx[k, :] = unravel(i) (K, ndim); 2: idx[:, k] = unravel(i) (ndim, K)
    int layout, ndim, vsize;
    int64_t shape[MI_MAX_NDIM];
    int64_t K;
    const void *src;       // with `vals`: vals[k] = src[i], elements of vsize bytes
    void *vals;
    __device__ void operator()(int64_t k, int64_t i) const
    {
        if (k >= K) return;
        if (layout == 0) idx[k] = i;
        else {
            int64_t r = i;
            for (int d = ndim - 1; d >= 0; d--) {
                const int64_t c = r % shape[d];
                r /= shape[d];
                if (layout == 1) idx[k * ndim + d] = c;
                else idx[(int64_t)d * K + k] = c;
            }
        }
        if (vals) {
            switch (vsize) {
            case 1: ((uint8_t *)vals)[k] = ((const uint8_t *)src)[i]; break;
            case 2: ((uint16_t *)vals)[k] = ((const uint16_t *)src)[i]; break;
            case 4: ((uint32_t *)vals)[k] = ((const uint32_t *)src)[i]; break;
            default: ((uint64_t *)vals)[k] = ((const uint64_t *)src)[i]; break;
            }
        }
    }
};

template <typename P>
__global__ void sel_count_kernel(P pred, int64_t n, int chunks, uint32_t *counts, unsigned long long *hdr)
{
    __shared__ uint32_t s_c[8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * chunks * blockDim.x;
    uint32_t cw = 0, ew = 0;
    for (int k = 0; k < chunks; k++) {
        const int64_t i = base + (int64_t)k * blockDim.x + threadIdx.x;
        bool equal = false;
        const bool p = i < n && pred(i, equal);
        cw += (uint32_t)__popcll(__ballot(p));
        if (P::kCountsEqual) ew += (uint32_t)__popcll(__ballot(equal));
    }
    if (lane == 0) { s_c[w] = cw; s_c[4 + w] = ew; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, e = 0;
        for (int k = 0; k < nw; k++) { c += s_c[k]; e += s_c[4 + k]; }
        counts[blockIdx.x] = c;
        if (P::kCountsEqual && e) atomicAdd(&hdr[1], (unsigned long long)e);
    }
}

template <typename P>
__global__ void sel_write_kernel(P pred, SelWriter out, int64_t n, int chunks, const uint32_t *offsets)
{
    __shared__ uint32_t s_w[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * chunks * blockDim.x;
    int64_t run = offsets[blockIdx.x];
    for (int k = 0; k < chunks; k++) {
        const int64_t i = base + (int64_t)k * blockDim.x + threadIdx.x;
        bool equal = false;
        const bool p = i < n && pred(i, equal);
        const uint64_t m = __ballot(p);
        if (lane == 0) s_w[w] = (uint32_t)__popcll(m);
        __syncthreads();
        int64_t off = run;
        uint32_t all = 0;
        for (int q = 0; q < nw; q++) {
            if (q < w) off += s_w[q];
            all += s_w[q];
        }
        if (p) out(off + lanes_below(m), i);
        run += all;
        __syncthreads();
    }
}

// count launch, scan launches, and the total (and the equal count) read back: the one synchronisation of a compaction
template <typename P>
static int sel_count(const P &pred, int64_t n, const mi_array *work, int64_t *total, int64_t *n_equal, hipStream_t s, const char *what,
                     int dtype)
{
    const SelGeom g = sel_geom(n);
    const int64_t need = kHdrBytes + 4 * (g.ntiles + scan_scratch_entries(g.ntiles, g.scan_block));
    MI_REQUIRE(work && work->data && work->dtype == MI_U8 && work->ndim == 1 && work->shape[0] >= need, MI_ERR_INVALID_ARG,
               "the work block is a uint8 array of at least mi_select_work_bytes bytes");
    unsigned long long *hdr = (unsigned long long *)work->data;
    uint32_t *counts = (uint32_t *)((char *)work->data + kHdrBytes);
    MI_HIP(hipMemsetAsync(hdr, 0, kHdrBytes, s));
    SEL_LAUNCH((sel_count_kernel<P>), g.ntiles, g.block, s, pred, n, g.chunks, counts, hdr);
    scan_u32(counts, g.ntiles, g.scan_block, counts + g.ntiles, hdr, s);
    MI_HIP(hipGetLastError());
    unsigned long long host[2] = {0, 0};
    MI_HIP(hipMemcpyAsync(host, hdr, sizeof(host), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    *total = (int64_t)host[0];
    if (n_equal) *n_equal = (int64_t)host[1];
    note_kernel("mi::sel_count_kernel<%s,%s> tile=%d tiles=%lld scan_block=%d (count launch, scan launches, one 16-byte read)", what,
                dtype_name(dtype), (int)g.tile, (long long)g.ntiles, g.scan_block);
    return MI_OK;
}

template <typename P>
static int sel_write(const P &pred, const SelWriter &out, int64_t n, const mi_array *work, hipStream_t s, const char *what, int dtype)
{
    const SelGeom g = sel_geom(n);
    const int64_t need = kHdrBytes + 4 * (g.ntiles + scan_scratch_entries(g.ntiles, g.scan_block));
    MI_REQUIRE(work && work->data && work->dtype == MI_U8 && work->ndim == 1 && work->shape[0] >= need, MI_ERR_INVALID_ARG,
               "the work block is a uint8 array of at least mi_select_work_bytes bytes");
    const uint32_t *offsets = (const uint32_t *)((const char *)work->data + kHdrBytes);
    SEL_LAUNCH((sel_write_kernel<P>), g.ntiles, g.block, s, pred, out, n, g.chunks, offsets);
    MI_HIP(hipGetLastError());
    note_kernel("mi::sel_write_kernel<%s,%s> tile=%d tiles=%lld layout=%d (scatter launch)", what, dtype_name(dtype), (int)g.tile,
                (long long)g.ntiles, out.layout);
    return MI_OK;
}

// the checks every selection entry point shares: 0 = go on, 1 = nothing to do (empty), < 0 = refusal
static int sel_check_input(const mi_array *a, const char *name)
{
    int rc = check_array(a, name);
    if (rc) return rc;
    MI_REQUIRE(a->dtype != MI_F16, MI_ERR_INVALID_ARG, "float16 arrays are storage only: convert with mi_copy (to float32) around this call");
    MI_REQUIRE(is_contiguous(a), MI_ERR_NOT_CONTIGUOUS, "the array must be C-contiguous");
    const int64_t n = numel(a);
    MI_REQUIRE(n <= kSelMaxN, MI_ERR_UNSUPPORTED, "selection and sorting take at most 2^31 - 1 elements");
    if (n == 0) return 1;
    MI_REQUIRE(a->data, MI_ERR_INVALID_ARG, "null data pointer");
    return 0;
}

template <typename T> struct storage_of { typedef T type; };
template <> struct storage_of<bool> { typedef uint8_t type; };

// ------------------------------------------------------------------ take
__global__ void take_kernel(const char *a, const int64_t *idx, char *out, int64_t nidx, int64_t nrows, int64_t inner, int esize, int *flag)
{
    const int64_t total = nidx * inner;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = t / inner, e = t - k * inner;
        int64_t j = idx[k];
        if (j < 0) j += nrows;
        const bool ok = j >= 0 && j < nrows;
        if (!ok) *flag = 1;                      // no read is issued for an index out of range
        const int64_t src = ok ? j * inner + e : 0;
        switch (esize) {
        case 1: ((uint8_t *)out)[t] = ok ? ((const uint8_t *)a)[src] : (uint8_t)0; break;
        case 2: ((uint16_t *)out)[t] = ok ? ((const uint16_t *)a)[src] : (uint16_t)0; break;
        case 4: ((uint32_t *)out)[t] = ok ? ((const uint32_t *)a)[src] : 0u; break;
        default: ((uint64_t *)out)[t] = ok ? ((const uint64_t *)a)[src] : 0ull; break;
        }
    }
}

// ------------------------------------------------------------------ radix sort
template <typename T> struct key_of { typedef typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type type; };

// Order-preserving unsigned key of `descending ? -v : v` (integers negate with wrap-around and bool negates logically, as
// `-a` / `~a` do in NumPy); -0.0 has the key of +0.0 and every NaN the one maximal key.
template <typename T>
__device__ __forceinline__ typename key_of<T>::type sort_key(T v, bool descending)
{
    typedef typename key_of<T>::type K;
    if constexpr (std::is_same<T, float>::value || std::is_same<T, double>::value) {
        if (v != v) return ~(K)0;
        if (descending) v = -v;
        if (v == (T)0) v = (T)0;
        K bits;
        memcpy(&bits, &v, sizeof(K));
        const K sign = (K)1 << (8 * sizeof(K) - 1);
        return (bits & sign) ? ~bits : (bits | sign);
    } else if constexpr (std::is_signed<T>::value) {
        typedef typename std::make_unsigned<T>::type U;
        U u = (U)v;
        if (descending) u = (U)((U)0 - u);
        return (K)(U)(u ^ (U)((U)1 << (8 * sizeof(U) - 1)));
    } else {
        T u = v;
        if (descending) u = (T)((T)0 - u);
        return (K)u;
    }
}

template <typename T, bool IS_BOOL>
__global__ void sort_init_kernel(const T *a, int64_t n, int descending, typename key_of<T>::type *keys, uint32_t *idx)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (IS_BOOL) keys[i] = (uint32_t)((a[i] != 0) != (descending != 0));
        else keys[i] = sort_key<T>(a[i], descending != 0);
        idx[i] = (uint32_t)i;
    }
}

// table[d * nwg + g]: occurrences of digit d in workgroup g's tile -- digit-major, so that its exclusive scan is where workgroup
// g's first element with digit d goes
template <typename K>
__global__ void sort_hist_kernel(const K *keys, int64_t n, int chunks, int shift, uint32_t *table, int nwg)
{
    __shared__ uint32_t h[256];
    for (int d = threadIdx.x; d < 256; d += blockDim.x) h[d] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * chunks * blockDim.x;
    for (int k = 0; k < chunks; k++) {
        const int64_t i = base + (int64_t)k * blockDim.x + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);       // integer counts: no order to depend on
    }
    __syncthreads();
    for (int d = threadIdx.x; d < 256; d += blockDim.x) table[(int64_t)d * nwg + blockIdx.x] = h[d];
}

template <typename K>
__global__ void sort_scatter_kernel(const K *kin, const uint32_t *iin, K *kout, uint32_t *iout, int64_t n, int chunks, int shift,
                                    const uint32_t *table, int nwg)
{
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_cnt[4][256];
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int d = threadIdx.x; d < 256; d += blockDim.x) {
        s_base[d] = table[(int64_t)d * nwg + blockIdx.x];
        for (int q = 0; q < 4; q++) s_cnt[q][d] = 0;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * chunks * blockDim.x;
    for (int k = 0; k < chunks; k++) {
        const int64_t i = base + (int64_t)k * blockDim.x + threadIdx.x;
        const bool valid = i < n;
        const K key = valid ? kin[i] : (K)0;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        // the lanes of this wave with the same digit: eight ballots, one per bit
        uint64_t m = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bb = __ballot(valid && bit);
            m &= bit ? bb : ~bb;
        }
        const uint32_t rank = lanes_below(m);
        if (valid && rank == 0) s_cnt[w][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (valid) {
            int64_t pos = s_base[d];
            for (int q = 0; q < w; q++) pos += s_cnt[q][d];
            pos += rank;
            if (pos < n) {
                kout[pos] = key;
                iout[pos] = iin[i];
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 256; e += blockDim.x) {
            uint32_t sum = 0;
            for (int q = 0; q < nw; q++) {
                sum += s_cnt[q][e];
                s_cnt[q][e] = 0;
            }
            s_base[e] += sum;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void sort_finish_kernel(const uint32_t *idx, const T *a, int64_t n, int64_t *idx_out, T *sorted_out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[i];
        if (idx_out) idx_out[i] = (int64_t)j;
        if (sorted_out) sorted_out[i] = (int64_t)j < n ? a[j] : a[0];
    }
}

template <typename T, bool IS_BOOL>
static int argsort_impl(const mi_array *a, int64_t *idx_out, void *sorted_out, int descending, hipStream_t s)
{
    typedef typename key_of<T>::type K;
    const int64_t n = numel(a);
    const bool small = g_sel_small && n <= (1 << 20);
    const int block = small ? 64 : 256;
    const int chunks = small ? 1 : (int)std::max<int64_t>(kSortChunks, (n + 256LL * 4096 - 1) / (256LL * 4096));
    const int S = small ? 64 : 1024;
    const int64_t tile = (int64_t)block * chunks;
    const int nwg = (int)((n + tile - 1) / tile);
    const int64_t entries = 256LL * nwg;
    const size_t n_al = (size_t)((n + 3) & ~3LL);
    const size_t bytes = 2 * n_al * sizeof(K) + 2 * n_al * sizeof(uint32_t) + 4 * (size_t)(entries + scan_scratch_entries(entries, S));
    void *block_mem = nullptr;
    int rc = pool_alloc(&block_mem, bytes, s);
    if (rc) return rc;
    K *keys[2] = {(K *)block_mem, (K *)block_mem + n_al};
    uint32_t *idx[2] = {(uint32_t *)(keys[1] + n_al), (uint32_t *)(keys[1] + n_al) + n_al};
    uint32_t *table = idx[1] + n_al;
    dim3 grid;
    grid_for(n, 256, &grid);
    SEL_LAUNCH((sort_init_kernel<T, IS_BOOL>), grid.x, 256, s, (const T *)a->data, n, descending, keys[0], idx[0]);
    const int passes = IS_BOOL ? 1 : (int)sizeof(T);
    int cur = 0;
    for (int p = 0; p < passes; p++, cur ^= 1) {
        SEL_LAUNCH((sort_hist_kernel<K>), nwg, block, s, (const K *)keys[cur], n, chunks, 8 * p, table, nwg);
        scan_u32(table, entries, S, table + entries, nullptr, s);
        SEL_LAUNCH((sort_scatter_kernel<K>), nwg, block, s, (const K *)keys[cur], (const uint32_t *)idx[cur], keys[cur ^ 1], idx[cur ^ 1], n,
                   chunks, 8 * p, (const uint32_t *)table, nwg);
    }
    SEL_LAUNCH((sort_finish_kernel<T>), grid.x, 256, s, (const uint32_t *)idx[cur], (const T *)a->data, n, idx_out, (T *)sorted_out);
    hipError_t e = hipGetLastError();
    pool_free(block_mem);
    MI_HIP(e);
    note_kernel("mi::sort_scatter_kernel<%s,%s> tile=%d workgroups=%d passes=%d scan_block=%d (LSD, 8 bits a pass: histogram, scan, stable scatter)",
                dtype_name(a->dtype), descending ? "descending" : "ascending", (int)tile, nwg, passes, S);
    return MI_OK;
}

// ------------------------------------------------------------------ greedy spacing
// status of a point: 2 live, 1 kept, 0 rejected (so that the survivors are the nonzero entries once nothing is live)
constexpr uint8_t kLive = 2, kKept = 1, kRejected = 0;

struct SpParams {
    int ndim, radius, p, inclusive;      // p: 0 = Chebyshev, 1, 2
    int64_t limit;                       // spacing (p 0, 1) or spacing^2 (p 2)
    int64_t shape[MI_MAX_NDIM];
};

__global__ void sp_init_kernel(const int64_t *coords, int64_t K, SpParams P, int32_t *map, uint8_t *status, int *bad)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t flat = 0;
        bool ok = true;
        for (int d = 0; d < P.ndim; d++) {
            const int64_t c = coords[i * P.ndim + d];
            if (c < 0 || c >= P.shape[d]) ok = false;
            flat = flat * P.shape[d] + c;
        }
        status[i] = ok ? kLive : kRejected;
        if (ok) map[flat] = (int32_t)(i + 1);
        else *bad = 1;
    }
}

// f(j) for every point j != i in the window of point i whose distance to i is in conflict; stops when f returns true
template <typename F>
__device__ __forceinline__ bool sp_any_conflict(const int64_t *coords, int64_t i, const SpParams &P, const int32_t *map, int64_t K, F f)
{
    int64_t c[MI_MAX_NDIM], lo[MI_MAX_NDIM], hi[MI_MAX_NDIM], o[MI_MAX_NDIM];
    for (int d = 0; d < P.ndim; d++) {
        c[d] = coords[i * P.ndim + d];
        lo[d] = -P.radius < -c[d] ? -c[d] : -(int64_t)P.radius;
        hi[d] = P.radius > P.shape[d] - 1 - c[d] ? P.shape[d] - 1 - c[d] : (int64_t)P.radius;
        o[d] = lo[d];
    }
    for (;;) {
        int64_t flat = 0, dist = 0;
        for (int d = 0; d < P.ndim; d++) {
            flat = flat * P.shape[d] + (c[d] + o[d]);
            const int64_t a = o[d] < 0 ? -o[d] : o[d];
            if (P.p == 0) dist = a > dist ? a : dist;
            else if (P.p == 1) dist += a;
            else dist += a * a;
        }
        if (dist != 0 && (P.inclusive ? dist <= P.limit : dist < P.limit)) {
            const int64_t j = (int64_t)map[flat] - 1;
            if (j >= 0 && j < K && j != i && f(j)) return true;
        }
        int d = P.ndim - 1;
        while (d >= 0 && ++o[d] > hi[d]) {
            o[d] = lo[d];
            d--;
        }
        if (d < 0) return false;
    }
}

// a live point is kept when no point of lower rank that is live -- or was when this launch began: kept points of earlier
// rounds have no live point left in conflict with them -- conflicts with it
__global__ void sp_keep_kernel(const int64_t *coords, int64_t K, SpParams P, const int32_t *map, uint8_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K || status[i] != kLive) return;
    const volatile uint8_t *st = status;
    const bool blocked = sp_any_conflict(coords, i, P, map, K, [&](int64_t j) { return j < i && st[j] != kRejected; });
    if (!blocked) status[i] = kKept;
}

// live points in conflict with a kept one are rejected; *live = 1 when a point stays live
__global__ void sp_reject_kernel(const int64_t *coords, int64_t K, SpParams P, const int32_t *map, uint8_t *status, int *live)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K || status[i] != kLive) return;
    const volatile uint8_t *st = status;
    const bool hit = sp_any_conflict(coords, i, P, map, K, [&](int64_t j) { return st[j] == kKept; });
    if (hit) status[i] = kRejected;
    else *live = 1;
}

__global__ void scatter_true_kernel(const int64_t *coords, int64_t K, int ndim, SpParams P, uint8_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t flat = 0;
        bool ok = true;
        for (int d = 0; d < ndim; d++) {
            const int64_t c = coords[i * ndim + d];
            if (c < 0 || c >= P.shape[d]) ok = false;
            flat = flat * P.shape[d] + c;
        }
        if (ok) out[flat] = 1;
    }
}

// coords: (K, ndim) int64, C-contiguous, ndim = rank of `grid`
static int sp_check_coords(const mi_array *coords, const mi_array *grid, int grid_dtype, int64_t *K)
{
    int rc;
    if ((rc = check_array(coords, "coords")) || (rc = check_array(grid, "map"))) return rc;
    MI_REQUIRE(coords->dtype == MI_I64 && coords->ndim == 2 && is_contiguous(coords), MI_ERR_INVALID_ARG,
               "coords is a C-contiguous (K, ndim) int64 array");
    MI_REQUIRE(grid->dtype == grid_dtype && grid->ndim >= 1 && is_contiguous(grid) && coords->shape[1] == grid->ndim, MI_ERR_INVALID_ARG,
               "the map / mask is C-contiguous, of the expected dtype and of rank coords.shape[1]");
    MI_REQUIRE(numel(grid) <= kSelMaxN && coords->shape[0] <= kSelMaxN - 1, MI_ERR_UNSUPPORTED,
               "selection and sorting take at most 2^31 - 1 elements");
    *K = coords->shape[0];
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_select(int small_tiles)
{
    g_sel_small = small_tiles != 0;
    return MI_OK;
}

extern "C" int mi_debug_select_launches(void) { return g_sel_launches.load(std::memory_order_relaxed); }

extern "C" int mi_select_work_bytes(int64_t n, int64_t *bytes)
{
    MI_REQUIRE(bytes && n >= 0, MI_ERR_INVALID_ARG, "mi_select_work_bytes: n >= 0 and a place for the answer");
    MI_REQUIRE(n <= kSelMaxN, MI_ERR_UNSUPPORTED, "selection and sorting take at most 2^31 - 1 elements");
    const SelGeom g = sel_geom(n);
    *bytes = kHdrBytes + 4 * (g.ntiles + scan_scratch_entries(g.ntiles, g.scan_block));
    return MI_OK;
}

extern "C" int mi_select_count(const mi_array *a, const mi_array *work, int64_t *total, mi_stream stream)
{
    MI_REQUIRE(total, MI_ERR_INVALID_ARG, "mi_select_count: no place for the total");
    const int st = sel_check_input(a, "a");
    if (st < 0) return st;
    *total = 0;
    if (st == 1) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    return dispatch_dtype(a->dtype, [&]<typename T>() -> int {
        typedef typename storage_of<T>::type U;
        NonzeroPred<U> pred{(const U *)a->data};
        return sel_count(pred, numel(a), work, total, nullptr, s, "nonzero", a->dtype);
    });
}

extern "C" int mi_select_write(const mi_array *a, const mi_array *work, const mi_array *out, int layout, mi_stream stream)
{
    const int st = sel_check_input(a, "a");
    if (st < 0) return st;
    int rc = check_array(out, "out");
    if (rc) return rc;
    MI_REQUIRE(layout >= 0 && layout <= 2, MI_ERR_INVALID_ARG, "layout: 0 flat indices, 1 (K, ndim) rows, 2 (ndim, K) columns");
    MI_REQUIRE(out->dtype == MI_I64 && is_contiguous(out), MI_ERR_INVALID_ARG, "the output is a C-contiguous int64 array");
    SelWriter w = {};
    w.idx = (int64_t *)out->data;
    w.layout = layout;
    w.ndim = a->ndim;
    for (int d = 0; d < a->ndim; d++) w.shape[d] = a->shape[d];
    if (layout == 0) {
        MI_REQUIRE(out->ndim == 1, MI_ERR_INVALID_ARG, "output shape: (K,) for flat indices");
        w.K = out->shape[0];
    } else {
        MI_REQUIRE(out->ndim == 2 && out->shape[layout == 1 ? 1 : 0] == a->ndim && a->ndim >= 1, MI_ERR_INVALID_ARG,
                   "output shape: (K, ndim) rows or (ndim, K) columns");
        w.K = out->shape[layout == 1 ? 0 : 1];
    }
    if (st == 1 || w.K == 0) return MI_OK;
    MI_REQUIRE(out->data, MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    return dispatch_dtype(a->dtype, [&]<typename T>() -> int {
        typedef typename storage_of<T>::type U;
        NonzeroPred<U> pred{(const U *)a->data};
        return sel_write(pred, w, numel(a), work, s, "nonzero", a->dtype);
    });
}

extern "C" int mi_take(const mi_array *a, const mi_array *indices, const mi_array *out, int64_t inner, int32_t *flag_dev, mi_stream stream)
{
    int rc;
    if ((rc = check_array(a, "a")) || (rc = check_array(indices, "indices")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(a->dtype != MI_F16, MI_ERR_INVALID_ARG, "float16 arrays are storage only: convert with mi_copy (to float32) around this call");
    MI_REQUIRE(is_contiguous(a) && is_contiguous(indices) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "the arrays must be C-contiguous");
    MI_REQUIRE(indices->dtype == MI_I64 && out->dtype == a->dtype && flag_dev && inner >= 1, MI_ERR_INVALID_ARG,
               "mi_take: int64 indices, an output of the array's dtype, a device flag, inner >= 1");
    const int64_t n = numel(a), nidx = numel(indices);
    MI_REQUIRE(n % inner == 0 && numel(out) == nidx * inner, MI_ERR_INVALID_ARG, "output shape: one row of `inner` elements per index");
    MI_REQUIRE(n <= kSelMaxN && nidx * inner <= kSelMaxN, MI_ERR_UNSUPPORTED, "selection and sorting take at most 2^31 - 1 elements");
    if (nidx == 0) return MI_OK;
    MI_REQUIRE(indices->data && out->data && (a->data || n == 0), MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    dim3 grid;
    grid_for(nidx * inner, 256, &grid);
    SEL_LAUNCH(take_kernel, grid.x, 256, s, (const char *)a->data, (const int64_t *)indices->data, (char *)out->data, nidx, n / inner, inner,
               (int)dtype_size(a->dtype), (int *)flag_dev);
    MI_HIP(hipGetLastError());
    note_kernel("mi::take_kernel<%s> grid=%d inner=%lld (gather; indices checked on the device)", dtype_name(a->dtype), (int)grid.x,
                (long long)inner);
    return MI_OK;
}

extern "C" int mi_argsort(const mi_array *a, const mi_array *idx_out, const mi_array *sorted_out, int descending, mi_stream stream)
{
    const int st = sel_check_input(a, "a");
    if (st < 0) return st;
    MI_REQUIRE(a->ndim == 1, MI_ERR_INVALID_ARG, "mi_argsort sorts 1-D arrays");
    MI_REQUIRE(idx_out || sorted_out, MI_ERR_INVALID_ARG, "mi_argsort: no output");
    if (idx_out) {
        int rc = check_array(idx_out, "idx_out");
        if (rc) return rc;
        MI_REQUIRE(idx_out->dtype == MI_I64 && idx_out->ndim == 1 && idx_out->shape[0] == a->shape[0] && is_contiguous(idx_out),
                   MI_ERR_INVALID_ARG, "output shape: the indices are a C-contiguous int64 array of the input's length");
    }
    if (sorted_out) {
        int rc = check_array(sorted_out, "sorted_out");
        if (rc) return rc;
        MI_REQUIRE(sorted_out->dtype == a->dtype && sorted_out->ndim == 1 && sorted_out->shape[0] == a->shape[0] && is_contiguous(sorted_out),
                   MI_ERR_INVALID_ARG, "output shape: the sorted values are a C-contiguous array of the input's dtype and length");
        MI_REQUIRE(sorted_out->data != a->data, MI_ERR_INVALID_ARG, "mi_argsort does not sort in place");
    }
    if (st == 1) return MI_OK;
    MI_REQUIRE((!idx_out || idx_out->data) && (!sorted_out || sorted_out->data), MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    int64_t *io = idx_out ? (int64_t *)idx_out->data : nullptr;
    void *so = sorted_out ? sorted_out->data : nullptr;
    if (a->dtype == MI_BOOL) return argsort_impl<uint8_t, true>(a, io, so, descending, s);
    return dispatch_dtype(a->dtype, [&]<typename T>() -> int {
        if constexpr (std::is_same<T, bool>::value) return MI_ERR_INTERNAL;
        else return argsort_impl<T, false>(a, io, so, descending, s);
    });
}

// the fused predicate of the peak candidates
template <typename T>
static int peak_pred(const mi_array *image, const mi_array *image_max, double threshold, const int64_t *border, PeakPred<T> *p)
{
    p->image = (const T *)image->data;
    p->image_max = image_max ? (const T *)image_max->data : nullptr;
    p->threshold = threshold;
    p->ndim = image->ndim;
    p->any_border = 0;
    for (int d = 0; d < image->ndim; d++) {
        p->shape[d] = image->shape[d];
        p->border[d] = border ? border[d] : 0;
        MI_REQUIRE(p->border[d] >= 0, MI_ERR_INVALID_ARG, "the excluded border cannot be negative");
        if (p->border[d] > 0) p->any_border = 1;
    }
    return MI_OK;
}

static int peak_check(const mi_array *image, const mi_array *image_max)
{
    const int st = sel_check_input(image, "image");
    if (st < 0) return st;
    MI_REQUIRE(image->dtype != MI_BOOL, MI_ERR_INVALID_ARG, "peak candidates of a bool image are not defined");
    if (image_max) {
        int rc = check_array(image_max, "image_max");
        if (rc) return rc;
        MI_REQUIRE(image_max->dtype == image->dtype && same_shape(image, image_max) && is_contiguous(image_max), MI_ERR_INVALID_ARG,
                   "image_max is a C-contiguous array of the image's dtype and shape");
        MI_REQUIRE(st == 1 || image_max->data, MI_ERR_INVALID_ARG, "null data pointer");
    }
    return st;
}

extern "C" int mi_peak_count(const mi_array *image, const mi_array *image_max, double threshold, const int64_t *border, const mi_array *work,
                             int64_t *total, int64_t *n_equal, mi_stream stream)
{
    MI_REQUIRE(total && n_equal, MI_ERR_INVALID_ARG, "mi_peak_count: no place for the counts");
    const int st = peak_check(image, image_max);
    if (st < 0) return st;
    *total = *n_equal = 0;
    if (st == 1) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    return dispatch_dtype(image->dtype, [&]<typename T>() -> int {
        typedef typename storage_of<T>::type U;
        PeakPred<U> pred;
        int rc = peak_pred<U>(image, image_max, threshold, border, &pred);
        if (rc) return rc;
        return sel_count(pred, numel(image), work, total, n_equal, s, image_max ? "peak" : "above", image->dtype);
    });
}

extern "C" int mi_peak_write(const mi_array *image, const mi_array *image_max, double threshold, const int64_t *border, const mi_array *work,
                             const mi_array *coords_out, const mi_array *values_out, mi_stream stream)
{
    const int st = peak_check(image, image_max);
    if (st < 0) return st;
    int rc;
    if ((rc = check_array(coords_out, "coords_out")) || (rc = check_array(values_out, "values_out"))) return rc;
    MI_REQUIRE(coords_out->dtype == MI_I64 && coords_out->ndim == 2 && coords_out->shape[1] == image->ndim && image->ndim >= 1 &&
               is_contiguous(coords_out), MI_ERR_INVALID_ARG, "output shape: the coordinates are a C-contiguous (K, ndim) int64 array");
    MI_REQUIRE(values_out->dtype == image->dtype && values_out->ndim == 1 && values_out->shape[0] == coords_out->shape[0] &&
               is_contiguous(values_out), MI_ERR_INVALID_ARG, "output shape: the values are a C-contiguous (K,) array of the image's dtype");
    if (st == 1 || coords_out->shape[0] == 0) return MI_OK;
    MI_REQUIRE(coords_out->data && values_out->data, MI_ERR_INVALID_ARG, "null data pointer");
    SelWriter w = {};
    w.idx = (int64_t *)coords_out->data;
    w.layout = 1;
    w.ndim = image->ndim;
    for (int d = 0; d < image->ndim; d++) w.shape[d] = image->shape[d];
    w.K = coords_out->shape[0];
    w.src = image->data;
    w.vals = values_out->data;
    w.vsize = (int)dtype_size(image->dtype);
    hipStream_t s = resolve_stream(stream);
    return dispatch_dtype(image->dtype, [&]<typename T>() -> int {
        typedef typename storage_of<T>::type U;
        PeakPred<U> pred;
        int rc2 = peak_pred<U>(image, image_max, threshold, border, &pred);
        if (rc2) return rc2;
        return sel_write(pred, w, numel(image), work, s, image_max ? "peak" : "above", image->dtype);
    });
}

static int sp_params(const mi_array *map, int64_t spacing, int p_norm, int inclusive, SpParams *P)
{
    MI_REQUIRE(p_norm >= 0 && p_norm <= 2, MI_ERR_INVALID_ARG, "p_norm: 0 (Chebyshev), 1 or 2");
    MI_REQUIRE(spacing >= 0 && spacing <= 46340, MI_ERR_INVALID_ARG, "spacing: 0 .. 46340");
    P->ndim = map->ndim;
    P->inclusive = inclusive != 0;
    P->p = p_norm;
    P->radius = (int)(inclusive ? spacing : spacing - 1);
    if (P->radius < 0) P->radius = 0;
    P->limit = p_norm == 2 ? spacing * spacing : spacing;
    for (int d = 0; d < map->ndim; d++) P->shape[d] = map->shape[d];
    return MI_OK;
}

extern "C" int mi_spacing_init(const mi_array *coords, const mi_array *map, const mi_array *status, int *bad, mi_stream stream)
{
    int64_t K = 0;
    int rc = sp_check_coords(coords, map, MI_I32, &K);
    if (rc) return rc;
    if ((rc = check_array(status, "status"))) return rc;
    MI_REQUIRE(status->dtype == MI_U8 && status->ndim == 1 && status->shape[0] == K && is_contiguous(status) && bad, MI_ERR_INVALID_ARG,
               "status is a (K,) uint8 array");
    *bad = 0;
    if (K == 0 || numel(map) == 0) {
        *bad = K != 0;
        return MI_OK;
    }
    MI_REQUIRE(coords->data && map->data && status->data, MI_ERR_INVALID_ARG, "null data pointer");
    SpParams P = {};
    if ((rc = sp_params(map, 0, 0, 0, &P))) return rc;
    hipStream_t s = resolve_stream(stream);
    void *flag = nullptr;
    if ((rc = pool_alloc(&flag, sizeof(int), s))) return rc;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e == hipSuccess) e = hipMemsetAsync(map->data, 0, (size_t)numel(map) * sizeof(int32_t), s);      // pooled memory arrives dirty
    dim3 grid;
    grid_for(K, 256, &grid);
    if (e == hipSuccess) {
        SEL_LAUNCH(sp_init_kernel, grid.x, 256, s, (const int64_t *)coords->data, K, P, (int32_t *)map->data, (uint8_t *)status->data, (int *)flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    pool_free(flag);
    MI_HIP(e);
    note_kernel("mi::sp_init_kernel grid=%d points=%lld (the map zeroed, rank + 1 scattered, one 4-byte read)", (int)grid.x, (long long)K);
    return MI_OK;
}

extern "C" int mi_spacing_rounds(const mi_array *coords, const mi_array *map, const mi_array *status, int64_t spacing, int p_norm,
                                 int inclusive, int nrounds, int *live, mi_stream stream)
{
    int64_t K = 0;
    int rc = sp_check_coords(coords, map, MI_I32, &K);
    if (rc) return rc;
    if ((rc = check_array(status, "status"))) return rc;
    MI_REQUIRE(status->dtype == MI_U8 && status->ndim == 1 && status->shape[0] == K && is_contiguous(status) && live && nrounds >= 1,
               MI_ERR_INVALID_ARG, "status is a (K,) uint8 array; at least one round");
    *live = 0;
    if (K == 0) return MI_OK;
    MI_REQUIRE(coords->data && map->data && status->data, MI_ERR_INVALID_ARG, "null data pointer");
    SpParams P = {};
    if ((rc = sp_params(map, spacing, p_norm, inclusive, &P))) return rc;
    hipStream_t s = resolve_stream(stream);
    void *flag = nullptr;
    if ((rc = pool_alloc(&flag, sizeof(int), s))) return rc;
    const int64_t grid = (K + 255) / 256;
    hipError_t e = hipSuccess;
    for (int r = 0; r < nrounds && e == hipSuccess; r++) {
        SEL_LAUNCH(sp_keep_kernel, grid, 256, s, (const int64_t *)coords->data, K, P, (const int32_t *)map->data, (uint8_t *)status->data);
        if (r == nrounds - 1) e = hipMemsetAsync(flag, 0, sizeof(int), s);
        if (e != hipSuccess) break;
        SEL_LAUNCH(sp_reject_kernel, grid, 256, s, (const int64_t *)coords->data, K, P, (const int32_t *)map->data, (uint8_t *)status->data,
                   (int *)flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(live, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    pool_free(flag);
    MI_HIP(e);
    note_kernel("mi::sp_keep_kernel + mi::sp_reject_kernel grid=%lld points=%lld radius=%d p=%d %s rounds=%d (two launches a round, one 4-byte read)",
                (long long)grid, (long long)K, P.radius, p_norm, inclusive ? "inclusive" : "strict", nrounds);
    return MI_OK;
}

extern "C" int mi_scatter_true(const mi_array *coords, const mi_array *out, mi_stream stream)
{
    int64_t K = 0;
    int rc = sp_check_coords(coords, out, MI_BOOL, &K);
    if (rc) return rc;
    const int64_t n = numel(out);
    if (n == 0) return MI_OK;
    MI_REQUIRE(out->data && (K == 0 || coords->data), MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    MI_HIP(hipMemsetAsync(out->data, 0, (size_t)n, s));
    if (K == 0) return MI_OK;
    SpParams P = {};
    for (int d = 0; d < out->ndim; d++) P.shape[d] = out->shape[d];
    dim3 grid;
    grid_for(K, 256, &grid);
    SEL_LAUNCH(scatter_true_kernel, grid.x, 256, s, (const int64_t *)coords->data, K, out->ndim, P, (uint8_t *)out->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::scatter_true_kernel grid=%d points=%lld", (int)grid.x, (long long)K);
    return MI_OK;
}
