// segment.hip -- skimage.segmentation boundaries and relabelling (cupyimg/skimage/segmentation/boundaries.py, _join.py),
// skimage.util.map_array (cupyimg/skimage/util/_map_array.py) and the pieces of `unique` of the array layer that select.hip
// does not have.  Every comparison is of integers and every atomic an integer minimum: the results do not depend on the order
// in which workgroups run.
//
//   mi_find_boundaries            modes thick / inner / outer.  With N1(p) the neighbours of p at city-block distance <=
//                                 connectivity, N(p) the 3^ndim window, both clamped to the array, MAX the largest value of the
//                                 dtype and g(v) = (v == background ? MAX : v):
//                                   thick(p) = some q in N1(p) has L[q] != L[p]
//                                   inner(p) = thick(p) and L[p] != background
//                                   outer(p) = thick(p) and (L[p] == background or max_N L[q] != min_N g(L[q]))
//                                 Ranks 2 and 3: bd_tile_kernel, a core box and its one-sample halo in LDS (skimage_common.hpp),
//                                 one launch; every other rank, a refusal of the planner, or after mi_debug_set_boundaries(.., 1):
//                                 bd_generic_kernel, one thread per voxel.
//   mi_find_boundaries_subpixel   the (2 s - 1)-shaped output of mode="subpixel", one thread per output element.
//   mi_paint_boundaries           the two masked assignments of mark_boundaries in one launch.
//   mi_map_array_table / _search  out[i] = output_vals[j] for the lowest j with input_vals[j] == input[i], 0 without one: through a
//                                 dense table of j over the key range (filled by atomicMin, kept in LDS when asked), or by a
//                                 leftmost binary search in the stably sorted keys.
//   mi_unique_heads / _counts / _inverse   head flags of a sorted array, the run lengths and the inverse permutation.
//   mi_join_key                   key = mul * r1 + r2 in int64.
#include <algorithm>
#include <limits>

#include "skimage_common.hpp"

namespace mi {

static Knob g_bd_small{0};
static Knob g_bd_generic{0};
static std::atomic<int> g_seg_launches{0};

constexpr int kSegNT = 256;
// the largest staged box of plan_halo1_box is (4 + 2) x (8 + 2) x (64 + 2) samples of 8 bytes = 31 680 bytes
constexpr int kBdLdsBytes = 32 * 1024;
constexpr int kMapLdsBytes = 64 * 1024;          // dynamic LDS a launch gets without an attribute
constexpr int32_t kNoKey = 0x7fffffff;

#define SEG_LAUNCH(kernel, grid, lds, stream, ...)                                                          \
    do {                                                                                                    \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(kSegNT), lds, stream, __VA_ARGS__);         \
        g_seg_launches.fetch_add(1, std::memory_order_relaxed);                                             \
    } while (0)

template <typename T> struct bd_storage { typedef T type; };
template <> struct bd_storage<bool> { typedef uint8_t type; };

// ------------------------------------------------------------------ boundaries
template <typename T>
struct BdRule {
    T bg, maxv;
    int has_bg;             // 0: the background is no value of the dtype, so no voxel is background
    int conn, mode;         // mode 0 thick, 1 inner, 2 outer
};

template <typename T>
__device__ __forceinline__ uint8_t bd_result(const BdRule<T> &r, T v0, bool thick, T mx, T mn)
{
    const bool is_bg = r.has_bg && v0 == r.bg;
    if (r.mode == 0) return thick;
    if (r.mode == 1) return thick && !is_bg;
    return thick && (is_bg || mx != mn);
}

template <typename T, int RANK, bool OUTER>
__global__ void __launch_bounds__(kSegNT) bd_tile_kernel(const T *__restrict__ in, BoxDims b, int64_t nboxes, BdRule<T> r, uint8_t *__restrict__ out)
{
    // dynamic, sized to the staged box: the staging is a chain of load round trips, so the workgroups a CU holds hide it
    extern __shared__ __align__(16) unsigned char bd_lds[];
    T *tile = (T *)bd_lds;
    constexpr int HZ = RANK == 3 ? 1 : 0;
    const int ey = b.t[1] + 2, ex = b.t[2] + 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t box = blockIdx.x; box < nboxes; box += gridDim.x) {
        int z0, y0, x0;
        box_origin(b, box, z0, y0, x0);
        stage_halo1_box<T, RANK, kSegNT>(tile, in, b, MI_MODE_REFLECT, z0, y0, x0);
        __syncthreads();
        // as in the staging, a wave takes rows and its lanes run along x: one division a row, none a voxel
        for (int row = wave; row < b.t[0] * b.t[1]; row += kSegNT / 64) {
            const int z = row / b.t[1], y = row - z * b.t[1];
            if (z0 + z >= b.n[0] || y0 + y >= b.n[1]) continue;
            const T *crow = tile + ((z + HZ) * ey + y + 1) * ex + 1;
            uint8_t *orow = out + ((int64_t)(z0 + z) * b.n[1] + y0 + y) * b.n[2] + x0;
            for (int x = lane; x < b.t[2] && x0 + x < b.n[2]; x += 64) {
                const T *c = crow + x;
                const T v0 = *c;
                bool thick = false;
                T mx = v0, mn = (r.has_bg && v0 == r.bg) ? r.maxv : v0;
#pragma unroll
                for (int dz = -HZ; dz <= HZ; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++) {
                            const int cb = (dz != 0) + (dy != 0) + (dx != 0);
                            if (cb == 0) continue;
                            if (!OUTER && cb > r.conn) continue;
                            const T v = c[(dz * ey + dy) * ex + dx];
                            if (cb <= r.conn) thick |= v != v0;
                            if (OUTER) {
                                mx = v > mx ? v : mx;
                                const T gv = (r.has_bg && v == r.bg) ? r.maxv : v;
                                mn = gv < mn ? gv : mn;
                            }
                        }
                orow[x] = bd_result<T>(r, v0, thick, mx, mn);
            }
        }
        __syncthreads();
    }
}

// one thread per voxel, any rank: the 3^ndim window walked by an odometer, every index clamped to the array
template <typename T>
__global__ void __launch_bounds__(kSegNT) bd_generic_kernel(const T *__restrict__ in, VoxelGeom<MI_MAX_NDIM> g, BdRule<T> r, uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kSegNT) {
        int64_t c[MI_MAX_NDIM];
        int o[MI_MAX_NDIM];
        voxel_coords<MI_MAX_NDIM, true>(g, i, c);
        for (int d = 0; d < MI_MAX_NDIM; d++) o[d] = -1;
        const T v0 = in[i];
        bool thick = false;
        T mx = v0, mn = (r.has_bg && v0 == r.bg) ? r.maxv : v0;
        for (;;) {
            int64_t idx = 0;
            int cb = 0;
            for (int d = 0; d < g.nd; d++) {
                int64_t q = c[d] + o[d];
                q = q < 0 ? 0 : (q >= g.shape[d] ? g.shape[d] - 1 : q);
                idx += q * g.stride[d];
                cb += o[d] != 0;
            }
            if (cb != 0 && (r.mode == 2 || cb <= r.conn)) {
                const T v = in[idx];
                if (cb <= r.conn) thick |= v != v0;
                mx = v > mx ? v : mx;
                const T gv = (r.has_bg && v == r.bg) ? r.maxv : v;
                mn = gv < mn ? gv : mn;
            }
            int d = g.nd - 1;
            while (d >= 0 && ++o[d] > 1) {
                o[d] = -1;
                d--;
            }
            if (d < 0) break;
        }
        out[i] = bd_result<T>(r, v0, thick, mx, mn);
    }
}

__device__ __forceinline__ uint64_t load_bits(const void *p, int64_t i, int esize)
{
    switch (esize) {
    case 1:  return ((const uint8_t *)p)[i];
    case 2:  return ((const uint16_t *)p)[i];
    case 4:  return ((const uint32_t *)p)[i];
    default: return ((const uint64_t *)p)[i];
    }
}

__device__ __forceinline__ void store_bits(void *p, int64_t i, int esize, uint64_t v)
{
    switch (esize) {
    case 1:  ((uint8_t *)p)[i] = (uint8_t)v; break;
    case 2:  ((uint16_t *)p)[i] = (uint16_t)v; break;
    case 4:  ((uint32_t *)p)[i] = (uint32_t)v; break;
    default: ((uint64_t *)p)[i] = v; break;
    }
}

// mode="subpixel": go is the output's geometry (2 s - 1 per axis), gi the label image's.  An element with every coordinate
// even is a pixel: false.  Any other one is true when {MAX} + {0 if a coordinate is first or last} + {the labels of the pixels its
// 3^ndim window covers} has more than two distinct values; only equality is asked of the labels, so they are compared as bits.
__global__ void __launch_bounds__(kSegNT) bd_subpixel_kernel(const void *__restrict__ in, int esize, VoxelGeom<MI_MAX_NDIM> go,
                                                            VoxelGeom<MI_MAX_NDIM> gi, uint64_t maxbits, uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < go.total; i += (int64_t)gridDim.x * kSegNT) {
        int64_t c[MI_MAX_NDIM];
        voxel_coords<MI_MAX_NDIM, true>(go, i, c);
        unsigned odd = 0;
        bool border = false;
        int64_t base = 0;
        for (int d = 0; d < go.nd; d++) {
            if (c[d] & 1) odd |= 1u << d;
            if (c[d] == 0 || c[d] == go.shape[d] - 1) border = true;
            base += (c[d] >> 1) * gi.stride[d];
        }
        if (!odd) {
            out[i] = 0;
            continue;
        }
        uint64_t second = 0;
        int nseen = 1;                   // MAX
        bool many = false;
        auto add = [&](uint64_t v) {
            if (v == maxbits) return;
            if (nseen == 1) {
                second = v;
                nseen = 2;
            } else if (v != second) {
                many = true;
            }
        };
        if (border) add(0);
        for (unsigned m = 0; m < (1u << go.nd) && !many; m++) {
            if (m & ~odd) continue;                          // the second pixel exists along odd coordinates only
            int64_t idx = base;
            for (int d = 0; d < go.nd; d++)
                if ((m >> d) & 1u) idx += gi.stride[d];      // (c + 1) / 2 <= s - 1: c is odd, so c <= 2 s - 3
            add(load_bits(in, idx, esize));
        }
        out[i] = many;
    }
}

// marked[boundaries] = color after marked[dilation(boundaries, square(3))] = outline_color, as one pass: the colour where
// the boundary is set, the outline colour where it is not but one of the 3 x 3 neighbours (clamped to the image) is
template <typename F>
struct PaintColors {
    F color[3], outline[3];
    int has_outline;
};

template <typename F>
__global__ void __launch_bounds__(kSegNT) paint_kernel(const uint8_t *__restrict__ bd, int64_t M, int64_t N, F *__restrict__ img, PaintColors<F> pc)
{
    for (int64_t p = (int64_t)blockIdx.x * kSegNT + threadIdx.x; p < M * N; p += (int64_t)gridDim.x * kSegNT) {
        if (bd[p]) {
            for (int k = 0; k < 3; k++) img[3 * p + k] = pc.color[k];
        } else if (pc.has_outline) {
            const int64_t y = p / N, x = p - y * N;
            bool any = false;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    int64_t yy = y + dy, xx = x + dx;
                    yy = yy < 0 ? 0 : (yy >= M ? M - 1 : yy);
                    xx = xx < 0 ? 0 : (xx >= N ? N - 1 : xx);
                    any |= bd[yy * N + xx] != 0;
                }
            if (any)
                for (int k = 0; k < 3; k++) img[3 * p + k] = pc.outline[k];
        }
    }
}

// ------------------------------------------------------------------ map_array
// an integer of any dtype as an unsigned key that orders like its value
__device__ __forceinline__ uint64_t ordered_key(const void *p, int64_t i, int dt)
{
    constexpr uint64_t sign = (uint64_t)1 << 63;
    switch (dt) {
    case MI_I8:   return (uint64_t)(int64_t)((const int8_t *)p)[i] ^ sign;
    case MI_U8:   return (uint64_t)((const uint8_t *)p)[i];
    case MI_I16:  return (uint64_t)(int64_t)((const int16_t *)p)[i] ^ sign;
    case MI_U16:  return (uint64_t)((const uint16_t *)p)[i];
    case MI_I32:  return (uint64_t)(int64_t)((const int32_t *)p)[i] ^ sign;
    case MI_U32:  return (uint64_t)((const uint32_t *)p)[i];
    case MI_I64:  return (uint64_t)((const int64_t *)p)[i] ^ sign;
    default:      return ((const uint64_t *)p)[i];
    }
}

__global__ void __launch_bounds__(kSegNT) map_table_fill_kernel(int32_t *__restrict__ table, int64_t range)
{
    for (int64_t k = (int64_t)blockIdx.x * kSegNT + threadIdx.x; k < range; k += (int64_t)gridDim.x * kSegNT) table[k] = kNoKey;
}

// table[key - kmin] = the lowest j that has the key: integer minima, whatever order they arrive in
__global__ void __launch_bounds__(kSegNT) map_table_set_kernel(const void *__restrict__ keys, int dt, int64_t nvals, uint64_t kmin, int64_t range,
                                                              int32_t *__restrict__ table)
{
    for (int64_t j = (int64_t)blockIdx.x * kSegNT + threadIdx.x; j < nvals; j += (int64_t)gridDim.x * kSegNT) {
        const uint64_t k = ordered_key(keys, j, dt) - kmin;
        if (k < (uint64_t)range) atomicMin(&table[k], (int32_t)j);
    }
}

template <bool LDS>
__global__ void __launch_bounds__(kSegNT) map_gather_kernel(const void *__restrict__ in, int dt, int64_t n, uint64_t kmin, int64_t range,
                                                           const int32_t *__restrict__ table, int64_t nvals, const void *__restrict__ vals,
                                                           int esize, void *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char map_lds[];
    const int32_t *tab = table;
    if (LDS) {
        int32_t *t = (int32_t *)map_lds;
        for (int64_t k = threadIdx.x; k < range; k += kSegNT) t[k] = table[k];
        __syncthreads();
        tab = t;
    }
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSegNT) {
        const uint64_t k = ordered_key(in, i, dt) - kmin;
        const int64_t j = k < (uint64_t)range ? (int64_t)tab[k] : (int64_t)kNoKey;
        store_bits(out, i, esize, j >= 0 && j < nvals ? load_bits(vals, j, esize) : 0ull);
    }
}

// sorted: the keys in ascending order, perm[k] the position of sorted[k] among the caller's keys; the sort is stable, so the
// leftmost equal key is the one of the lowest position
__global__ void __launch_bounds__(kSegNT) map_search_kernel(const void *__restrict__ in, int dt, int64_t n, const void *__restrict__ sorted,
                                                           const int64_t *__restrict__ perm, int64_t nvals, const void *__restrict__ vals, int esize,
                                                           void *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSegNT) {
        const uint64_t key = ordered_key(in, i, dt);
        int64_t lo = 0, hi = nvals;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (ordered_key(sorted, mid, dt) < key) lo = mid + 1;
            else hi = mid;
        }
        uint64_t v = 0;
        if (lo < nvals && ordered_key(sorted, lo, dt) == key) {
            const int64_t j = perm[lo];
            if (j >= 0 && j < nvals) v = load_bits(vals, j, esize);
        }
        store_bits(out, i, esize, v);
    }
}

// ------------------------------------------------------------------ unique
__global__ void __launch_bounds__(kSegNT) unique_heads_kernel(const void *__restrict__ sorted, int esize, int64_t n, uint8_t *__restrict__ heads)
{
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSegNT)
        heads[i] = i == 0 || load_bits(sorted, i, esize) != load_bits(sorted, i - 1, esize);
}

__global__ void __launch_bounds__(kSegNT) unique_counts_kernel(const int64_t *__restrict__ pos, int64_t K, int64_t n, int64_t *__restrict__ counts)
{
    for (int64_t k = (int64_t)blockIdx.x * kSegNT + threadIdx.x; k < K; k += (int64_t)gridDim.x * kSegNT)
        counts[k] = (k + 1 < K ? pos[k + 1] : n) - pos[k];
}

// inverse[perm[i]] = the number of heads at or before sorted position i, less one: the rank of the last head <= i in pos
__global__ void __launch_bounds__(kSegNT) unique_inverse_kernel(const int64_t *__restrict__ pos, int64_t K, const int64_t *__restrict__ perm, int64_t n,
                                                               int64_t *__restrict__ inverse)
{
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSegNT) {
        int64_t lo = 0, hi = K;                  // first k with pos[k] > i
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (pos[mid] <= i) lo = mid + 1;
            else hi = mid;
        }
        const int64_t j = perm[i];
        if (j >= 0 && j < n) inverse[j] = lo - 1;
    }
}

// ------------------------------------------------------------------ join key
__device__ __forceinline__ int64_t load_i64(const void *p, int64_t i, int dt)
{
    switch (dt) {
    case MI_BOOL: return (int64_t)(((const uint8_t *)p)[i] != 0);
    case MI_I8:   return (int64_t)((const int8_t *)p)[i];
    case MI_U8:   return (int64_t)((const uint8_t *)p)[i];
    case MI_I16:  return (int64_t)((const int16_t *)p)[i];
    case MI_U16:  return (int64_t)((const uint16_t *)p)[i];
    case MI_I32:  return (int64_t)((const int32_t *)p)[i];
    case MI_U32:  return (int64_t)((const uint32_t *)p)[i];
    case MI_I64:  return ((const int64_t *)p)[i];
    default:      return (int64_t)((const uint64_t *)p)[i];
    }
}

__global__ void __launch_bounds__(kSegNT) join_key_kernel(const void *__restrict__ r1, int dt1, const void *__restrict__ r2, int dt2, int64_t n, int64_t mul,
                                                         int64_t *__restrict__ key)
{
    for (int64_t i = (int64_t)blockIdx.x * kSegNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSegNT)
        key[i] = mul * load_i64(r1, i, dt1) + load_i64(r2, i, dt2);
}

// ------------------------------------------------------------------ host side
static bool is_integer_dtype(int dt) { return dt >= MI_I8 && dt <= MI_U64; }

static bool overlaps(const mi_array *a, const mi_array *b)
{
    const char *pa = (const char *)a->data, *pb = (const char *)b->data;
    const int64_t na = numel(a) * (int64_t)dtype_size(a->dtype), nb = numel(b) * (int64_t)dtype_size(b->dtype);
    return pa < pb + nb && pb < pa + na;
}

template <typename T, int RANK>
static int bd_tile(const mi_array *labels, const BdRule<T> &r, uint8_t *out, hipStream_t s)
{
    BoxDims b;
    int64_t nboxes;
    const int rc = plan_halo1_box(labels, g_bd_small != 0, kBdLdsBytes, &b, &nboxes);
    if (rc) return rc == MI_ERR_INTERNAL ? MI_ERR_UNSUPPORTED : rc;
    const int grid = box_grid(nboxes);
    // the staged box, which the planner held to kBdLdsBytes, rounded up to 16 bytes
    const size_t lds = ((size_t)(b.t[0] + (RANK == 3 ? 2 : 0)) * (b.t[1] + 2) * (b.t[2] + 2) * sizeof(T) + 15) & ~(size_t)15;
    if (r.mode == 2) SEG_LAUNCH((bd_tile_kernel<T, RANK, true>), grid, lds, s, (const T *)labels->data, b, nboxes, r, out);
    else SEG_LAUNCH((bd_tile_kernel<T, RANK, false>), grid, lds, s, (const T *)labels->data, b, nboxes, r, out);
    MI_HIP(hipGetLastError());
    note_kernel("mi::bd_tile_kernel<%d bytes,%d> grid=%d box=%dx%dx%d lds=%zu mode=%d connectivity=%d (one launch)", (int)sizeof(T), RANK, grid, b.t[0],
                b.t[1], b.t[2], lds, r.mode, r.conn);
    return MI_OK;
}

template <typename T>
static int bd_generic(const mi_array *labels, const BdRule<T> &r, uint8_t *out, hipStream_t s)
{
    VoxelGeom<MI_MAX_NDIM> g;
    voxel_geom(labels, &g);
    const int grid = capped_grid(g.total, kSegNT, 1 << 16);
    SEG_LAUNCH((bd_generic_kernel<T>), grid, 0, s, (const T *)labels->data, g, r, out);
    MI_HIP(hipGetLastError());
    note_kernel("mi::bd_generic_kernel<%d bytes> grid=%d rank %d mode=%d connectivity=%d (one launch)", (int)sizeof(T), grid, g.nd, r.mode, r.conn);
    return MI_OK;
}

static int map_check(const mi_array *input, const mi_array *keys, const mi_array *vals, const mi_array *out)
{
    int rc;
    if ((rc = check_array(input, "input")) || (rc = check_array(keys, "keys")) || (rc = check_array(vals, "output_vals")) || (rc = check_array(out, "out")))
        return rc;
    MI_REQUIRE(is_integer_dtype(input->dtype) && keys->dtype == input->dtype, MI_ERR_INVALID_ARG, "map_array: an integer input and keys of its dtype");
    MI_REQUIRE(vals->dtype == out->dtype && vals->dtype != MI_F16, MI_ERR_INVALID_ARG, "map_array: the output has the dtype of the output values (not float16)");
    MI_REQUIRE(keys->ndim == 1 && vals->ndim == 1 && keys->shape[0] == vals->shape[0] && keys->shape[0] >= 1 && keys->shape[0] < kNoKey,
               MI_ERR_INVALID_ARG, "map_array: 1 to 2^31 - 2 keys, one output value each");
    MI_REQUIRE(is_contiguous(input) && is_contiguous(keys) && is_contiguous(vals) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS,
               "map_array needs C-contiguous arrays");
    MI_REQUIRE(numel(out) == numel(input), MI_ERR_INVALID_ARG, "map_array: the output has as many elements as the input");
    if (numel(input) == 0) return 1;
    MI_REQUIRE(input->data && keys->data && vals->data && out->data, MI_ERR_INVALID_ARG, "null data pointer");
    MI_REQUIRE(!overlaps(input, out) && !overlaps(vals, out) && !overlaps(keys, out), MI_ERR_INVALID_ARG, "map_array: the output may not share memory with an input");
    return 0;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_boundaries(int small_tiles, int force_generic)
{
    g_bd_small = small_tiles != 0;
    g_bd_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_debug_segment_launches(void) { return g_seg_launches.load(std::memory_order_relaxed); }

extern "C" int mi_find_boundaries(const mi_array *labels, int connectivity, int mode, int has_background, int64_t background, const mi_array *out,
                                  mi_stream stream)
{
    int rc;
    if ((rc = check_array(labels, "labels")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(labels->dtype == MI_BOOL || is_integer_dtype(labels->dtype), MI_ERR_INVALID_ARG, "find_boundaries: an integer or bool label image");
    MI_REQUIRE(labels->ndim >= 1, MI_ERR_INVALID_ARG, "find_boundaries: arrays of rank 1 to 8");
    MI_REQUIRE(connectivity >= 1 && connectivity <= labels->ndim, MI_ERR_INVALID_ARG, "find_boundaries: connectivity 1 .. ndim");
    MI_REQUIRE(mode >= 0 && mode <= 2, MI_ERR_INVALID_ARG, "find_boundaries: mode 0 (thick), 1 (inner) or 2 (outer)");
    MI_REQUIRE(is_contiguous(labels), MI_ERR_NOT_CONTIGUOUS, "find_boundaries needs a C-contiguous label image");
    MI_REQUIRE(out->dtype == MI_BOOL && same_shape(out, labels) && is_contiguous(out), MI_ERR_INVALID_ARG,
               "find_boundaries: a C-contiguous bool output of the image's shape");
    if (numel(labels) == 0) return MI_OK;
    MI_REQUIRE(labels->data && out->data, MI_ERR_INVALID_ARG, "null data pointer");
    MI_REQUIRE(!overlaps(labels, out), MI_ERR_INVALID_ARG, "find_boundaries: the output may not share memory with the image");
    hipStream_t s = resolve_stream(stream);
    return dispatch_dtype(labels->dtype, [&]<typename T0>() -> int {
        if constexpr (std::is_floating_point<T0>::value) {
            return MI_ERR_INVALID_ARG;
        } else {
            typedef typename bd_storage<T0>::type T;
            BdRule<T> r;
            r.bg = (T)background;
            r.maxv = std::numeric_limits<T>::max();
            r.has_bg = has_background != 0;
            r.conn = connectivity;
            r.mode = mode;
            uint8_t *o = (uint8_t *)out->data;
            if (!g_bd_generic && (labels->ndim == 2 || labels->ndim == 3)) {
                const int rc2 = labels->ndim == 3 ? bd_tile<T, 3>(labels, r, o, s) : bd_tile<T, 2>(labels, r, o, s);
                if (rc2 != MI_ERR_UNSUPPORTED) return rc2;
            }
            return bd_generic<T>(labels, r, o, s);
        }
    });
}

extern "C" int mi_find_boundaries_subpixel(const mi_array *labels, const mi_array *out, mi_stream stream)
{
    int rc;
    if ((rc = check_array(labels, "labels")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(labels->dtype == MI_BOOL || is_integer_dtype(labels->dtype), MI_ERR_INVALID_ARG, "find_boundaries: an integer or bool label image");
    MI_REQUIRE(labels->ndim >= 1 && out->ndim == labels->ndim, MI_ERR_INVALID_ARG, "find_boundaries: arrays of rank 1 to 8");
    MI_REQUIRE(is_contiguous(labels), MI_ERR_NOT_CONTIGUOUS, "find_boundaries needs a C-contiguous label image");
    MI_REQUIRE(out->dtype == MI_BOOL && is_contiguous(out), MI_ERR_INVALID_ARG, "find_boundaries: a C-contiguous bool output");
    for (int d = 0; d < labels->ndim; d++)
        MI_REQUIRE(labels->shape[d] >= 1 && out->shape[d] == 2 * labels->shape[d] - 1, MI_ERR_INVALID_ARG,
                   "output shape: 2 s - 1 along every axis of s >= 1 samples");
    MI_REQUIRE(labels->data && out->data, MI_ERR_INVALID_ARG, "null data pointer");
    MI_REQUIRE(!overlaps(labels, out), MI_ERR_INVALID_ARG, "find_boundaries: the output may not share memory with the image");
    VoxelGeom<MI_MAX_NDIM> go, gi;
    voxel_geom(out, &go);
    voxel_geom(labels, &gi);
    const int esize = (int)dtype_size(labels->dtype);
    uint64_t maxbits;
    switch (labels->dtype) {
    case MI_BOOL: case MI_U8: maxbits = 0xffull; break;          // bool images are uint8 images here
    case MI_I8:   maxbits = 0x7full; break;
    case MI_I16:  maxbits = 0x7fffull; break;
    case MI_U16:  maxbits = 0xffffull; break;
    case MI_I32:  maxbits = 0x7fffffffull; break;
    case MI_U32:  maxbits = 0xffffffffull; break;
    case MI_I64:  maxbits = 0x7fffffffffffffffull; break;
    default:      maxbits = ~0ull; break;
    }
    hipStream_t s = resolve_stream(stream);
    const int grid = capped_grid(go.total, kSegNT, 1 << 16);
    SEG_LAUNCH(bd_subpixel_kernel, grid, 0, s, (const void *)labels->data, esize, go, gi, maxbits, (uint8_t *)out->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::bd_subpixel_kernel<%d bytes> grid=%d rank %d (one launch)", esize, grid, go.nd);
    return MI_OK;
}

extern "C" int mi_paint_boundaries(const mi_array *boundaries, const mi_array *image, const double *color, const double *outline_color, mi_stream stream)
{
    int rc;
    if ((rc = check_array(boundaries, "boundaries")) || (rc = check_array(image, "image"))) return rc;
    MI_REQUIRE(color, MI_ERR_INVALID_ARG, "paint_boundaries: no colour");
    MI_REQUIRE(boundaries->dtype == MI_BOOL && boundaries->ndim == 2 && is_contiguous(boundaries), MI_ERR_INVALID_ARG,
               "paint_boundaries: a C-contiguous (M, N) bool array of boundaries");
    MI_REQUIRE((image->dtype == MI_F32 || image->dtype == MI_F64) && image->ndim == 3 && image->shape[2] == 3 && image->shape[0] == boundaries->shape[0] &&
               image->shape[1] == boundaries->shape[1] && is_contiguous(image), MI_ERR_INVALID_ARG,
               "paint_boundaries: a C-contiguous (M, N, 3) float32 or float64 image");
    const int64_t M = boundaries->shape[0], N = boundaries->shape[1];
    if (M * N == 0) return MI_OK;
    MI_REQUIRE(boundaries->data && image->data, MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    const int grid = capped_grid(M * N, kSegNT, 1 << 16);
    if (image->dtype == MI_F32) {
        PaintColors<float> pc;
        for (int k = 0; k < 3; k++) {
            pc.color[k] = (float)color[k];
            pc.outline[k] = outline_color ? (float)outline_color[k] : 0.0f;
        }
        pc.has_outline = outline_color != nullptr;
        SEG_LAUNCH((paint_kernel<float>), grid, 0, s, (const uint8_t *)boundaries->data, M, N, (float *)image->data, pc);
    } else {
        PaintColors<double> pc;
        for (int k = 0; k < 3; k++) {
            pc.color[k] = color[k];
            pc.outline[k] = outline_color ? outline_color[k] : 0.0;
        }
        pc.has_outline = outline_color != nullptr;
        SEG_LAUNCH((paint_kernel<double>), grid, 0, s, (const uint8_t *)boundaries->data, M, N, (double *)image->data, pc);
    }
    MI_HIP(hipGetLastError());
    note_kernel("mi::paint_kernel<%s> grid=%d outline=%d (one launch)", image->dtype == MI_F32 ? "float32" : "float64", grid, outline_color != nullptr);
    return MI_OK;
}

extern "C" int mi_map_array_table(const mi_array *input, const mi_array *keys, const mi_array *output_vals, const mi_array *out, uint64_t key_min,
                                  int64_t range, int use_lds, mi_stream stream)
{
    const int st = map_check(input, keys, output_vals, out);
    if (st < 0) return st;
    MI_REQUIRE(range >= 1 && range <= ((int64_t)1 << 31), MI_ERR_INVALID_ARG, "map_array: a key range of 1 to 2^31 values for the table route");
    MI_REQUIRE(!use_lds || range * 4 <= kMapLdsBytes, MI_ERR_INVALID_ARG, "map_array: the table does not fit the LDS of a workgroup");
    if (st == 1) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int64_t n = numel(input), nvals = keys->shape[0];
    void *mem = nullptr;
    int rc = pool_alloc(&mem, (size_t)range * sizeof(int32_t), s);
    if (rc) return rc;
    int32_t *table = (int32_t *)mem;
    const int dt = (int)input->dtype, esize = (int)dtype_size(out->dtype);
    SEG_LAUNCH(map_table_fill_kernel, capped_grid(range, kSegNT, 1 << 14), 0, s, table, range);
    SEG_LAUNCH(map_table_set_kernel, capped_grid(nvals, kSegNT, 1 << 14), 0, s, (const void *)keys->data, dt, nvals, key_min, range, table);
    int grid;
    if (use_lds) {
        // every workgroup reads the whole table once: give each at least 16 voxels a thread to spread that over
        grid = capped_grid(n, kSegNT * 16, 2048);
        SEG_LAUNCH((map_gather_kernel<true>), grid, (size_t)range * sizeof(int32_t), s, (const void *)input->data, dt, n, key_min, range, (const int32_t *)table,
                   nvals, (const void *)output_vals->data, esize, out->data);
    } else {
        grid = capped_grid(n, kSegNT, 1 << 16);
        SEG_LAUNCH((map_gather_kernel<false>), grid, 0, s, (const void *)input->data, dt, n, key_min, range, (const int32_t *)table, nvals,
                   (const void *)output_vals->data, esize, out->data);
    }
    const hipError_t e = hipGetLastError();
    pool_free(mem);
    MI_HIP(e);
    note_kernel("mi::map_gather_kernel<%s> grid=%d keys=%lld range=%lld (table fill, atomicMin set, gather: three launches)", use_lds ? "lds" : "global", grid,
                (long long)nvals, (long long)range);
    return MI_OK;
}

extern "C" int mi_map_array_search(const mi_array *input, const mi_array *sorted_keys, const mi_array *perm, const mi_array *output_vals,
                                   const mi_array *out, mi_stream stream)
{
    const int st = map_check(input, sorted_keys, output_vals, out);
    if (st < 0) return st;
    int rc;
    if ((rc = check_array(perm, "perm"))) return rc;
    MI_REQUIRE(perm->dtype == MI_I64 && perm->ndim == 1 && perm->shape[0] == sorted_keys->shape[0] && is_contiguous(perm) && perm->data, MI_ERR_INVALID_ARG,
               "map_array: the permutation is a C-contiguous int64 array, one entry per key");
    if (st == 1) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int64_t n = numel(input), nvals = sorted_keys->shape[0];
    const int grid = capped_grid(n, kSegNT, 1 << 16);
    SEG_LAUNCH(map_search_kernel, grid, 0, s, (const void *)input->data, (int)input->dtype, n, (const void *)sorted_keys->data, (const int64_t *)perm->data,
               nvals, (const void *)output_vals->data, (int)dtype_size(out->dtype), out->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::map_search_kernel grid=%d keys=%lld (leftmost binary search, one launch)", grid, (long long)nvals);
    return MI_OK;
}

extern "C" int mi_unique_heads(const mi_array *sorted, const mi_array *heads, mi_stream stream)
{
    int rc;
    if ((rc = check_array(sorted, "sorted")) || (rc = check_array(heads, "heads"))) return rc;
    MI_REQUIRE(sorted->ndim == 1 && is_contiguous(sorted) && sorted->dtype != MI_F16, MI_ERR_INVALID_ARG, "unique_heads: a C-contiguous 1-D array");
    MI_REQUIRE(heads->dtype == MI_BOOL && heads->ndim == 1 && heads->shape[0] == sorted->shape[0] && is_contiguous(heads), MI_ERR_INVALID_ARG,
               "unique_heads: a bool output of the array's length");
    const int64_t n = sorted->shape[0];
    if (n == 0) return MI_OK;
    MI_REQUIRE(sorted->data && heads->data, MI_ERR_INVALID_ARG, "null data pointer");
    hipStream_t s = resolve_stream(stream);
    const int grid = capped_grid(n, kSegNT, 1 << 16);
    SEG_LAUNCH(unique_heads_kernel, grid, 0, s, (const void *)sorted->data, (int)dtype_size(sorted->dtype), n, (uint8_t *)heads->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::unique_heads_kernel grid=%d (one launch)", grid);
    return MI_OK;
}

static int unique_pos_check(const mi_array *pos, const mi_array *o, int64_t n_out, const char *name)
{
    int rc;
    if ((rc = check_array(pos, "pos")) || (rc = check_array(o, name))) return rc;
    MI_REQUIRE(pos->dtype == MI_I64 && pos->ndim == 1 && is_contiguous(pos) && o->dtype == MI_I64 && o->ndim == 1 && is_contiguous(o) && o->shape[0] == n_out,
               MI_ERR_INVALID_ARG, "unique: C-contiguous 1-D int64 arrays of the expected lengths");
    return MI_OK;
}

extern "C" int mi_unique_counts(const mi_array *pos, int64_t n, const mi_array *counts, mi_stream stream)
{
    int rc;
    if ((rc = unique_pos_check(pos, counts, pos ? pos->shape[0] : 0, "counts"))) return rc;
    const int64_t K = pos->shape[0];
    if (K == 0) return MI_OK;
    MI_REQUIRE(pos->data && counts->data && n >= K, MI_ERR_INVALID_ARG, "unique_counts: at least as many elements as heads");
    hipStream_t s = resolve_stream(stream);
    const int grid = capped_grid(K, kSegNT, 1 << 16);
    SEG_LAUNCH(unique_counts_kernel, grid, 0, s, (const int64_t *)pos->data, K, n, (int64_t *)counts->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::unique_counts_kernel grid=%d (one launch)", grid);
    return MI_OK;
}

extern "C" int mi_unique_inverse(const mi_array *pos, const mi_array *perm, const mi_array *inverse, mi_stream stream)
{
    int rc;
    if ((rc = check_array(perm, "perm"))) return rc;
    MI_REQUIRE(perm->dtype == MI_I64 && perm->ndim == 1 && is_contiguous(perm), MI_ERR_INVALID_ARG, "unique_inverse: a C-contiguous int64 permutation");
    if ((rc = unique_pos_check(pos, inverse, perm->shape[0], "inverse"))) return rc;
    const int64_t n = perm->shape[0], K = pos->shape[0];
    if (n == 0) return MI_OK;
    MI_REQUIRE(pos->data && perm->data && inverse->data && K >= 1, MI_ERR_INVALID_ARG, "unique_inverse: null data pointer or no heads");
    hipStream_t s = resolve_stream(stream);
    const int grid = capped_grid(n, kSegNT, 1 << 16);
    SEG_LAUNCH(unique_inverse_kernel, grid, 0, s, (const int64_t *)pos->data, K, (const int64_t *)perm->data, n, (int64_t *)inverse->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::unique_inverse_kernel grid=%d heads=%lld (one launch)", grid, (long long)K);
    return MI_OK;
}

extern "C" int mi_join_key(const mi_array *r1, const mi_array *r2, int64_t mul, const mi_array *key, mi_stream stream)
{
    int rc;
    if ((rc = check_array(r1, "r1")) || (rc = check_array(r2, "r2")) || (rc = check_array(key, "key"))) return rc;
    MI_REQUIRE(is_integer_dtype(r1->dtype) && is_integer_dtype(r2->dtype) && key->dtype == MI_I64, MI_ERR_INVALID_ARG,
               "join_key: integer fields and an int64 key");
    MI_REQUIRE(same_shape(r1, r2) && same_shape(r1, key), MI_ERR_INVALID_ARG, "join_key: arrays of one shape");
    MI_REQUIRE(is_contiguous(r1) && is_contiguous(r2) && is_contiguous(key), MI_ERR_NOT_CONTIGUOUS, "join_key needs C-contiguous arrays");
    const int64_t n = numel(r1);
    if (n == 0) return MI_OK;
    MI_REQUIRE(r1->data && r2->data && key->data && mul >= 1, MI_ERR_INVALID_ARG, "join_key: null data pointer or a multiplier below 1");
    hipStream_t s = resolve_stream(stream);
    const int grid = capped_grid(n, kSegNT, 1 << 16);
    SEG_LAUNCH(join_key_kernel, grid, 0, s, (const void *)r1->data, (int)r1->dtype, (const void *)r2->data, (int)r2->dtype, n, mul, (int64_t *)key->data);
    MI_HIP(hipGetLastError());
    note_kernel("mi::join_key_kernel grid=%d (one launch)", grid);
    return MI_OK;
}
