// morphsnakes.hip -- morphological snakes (skimage.segmentation.morphological_chan_vese / morphological_geodesic_active_contour):
// one iteration of the evolution as ONE main launch, no host round trip inside the loop.
//
// Reference path replaced: cupyimg/skimage/segmentation/morphsnakes.py:55-92 (sup_inf / inf_sup), :347-378 (MorphACWE) and
// :468-510 (MorphGAC), which run one iteration with smoothing = 1 as about 60 launches and over 100 volume passes plus, for
// MorphACWE, two host synchronisations.
//
// An iteration is a chain of STAGES, each a radius-1 stencil on the binary field u (int8, 0 / 1), voxels outside the array
// counting as 0 for the morphological stages:
//
//     DILATE / ERODE  (MorphGAC balloon)  u' = OR / AND of u over the full 3^ndim neighbourhood, taken only where
//                                         double(image) > mask_threshold, else u
//     ACWE            du_a = numpy.gradient(u) along axis a: (u[+1] - u[-1]) / 2 inside, u[1] - u[0] and u[n-1] - u[n-2] at
//                     the two ends;  where some du_a != 0:  b = lambda1 (I - c1)^2 - lambda2 (I - c0)^2 in the image dtype T,
//                     b < 0: u' = 1, b > 0: u' = 0;  everywhere else u' = u
//     GAC             aux = ((0 + gI_0 du_0) + gI_1 du_1) + gI_2 du_2 in T, gI_a = numpy.gradient(I) by the same rule with
//                     `/ 2`;  aux > 0: u' = 1, aux < 0: u' = 0, else u.  (Where every du_a is 0, aux is 0 or NaN: u' = u
//                     without a read of the image.)
//     SI  (sup_inf)   u' = OR over the 9 planes (3-D: _P3) / 4 lines (2-D: _P2) P through the voxel of (AND of u over P)
//     IS  (inf_sup)   u' = AND over the same P of (OR of u over P)
//
// This file is compiled with -ffp-contract=off: every product and sum rounds on its own.
//
// snake_fused_kernel: a workgroup owns a core box of tz x ty x tx voxels (ty x tx pixels), stages u on the box plus a halo of
// one voxel per stage as BYTES in LDS, runs the stages one after the other between two LDS buffers on extents that shrink by
// one voxel per stage, and writes its core.  The halo is recomputed by the neighbours (overlapped boxes); nothing crosses
// workgroups inside a launch.  Positions outside the array hold 0 in every buffer, which is the border value of every
// morphological stage; the one-sided differences at the ends of an axis are decided from the voxel's coordinates, so a tile
// border is never mistaken for the array's.  With `sums` the launch also leaves, per workgroup, the four double partial
// sums of MorphACWE over its core and the NEW u.
// snake_generic_kernel: ONE stage, one thread per voxel, straight from global memory: the in-tree comparator.
// snake_sums_kernel / snake_finish_kernel: the partial sums on their own, and the one workgroup that adds the partials in a
// fixed order and writes c0 and c1 (rounded to T) into the state block.
// snake_hist_kernel / snake_pick_kernel: radix select (8 bits a pass) of two neighbouring order statistics for
// threshold = "auto".
#include "skimage_common.hpp"

namespace mi {

constexpr int kSnNT = 256;
constexpr int kSnMaxStages = 8;              // stages of one launch at most (LDS: two byte buffers of the box plus halo)
constexpr int kSnGenericMaxGrid = 2048;

enum { SN_IS = 0, SN_SI = 1, SN_ACWE = 2, SN_GAC = 3, SN_DILATE = 4, SN_ERODE = 5 };

// the first MI_SNAKE_STATE_BYTES of the caller's work block (include/mi355img.h)
struct SnakeState {
    double c0, c1;              // MorphACWE: the means outside / inside, rounded to the image dtype
    double sums[4];             // sum I (1 - u), sum I u, sum (1 - u), sum u  of the last finish (a diagnostic)
    double stat[2];             // mi_snake_order_stats: the two order statistics
};
static_assert(sizeof(SnakeState) == MI_SNAKE_STATE_BYTES, "state block layout");

struct SnakeSelect {            // radix-select state, in the partials region of the work block
    unsigned long long hist[2][256];
    unsigned long long prefix[2];
    unsigned long long rank[2];
};

struct SnakeProg {
    int nz, ny, nx;             // an image is one plane (nz = 1)
    int tz, ty, tx;             // core box
    int ntz, nty, ntx;
    int nst;
    int kind[kSnMaxStages];
    int sums;
};

template <typename T>
struct SnakeArgs {
    const T *img;
    T lam1, lam2;
    double mask_thr;
    const SnakeState *state;
};

// ------------------------------------------------------------------ the stencils
// bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of a neighbourhood word; images use the nine bits of dz = 0
constexpr uint32_t sn_plane(int k)
{
    uint32_t m = 0;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const bool in = k == 0 ? dx == 0 : k == 1 ? dy == 0 : k == 2 ? dz == 0 : k == 3 ? dy == dx : k == 4 ? dy == -dx
                              : k == 5 ? dz == dx : k == 6 ? dz == -dx : k == 7 ? dz == dy : dz == -dy;
                if (in) m |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
            }
    return m;
}
constexpr uint32_t kSnMid = 0x1FFu << 9;     // the plane dz = 0

template <int ND, typename Acc>
__device__ __forceinline__ uint32_t sn_gather(Acc at)
{
    uint32_t m = 0;
#pragma unroll
    for (int dz = (ND == 3 ? -1 : 0); dz <= (ND == 3 ? 1 : 0); dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) m |= (uint32_t)at(dz, dy, dx) << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
    return m;
}

template <int ND>
__device__ __forceinline__ int sn_morph(int kind, uint32_t m)
{
    constexpr uint32_t full = ND == 3 ? (1u << 27) - 1 : kSnMid;
    if (kind == SN_DILATE) return m != 0;
    if (kind == SN_ERODE) return m == full;
    int si = 0, is = 1;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        if (ND == 2 && (k == 2 || k >= 5)) continue;          // _P2: the lines dx = 0, dy = 0, dy = dx, dy = -dx
        const uint32_t p = ND == 3 ? sn_plane(k) : (sn_plane(k) & kSnMid);
        si |= (m & p) == p;
        is &= (m & p) != 0;
    }
    return kind == SN_SI ? si : is;
}

// One stage at voxel (z, y, x) = linear index gi of an array of nz x ny x nx, c = u there, at(dz, dy, dx) = u of a neighbour
// INSIDE the array (never called for one outside by the update stages; 0 outside for the morphological ones).
template <typename T, int ND, typename Acc>
__device__ __forceinline__ int sn_eval(int kind, Acc at, int c, int z, int y, int x, int64_t gi, const SnakeProg &g, const SnakeArgs<T> &a,
                                       T c0, T c1)
{
    if (kind == SN_ACWE || kind == SN_GAC) {
        // numpy.gradient(u): lo / hi = the two voxels of the difference, end = a one-sided difference (no halving)
        int lo[3], hi[3];
        bool end[3];
        if (ND == 3) {
            lo[0] = z > 0 ? at(-1, 0, 0) : c; hi[0] = z < g.nz - 1 ? at(1, 0, 0) : c; end[0] = z == 0 || z == g.nz - 1;
        } else {
            lo[0] = hi[0] = 0; end[0] = true;
        }
        lo[1] = y > 0 ? at(0, -1, 0) : c; hi[1] = y < g.ny - 1 ? at(0, 1, 0) : c; end[1] = y == 0 || y == g.ny - 1;
        lo[2] = x > 0 ? at(0, 0, -1) : c; hi[2] = x < g.nx - 1 ? at(0, 0, 1) : c; end[2] = x == 0 || x == g.nx - 1;
        if (lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2]) return c;
        if (kind == SN_ACWE) {
            const T v = a.img[gi];
            const T d1 = v - c1, d0 = v - c0;
            const T b = a.lam1 * (d1 * d1) - a.lam2 * (d0 * d0);
            return b < T(0) ? 1 : (b > T(0) ? 0 : c);
        }
        const int64_t st[3] = {(int64_t)g.ny * g.nx, (int64_t)g.nx, 1};
        const int pos[3] = {z, y, x}, len[3] = {g.nz, g.ny, g.nx};
        const T v = a.img[gi];
        T aux = T(0);
#pragma unroll
        for (int ax = (ND == 3 ? 0 : 1); ax < 3; ax++) {
            const T du = end[ax] ? T(hi[ax] - lo[ax]) : T(hi[ax] - lo[ax]) / T(2);
            T gr;
            if (pos[ax] == 0) gr = a.img[gi + st[ax]] - v;
            else if (pos[ax] == len[ax] - 1) gr = v - a.img[gi - st[ax]];
            else gr = (a.img[gi + st[ax]] - a.img[gi - st[ax]]) / T(2);
            aux = aux + gr * du;
        }
        return aux > T(0) ? 1 : (aux < T(0) ? 0 : c);
    }
    if (kind == SN_DILATE || kind == SN_ERODE) {
        if (!((double)a.img[gi] > a.mask_thr)) return c;
    }
    return sn_morph<ND>(kind, sn_gather<ND>(at));
}

// four partial sums of a workgroup, reduced in a fixed order (a tree over the thread index): no floating-point atomics
__device__ __forceinline__ void sn_block_partials(const double (&v)[4], double *__restrict__ part)
{
    __shared__ double red[4][kSnNT];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; k++) red[k][tid] = v[k];
    __syncthreads();
    for (int sft = kSnNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) {
#pragma unroll
            for (int k = 0; k < 4; k++) red[k][tid] += red[k][tid + sft];
        }
        __syncthreads();
    }
    if (tid < 4) part[4 * (int64_t)blockIdx.x + tid] = red[tid][0];
}

template <typename T>
__device__ __forceinline__ void sn_accumulate(double (&s)[4], T v, int u)
{
    // image * (1 - u), image * u, (1 - u), u: the products are exact, the sums are in double
    s[0] += u ? 0.0 : (double)v;
    s[1] += u ? (double)v : 0.0;
    s[2] += u ? 0.0 : 1.0;
    s[3] += u ? 1.0 : 0.0;
}

template <typename T, int ND>
__global__ void __launch_bounds__(kSnNT)
snake_fused_kernel(const int8_t *__restrict__ uin, int8_t *__restrict__ uout, const SnakeProg g, const SnakeArgs<T> a,
                   double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sn_lds[];
    const int tid = threadIdx.x;
    const int H = g.nst;
    const int LX = g.tx + 2 * H, LY = g.ty + 2 * H, LZ = ND == 3 ? g.tz + 2 * H : 1;
    const int LYX = LY * LX;
    const int npos = LZ * LYX;
    unsigned char *buf[2] = {sn_lds, sn_lds + ((npos + 15) & ~15)};

    int b = blockIdx.x;
    const int xt = b % g.ntx;
    b /= g.ntx;
    const int yt = b % g.nty, zt = b / g.nty;
    // the voxel of local position (0, 0, 0)
    const int ox = xt * g.tx - H, oy = yt * g.ty - H, oz = ND == 3 ? zt * g.tz - H : 0;
    const int64_t plane = (int64_t)g.ny * g.nx;

    T c0 = T(0), c1 = T(0);
    if (a.state) {
        c0 = (T)a.state->c0;
        c1 = (T)a.state->c1;
    }

    for (int l = tid; l < npos; l += kSnNT) {
        const int lz = l / LYX, r = l - lz * LYX, ly = r / LX, lx = r - ly * LX;
        const int z = oz + lz, y = oy + ly, x = ox + lx;
        unsigned char v = 0;
        if (z >= 0 && z < g.nz && y >= 0 && y < g.ny && x >= 0 && x < g.nx) v = uin[z * plane + (int64_t)y * g.nx + x] != 0;
        buf[0][l] = v;
    }
    __syncthreads();

    for (int s = 0; s < H; s++) {
        const unsigned char *src = buf[s & 1];
        unsigned char *dst = buf[(s + 1) & 1];
        const int kind = g.kind[s];
        const int m = s + 1;                                   // the margin this stage leaves
        const int ex = LX - 2 * m, ey = LY - 2 * m, ez = ND == 3 ? LZ - 2 * m : 1;
        const int eyx = ey * ex, n = ez * eyx;
        for (int e = tid; e < n; e += kSnNT) {
            const int qz = e / eyx, r = e - qz * eyx, qy = r / ex, qx = r - qy * ex;
            const int lz = ND == 3 ? qz + m : 0, ly = qy + m, lx = qx + m;
            const int l = lz * LYX + ly * LX + lx;
            const int z = oz + lz, y = oy + ly, x = ox + lx;
            int v = 0;
            if (z >= 0 && z < g.nz && y >= 0 && y < g.ny && x >= 0 && x < g.nx) {
                const unsigned char *p = src + l;
                auto at = [&](int dz, int dy, int dx) -> int { return p[dz * LYX + dy * LX + dx]; };
                v = sn_eval<T, ND>(kind, at, (int)p[0], z, y, x, z * plane + (int64_t)y * g.nx + x, g, a, c0, c1);
            }
            dst[l] = (unsigned char)v;
        }
        __syncthreads();
    }

    const unsigned char *res = buf[H & 1];
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    const int cyx = g.ty * g.tx, ncore = (ND == 3 ? g.tz : 1) * cyx;
    for (int e = tid; e < ncore; e += kSnNT) {
        const int qz = e / cyx, r = e - qz * cyx, qy = r / g.tx, qx = r - qy * g.tx;
        const int lz = ND == 3 ? qz + H : 0, ly = qy + H, lx = qx + H;
        const int z = oz + lz, y = oy + ly, x = ox + lx;
        if (z < g.nz && y < g.ny && x < g.nx) {
            const int64_t gi = z * plane + (int64_t)y * g.nx + x;
            const int v = res[lz * LYX + ly * LX + lx];
            uout[gi] = (int8_t)v;
            if (g.sums) sn_accumulate<T>(s4, a.img[gi], v);
        }
    }
    if (g.sums) sn_block_partials(s4, part);
}

template <typename T, int ND>
__global__ void __launch_bounds__(kSnNT)
snake_generic_kernel(const int8_t *__restrict__ uin, int8_t *__restrict__ uout, const SnakeProg g, const SnakeArgs<T> a)
{
    const int64_t plane = (int64_t)g.ny * g.nx, total = plane * g.nz;
    T c0 = T(0), c1 = T(0);
    if (a.state) {
        c0 = (T)a.state->c0;
        c1 = (T)a.state->c1;
    }
    const int kind = g.kind[0];
    for (int64_t i = (int64_t)blockIdx.x * kSnNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kSnNT) {
        const int z = (int)(i / plane);
        const int64_t r = i - z * plane;
        const int y = (int)(r / g.nx), x = (int)(r - (int64_t)y * g.nx);
        auto at = [&](int dz, int dy, int dx) -> int {
            const int zz = z + dz, yy = y + dy, xx = x + dx;
            if (zz < 0 || zz >= g.nz || yy < 0 || yy >= g.ny || xx < 0 || xx >= g.nx) return 0;
            return uin[zz * plane + (int64_t)yy * g.nx + xx] != 0;
        };
        uout[i] = (int8_t)sn_eval<T, ND>(kind, at, (int)(uin[i] != 0), z, y, x, i, g, a, c0, c1);
    }
}

template <typename T>
__global__ void __launch_bounds__(kSnNT)
snake_sums_kernel(const T *__restrict__ img, const int8_t *__restrict__ u, int64_t total, double *__restrict__ part)
{
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kSnNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kSnNT)
        sn_accumulate<T>(s4, img[i], u[i] != 0);
    sn_block_partials(s4, part);
}

// One workgroup: thread t adds partials t, t + 256, ... in that order, a tree adds the threads; thread 0 forms c0 and c1 as
// the reference does (morphsnakes.py:359-360), every operand rounded to T first.
template <typename T>
__global__ void __launch_bounds__(kSnNT)
snake_finish_kernel(const double *__restrict__ part, int npart, SnakeState *state)
{
    __shared__ double red[4][kSnNT];
    const int tid = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < npart; i += kSnNT) {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] += part[4 * (int64_t)i + k];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) red[k][tid] = v[k];
    __syncthreads();
    for (int sft = kSnNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) {
#pragma unroll
            for (int k = 0; k < 4; k++) red[k][tid] += red[k][tid + sft];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int k = 0; k < 4; k++) state->sums[k] = red[k][0];
        state->c0 = (double)((T)red[0][0] / (T)(red[2][0] + 1e-8));
        state->c1 = (double)((T)red[1][0] / (T)(red[3][0] + 1e-8));
    }
}

// ------------------------------------------------------------------ order statistics (threshold = "auto")
// the smaller the value, the smaller the key; -0.0 below +0.0 (equal as values), NaN at the two far ends
template <typename T>
__device__ __forceinline__ unsigned long long sn_key(T v)
{
    if constexpr (sizeof(T) == 4) {
        const uint32_t b = __float_as_uint(v);
        return (b & 0x80000000u) ? (uint32_t)~b : (b | 0x80000000u);
    } else {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
}

template <typename T>
__global__ void __launch_bounds__(kSnNT)
snake_hist_kernel(const T *__restrict__ img, int64_t total, int shift, int first, SnakeSelect *sel)
{
    __shared__ unsigned int h[2][256];
    const int tid = threadIdx.x;
    h[0][tid] = 0;
    h[1][tid] = 0;
    __syncthreads();
    const unsigned long long p0 = sel->prefix[0], p1 = sel->prefix[1];
    for (int64_t i = (int64_t)blockIdx.x * kSnNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kSnNT) {
        const unsigned long long k = sn_key<T>(img[i]);
        const unsigned long long hi = first ? 0ull : k >> (shift + 8);
        const int bin = (int)((k >> shift) & 255u);
        if (first || hi == p0) atomicAdd(&h[0][bin], 1u);
        if (first || hi == p1) atomicAdd(&h[1][bin], 1u);
    }
    __syncthreads();
    // (a workgroup sees at most total / gridDim.x + 256 voxels of a grid-stride loop: well inside 32 bits)
    if (h[0][tid]) atomicAdd(&sel->hist[0][tid], (unsigned long long)h[0][tid]);
    if (h[1][tid]) atomicAdd(&sel->hist[1][tid], (unsigned long long)h[1][tid]);
}

template <typename T>
__global__ void snake_pick_kernel(SnakeSelect *sel, int first, int last, unsigned long long k0, unsigned long long k1, SnakeState *state)
{
    const int j = threadIdx.x;
    if (j < 2) {
        unsigned long long r = first ? (j ? k1 : k0) : sel->rank[j], cum = 0;
        int bin = 255;
        for (int k = 0; k < 256; k++) {
            const unsigned long long c = sel->hist[j][k];
            if (r < cum + c) {
                bin = k;
                break;
            }
            cum += c;
        }
        sel->rank[j] = r - cum;
        const unsigned long long key = (sel->prefix[j] << 8) | (unsigned long long)bin;
        sel->prefix[j] = key;
        if (last) {
            if constexpr (sizeof(T) == 4) {
                const uint32_t k32 = (uint32_t)key;
                const uint32_t bits = (k32 & 0x80000000u) ? (k32 & 0x7FFFFFFFu) : ~k32;
                state->stat[j] = (double)__uint_as_float(bits);
            } else {
                const unsigned long long bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
                state->stat[j] = __longlong_as_double((long long)bits);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 512; k += blockDim.x) sel->hist[k >> 8][k & 255] = 0;
}

// ------------------------------------------------------------------ small elementwise kernels
__global__ void __launch_bounds__(kSnNT)
snake_binarize_kernel(const void *__restrict__ src, int dt, int8_t *__restrict__ out, int64_t total, int nonzero)
{
    for (int64_t i = (int64_t)blockIdx.x * kSnNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kSnNT) {
        const double v = load_as_f64(src, i, dt);
        out[i] = (int8_t)(nonzero ? v != 0.0 : v > 0.0);
    }
}

template <typename T>
__global__ void __launch_bounds__(kSnNT)
snake_invgrad_kernel(const T *__restrict__ gm, T *__restrict__ out, int64_t total, T alpha)
{
    for (int64_t i = (int64_t)blockIdx.x * kSnNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kSnNT) {
        const T s = T(1) + alpha * gm[i];
        out[i] = T(1) / sqrt_t<T>(s);
    }
}

// ------------------------------------------------------------------ host side
// test / tuning hook: small core boxes (many seams), every stage on the generic kernel
static Knob g_sn_small{0}, g_sn_generic{0};
static std::atomic<int> g_sn_launches{0};

static inline void sn_count(int n = 1) { g_sn_launches.fetch_add(n, std::memory_order_relaxed); }

static int sn_grid(int64_t total)
{
    return capped_grid(total, kSnNT, kSnGenericMaxGrid);
}

static int sn_check_u(const mi_array *u, const char *name, const mi_array *like)
{
    int rc;
    if ((rc = check_array(u, name))) return rc;
    MI_REQUIRE(u->ndim == 2 || u->ndim == 3, MI_ERR_INVALID_ARG, "morphological snakes take arrays of rank 2 or 3");
    MI_REQUIRE(u->dtype == MI_I8, MI_ERR_INVALID_ARG, "the level set must be an int8 array");
    MI_REQUIRE(is_contiguous(u), MI_ERR_NOT_CONTIGUOUS, "morphological snakes need C-contiguous arrays");
    if (like) MI_REQUIRE(same_shape(u, like), MI_ERR_INVALID_ARG, "the level set must have the image's shape");
    for (int d = 0; d < u->ndim; d++) MI_REQUIRE(u->shape[d] < ((int64_t)1 << 30), MI_ERR_UNSUPPORTED, "axis too long");
    return MI_OK;
}

static int sn_check_image(const mi_array *image)
{
    int rc;
    if ((rc = check_array(image, "image"))) return rc;
    MI_REQUIRE(image->ndim == 2 || image->ndim == 3, MI_ERR_INVALID_ARG, "morphological snakes take arrays of rank 2 or 3");
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "morphological snakes need C-contiguous arrays");
    if (image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("morphological snakes: float32 and float64 images only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    return MI_OK;
}

static void sn_geom(const mi_array *u, SnakeProg *p)
{
    memset(p, 0, sizeof(*p));
    const bool vol = u->ndim == 3;
    p->nz = vol ? (int)u->shape[0] : 1;
    p->ny = (int)u->shape[vol ? 1 : 0];
    p->nx = (int)u->shape[vol ? 2 : 1];
}

// false: no tiling of this array for the fused kernel (more workgroups than partial sums)
static bool sn_plan(SnakeProg *p, bool vol)
{
    if (g_sn_small) {
        p->tz = vol ? 3 : 1; p->ty = 3; p->tx = 5;
    } else if (vol) {
        p->tz = 8; p->ty = 8; p->tx = 32;
    } else {
        p->tz = 1; p->ty = 16; p->tx = 64;
    }
    p->ntz = (p->nz + p->tz - 1) / p->tz;
    p->nty = (p->ny + p->ty - 1) / p->ty;
    p->ntx = (p->nx + p->tx - 1) / p->tx;
    return (int64_t)p->ntz * p->nty * p->ntx <= MI_SNAKE_MAX_PARTIALS;
}

static const char *sn_kind_name(int k)
{
    static const char *names[] = {"IS", "SI", "acwe", "gac", "dilate", "erode"};
    return names[k];
}

static void sn_describe(const SnakeProg &p, char *text, size_t n)
{
    size_t at = 0;
    text[0] = 0;
    for (int s = 0; s < p.nst && at + 8 < n; s++) at += (size_t)snprintf(text + at, n - at, "%s%s", s ? "+" : "", sn_kind_name(p.kind[s]));
}

// One launch of the stages p.kind[0 .. nst): fused, or (generic) exactly one stage.
template <typename T>
static int sn_launch(const int8_t *uin, int8_t *uout, SnakeProg p, const SnakeArgs<T> &a, bool vol, bool generic, double *part,
                     const char *what, int fused_smoothing, hipStream_t s)
{
    char stages[96];
    sn_describe(p, stages, sizeof(stages));
    const char *tn = sizeof(T) == 4 ? "float32" : "float64";
    if (generic) {
        const int grid = sn_grid((int64_t)p.nz * p.ny * p.nx);
        if (vol) hipLaunchKernelGGL((snake_generic_kernel<T, 3>), dim3(grid), dim3(kSnNT), 0, s, uin, uout, p, a);
        else hipLaunchKernelGGL((snake_generic_kernel<T, 2>), dim3(grid), dim3(kSnNT), 0, s, uin, uout, p, a);
        MI_HIP(hipGetLastError());
        sn_count();
        note_kernel("mi::snake_generic_kernel<%s,%s,%d> grid=%d stage=%s (one stage, one thread per voxel)",
                    what, tn, vol ? 3 : 2, grid, stages);
        return MI_OK;
    }
    const int H = p.nst;
    const size_t npos = (size_t)(vol ? p.tz + 2 * H : 1) * (p.ty + 2 * H) * (p.tx + 2 * H);
    const size_t lds = 2 * ((npos + 15) & ~(size_t)15);
    const int grid = p.ntz * p.nty * p.ntx;
    if (vol) hipLaunchKernelGGL((snake_fused_kernel<T, 3>), dim3(grid), dim3(kSnNT), lds, s, uin, uout, p, a, part);
    else hipLaunchKernelGGL((snake_fused_kernel<T, 2>), dim3(grid), dim3(kSnNT), lds, s, uin, uout, p, a, part);
    MI_HIP(hipGetLastError());
    sn_count();
    note_kernel("mi::snake_fused_kernel<%s,%s,%d,smoothing=%d> grid=%d box=%dx%dx%d halo=%d stages=%s%s", what, tn, vol ? 3 : 2, fused_smoothing, grid, p.tz, p.ty, p.tx, H, stages, p.sums ? " +sums" : "");
    return MI_OK;
}

// The launches of a chain of stages: the first takes `head` update stages and up to MI_SNAKE_FUSED_SMOOTHING smoothing steps
// (two stages each), every further one up to two smoothing steps; the generic route takes one launch per stage.  The
// launches alternate between u_out and u_tmp so that the last one writes u_out; u_in is only read.  want_sums: the last
// launch leaves the MorphACWE partials (*npart of them) -- the generic route adds a launch of snake_sums_kernel.
template <typename T>
static int sn_chain(const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, const int *kinds, int nkinds, int head,
                    const SnakeArgs<T> &a, bool want_sums, double *part, int *npart, const char *what, hipStream_t s)
{
    const bool vol = u_in->ndim == 3;
    SnakeProg base;
    sn_geom(u_in, &base);
    const bool generic = g_sn_generic != 0 || !sn_plan(&base, vol);
    // cut the chain into launches: [begin, end) of kinds
    constexpr int kMaxLaunches = 2 * 64 + 2;
    int cuts[kMaxLaunches + 1];
    int nl = 0, at = 0;
    MI_REQUIRE(nkinds >= 1 && nkinds <= kMaxLaunches, MI_ERR_INVALID_ARG, "1 to 130 stages");
    while (at < nkinds) {
        const int take = generic ? 1 : (nl == 0 ? head + 2 * MI_SNAKE_FUSED_SMOOTHING : 4);
        cuts[nl++] = at;
        at = std::min(nkinds, at + take);
    }
    cuts[nl] = nkinds;
    MI_REQUIRE(nl == 1 || u_tmp, MI_ERR_INVALID_ARG, "u_tmp is needed for a chain of more than one launch");
    const int8_t *src = (const int8_t *)u_in->data;
    for (int l = 0; l < nl; l++) {
        int8_t *dst = (int8_t *)(((nl - 1 - l) & 1) ? u_tmp->data : u_out->data);
        SnakeProg p = base;
        p.nst = cuts[l + 1] - cuts[l];
        for (int k = 0; k < p.nst; k++) p.kind[k] = kinds[cuts[l] + k];
        p.sums = want_sums && !generic && l == nl - 1;
        const int fused = l == 0 ? (p.nst - head) / 2 : p.nst / 2;
        int rc = sn_launch<T>(src, dst, p, a, vol, generic, part, what, fused, s);
        if (rc) return rc;
        src = dst;
    }
    if (want_sums) {
        if (generic) {
            const int64_t total = numel(u_in);
            const int grid = sn_grid(total);
            hipLaunchKernelGGL((snake_sums_kernel<T>), dim3(grid), dim3(kSnNT), 0, s, a.img, (const int8_t *)u_out->data, total, part);
            MI_HIP(hipGetLastError());
            sn_count();
            *npart = grid;
        } else {
            *npart = base.ntz * base.nty * base.ntx;
        }
    }
    return MI_OK;
}

// the stages of `smoothing` applications of the curvature operator, the first of them the `first`-th of its call:
// even: SI o IS (inf_sup first), odd: IS o SI
static int sn_smoothing_kinds(int *kinds, int at, int smoothing, int first)
{
    for (int j = 0; j < smoothing; j++) {
        const bool si_is = ((first + j) & 1) == 0;
        kinds[at++] = si_is ? SN_IS : SN_SI;
        kinds[at++] = si_is ? SN_SI : SN_IS;
    }
    return at;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_morphsnakes(int small_boxes, int force_generic)
{
    g_sn_small = small_boxes != 0;
    g_sn_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_debug_morphsnakes_launches(void)
{
    return g_sn_launches.load(std::memory_order_relaxed);
}

extern "C" int mi_snake_curvature(const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, int nops, unsigned ops, mi_stream stream)
{
    int rc;
    if ((rc = sn_check_u(u_in, "u_in", nullptr)) || (rc = sn_check_u(u_out, "u_out", u_in))) return rc;
    if (u_tmp && (rc = sn_check_u(u_tmp, "u_tmp", u_in))) return rc;
    MI_REQUIRE(nops >= 1 && nops <= 32, MI_ERR_INVALID_ARG, "1 to 32 operators");
    MI_REQUIRE(u_in->data != u_out->data && (!u_tmp || (u_tmp->data != u_in->data && u_tmp->data != u_out->data)), MI_ERR_INVALID_ARG,
               "u_in, u_out and u_tmp may not share memory");
    if (numel(u_in) == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    int kinds[32];
    for (int k = 0; k < nops; k++) kinds[k] = (ops >> k) & 1u ? SN_SI : SN_IS;
    SnakeArgs<float> a;
    memset(&a, 0, sizeof(a));
    int npart = 0;
    return sn_chain<float>(u_in, u_out, u_tmp, kinds, nops, 0, a, false, nullptr, &npart, "curvature", s);
}

template <typename T>
static int sn_finish(int npart, void *work_dev, hipStream_t s)
{
    double *part = (double *)((char *)work_dev + MI_SNAKE_STATE_BYTES);
    hipLaunchKernelGGL((snake_finish_kernel<T>), dim3(1), dim3(kSnNT), 0, s, (const double *)part, npart, (SnakeState *)work_dev);
    MI_HIP(hipGetLastError());
    sn_count();
    return MI_OK;
}

extern "C" int mi_snake_acwe_init(const mi_array *image, const mi_array *u, void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = sn_check_image(image)) || (rc = sn_check_u(u, "u", image))) return rc;
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    double *part = (double *)((char *)work_dev + MI_SNAKE_STATE_BYTES);
    const int grid = sn_grid(total);
    if (image->dtype == MI_F32)
        hipLaunchKernelGGL((snake_sums_kernel<float>), dim3(grid), dim3(kSnNT), 0, s, (const float *)image->data, (const int8_t *)u->data, total, part);
    else
        hipLaunchKernelGGL((snake_sums_kernel<double>), dim3(grid), dim3(kSnNT), 0, s, (const double *)image->data, (const int8_t *)u->data, total, part);
    MI_HIP(hipGetLastError());
    sn_count();
    note_kernel("mi::snake_sums_kernel<%s> grid=%d (the four sums of MorphACWE)", image->dtype == MI_F32 ? "float32" : "float64", grid);
    return image->dtype == MI_F32 ? sn_finish<float>(grid, work_dev, s) : sn_finish<double>(grid, work_dev, s);
}

template <typename T>
static int sn_acwe_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, double lambda1,
                        double lambda2, int smoothing, int first, void *work_dev, hipStream_t s)
{
    int kinds[2 * 64 + 2];
    kinds[0] = SN_ACWE;
    const int n = sn_smoothing_kinds(kinds, 1, smoothing, first);
    SnakeArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.img = (const T *)image->data;
    a.lam1 = (T)lambda1;
    a.lam2 = (T)lambda2;
    a.state = (const SnakeState *)work_dev;
    double *part = (double *)((char *)work_dev + MI_SNAKE_STATE_BYTES);
    int npart = 0;
    int rc = sn_chain<T>(u_in, u_out, u_tmp, kinds, n, 1, a, true, part, &npart, "acwe", s);
    if (rc) return rc;
    return sn_finish<T>(npart, work_dev, s);
}

extern "C" int mi_snake_acwe_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, double lambda1,
                                  double lambda2, int smoothing, int first, void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = sn_check_image(image)) || (rc = sn_check_u(u_in, "u_in", image)) || (rc = sn_check_u(u_out, "u_out", image))) return rc;
    if (u_tmp && (rc = sn_check_u(u_tmp, "u_tmp", image))) return rc;
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(smoothing >= 0 && smoothing <= 64 && first >= 0, MI_ERR_INVALID_ARG, "smoothing must be 0 to 64");
    MI_REQUIRE(u_in->data != u_out->data && (!u_tmp || (u_tmp->data != u_in->data && u_tmp->data != u_out->data)), MI_ERR_INVALID_ARG,
               "u_in, u_out and u_tmp may not share memory");
    for (int d = 0; d < image->ndim; d++) MI_REQUIRE(image->shape[d] != 1, MI_ERR_INVALID_ARG, "every axis must have at least 2 elements");
    if (numel(image) == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    return image->dtype == MI_F32 ? sn_acwe_step<float>(image, u_in, u_out, u_tmp, lambda1, lambda2, smoothing, first, work_dev, s)
                                  : sn_acwe_step<double>(image, u_in, u_out, u_tmp, lambda1, lambda2, smoothing, first, work_dev, s);
}

template <typename T>
static int sn_gac_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp, double mask_threshold,
                       int balloon, int smoothing, int first, hipStream_t s)
{
    int kinds[2 * 64 + 2];
    int head = 0;
    if (balloon) kinds[head++] = balloon > 0 ? SN_DILATE : SN_ERODE;
    kinds[head++] = SN_GAC;
    const int n = sn_smoothing_kinds(kinds, head, smoothing, first);
    SnakeArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.img = (const T *)image->data;
    a.mask_thr = mask_threshold;
    int npart = 0;
    return sn_chain<T>(u_in, u_out, u_tmp, kinds, n, head, a, false, nullptr, &npart, "gac", s);
}

extern "C" int mi_snake_gac_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const mi_array *u_tmp,
                                 double mask_threshold, int balloon, int smoothing, int first, mi_stream stream)
{
    int rc;
    if ((rc = sn_check_image(image)) || (rc = sn_check_u(u_in, "u_in", image)) || (rc = sn_check_u(u_out, "u_out", image))) return rc;
    if (u_tmp && (rc = sn_check_u(u_tmp, "u_tmp", image))) return rc;
    MI_REQUIRE(smoothing >= 0 && smoothing <= 64 && first >= 0, MI_ERR_INVALID_ARG, "smoothing must be 0 to 64");
    MI_REQUIRE(u_in->data != u_out->data && (!u_tmp || (u_tmp->data != u_in->data && u_tmp->data != u_out->data)), MI_ERR_INVALID_ARG,
               "u_in, u_out and u_tmp may not share memory");
    for (int d = 0; d < image->ndim; d++) MI_REQUIRE(image->shape[d] != 1, MI_ERR_INVALID_ARG, "every axis must have at least 2 elements");
    if (numel(image) == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    return image->dtype == MI_F32 ? sn_gac_step<float>(image, u_in, u_out, u_tmp, mask_threshold, balloon, smoothing, first, s)
                                  : sn_gac_step<double>(image, u_in, u_out, u_tmp, mask_threshold, balloon, smoothing, first, s);
}

template <typename T>
static int sn_order_stats(const mi_array *image, int64_t k0, int64_t k1, void *work_dev, hipStream_t s)
{
    SnakeSelect *sel = (SnakeSelect *)((char *)work_dev + MI_SNAKE_STATE_BYTES);
    MI_HIP(hipMemsetAsync(sel, 0, sizeof(SnakeSelect), s));
    const int64_t total = numel(image);
    const int grid = sn_grid(total);
    const int passes = (int)sizeof(T);
    for (int p = 0; p < passes; p++) {
        const int shift = 8 * (passes - 1 - p);
        hipLaunchKernelGGL((snake_hist_kernel<T>), dim3(grid), dim3(kSnNT), 0, s, (const T *)image->data, total, shift, p == 0, sel);
        hipLaunchKernelGGL((snake_pick_kernel<T>), dim3(1), dim3(kSnNT), 0, s, sel, p == 0, p == passes - 1, (unsigned long long)k0,
                           (unsigned long long)k1, (SnakeState *)work_dev);
        sn_count(2);
    }
    MI_HIP(hipGetLastError());
    note_kernel("mi::snake_hist_kernel<%s> grid=%d passes=%d (radix select of two order statistics)", sizeof(T) == 4 ? "float32" : "float64",
                grid, passes);
    return MI_OK;
}

extern "C" int mi_snake_order_stats(const mi_array *image, int64_t k0, int64_t k1, void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image"))) return rc;
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "morphological snakes need C-contiguous arrays");
    MI_REQUIRE(image->dtype == MI_F32 || image->dtype == MI_F64, MI_ERR_UNSUPPORTED, "float32 and float64 arrays only");
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    const int64_t total = numel(image);
    MI_REQUIRE(k0 >= 0 && k0 < total && k1 >= 0 && k1 < total, MI_ERR_INVALID_ARG, "rank outside the array");
    hipStream_t s = resolve_stream(stream);
    return image->dtype == MI_F32 ? sn_order_stats<float>(image, k0, k1, work_dev, s) : sn_order_stats<double>(image, k0, k1, work_dev, s);
}

extern "C" int mi_snake_binarize(const mi_array *src, const mi_array *out, int nonzero, mi_stream stream)
{
    int rc;
    if ((rc = check_array(src, "src")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(same_shape(src, out) && out->dtype == MI_I8, MI_ERR_INVALID_ARG, "out must be an int8 array of the source's shape");
    MI_REQUIRE(src->dtype != MI_F16, MI_ERR_UNSUPPORTED, "float16 arrays are storage only");
    MI_REQUIRE(is_contiguous(src) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "morphological snakes need C-contiguous arrays");
    MI_REQUIRE(src->data != out->data, MI_ERR_INVALID_ARG, "out may not be src");
    const int64_t total = numel(src);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    hipLaunchKernelGGL(snake_binarize_kernel, dim3(sn_grid(total)), dim3(kSnNT), 0, s, (const void *)src->data, src->dtype, (int8_t *)out->data,
                       total, nonzero);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_snake_inverse_gradient(const mi_array *gradnorm, const mi_array *out, double alpha, mi_stream stream)
{
    int rc;
    if ((rc = check_array(gradnorm, "gradnorm")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(same_shape(gradnorm, out) && out->dtype == gradnorm->dtype, MI_ERR_INVALID_ARG, "out must have the input's shape and dtype");
    MI_REQUIRE(gradnorm->dtype == MI_F32 || gradnorm->dtype == MI_F64, MI_ERR_UNSUPPORTED, "float32 and float64 arrays only");
    MI_REQUIRE(is_contiguous(gradnorm) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "morphological snakes need C-contiguous arrays");
    const int64_t total = numel(gradnorm);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int grid = sn_grid(total);
    if (gradnorm->dtype == MI_F32)
        hipLaunchKernelGGL((snake_invgrad_kernel<float>), dim3(grid), dim3(kSnNT), 0, s, (const float *)gradnorm->data, (float *)out->data, total, (float)alpha);
    else
        hipLaunchKernelGGL((snake_invgrad_kernel<double>), dim3(grid), dim3(kSnNT), 0, s, (const double *)gradnorm->data, (double *)out->data, total, alpha);
    MI_HIP(hipGetLastError());
    note_kernel("mi::snake_invgrad_kernel<%s> grid=%d (1 / sqrt(1 + alpha g))", gradnorm->dtype == MI_F32 ? "float32" : "float64", grid);
    return MI_OK;
}
