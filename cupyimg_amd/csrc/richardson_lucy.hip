// richardson_lucy.hip -- skimage.restoration.richardson_lucy: one iteration of Richardson-Lucy deconvolution per call.
//
// Reference path replaced: cupyimg/skimage/restoration/deconvolution.py:356-416 (per iteration two whole-array convolutions, a
// division, an optional where and a multiply: five or six passes over the volume and as many launches).
//
// The contract (include/mi355img.h, tests/helpers/rl_ref.py).  T is float or double, s the PSF's shape, every axis on its own:
//     c[i]     = sum_k psf[k] * u_in[i + (s - 1) / 2 - k]       the taps in C order of t = s - 1 - k (the reversed PSF)
//     r[i]     = image[i] / c[i];   r[i] = 0 where use_epsilon and c[i] < T(epsilon)
//     u_out[i] = u_in[i] * sum_j psf[j] * r[i - s / 2 + j]      the taps in C order of j
//     clip:      u_out > 1 -> 1, u_out < -1 -> -1 (a NaN stays)
// Both sums follow csrc/correlate_nd.hip's rule for dtype_mode="numpy": taps whose PSF value is 0.0 are skipped, every other
// product is formed and added in double, starting from +0.0, a sample outside the image is a 0 that is multiplied and added like
// any other, and the sum is rounded once to T.  The division and the final product are single operations in T.  Both sums reach
// from i - s / 2 to i + (s - 1) / 2 along every axis.  This file is compiled with -ffp-contract=off.
//
// Split route: rl_ratio_kernel writes r into a scratch volume, rl_update_kernel writes u_out; one thread per voxel over
// nd_common.hpp's tap tables, any rank, any PSF.  This route defines the bits.
//
// Fused route, rl_fused_kernel<T, ND> (ND 2 and 3), one launch: r never exists in memory.  A workgroup of 256 threads owns a tile
// of ty rows x tx columns and a chunk of planes, and streams along axis 0.  With lo = s / 2 and hi = (s - 1) / 2, an output plane
// z needs r on planes z - lo0 .. z + hi0 over the tile plus lo / hi in-plane, and an r plane q needs u on planes q - lo0 .. q + hi0
// over that box plus lo / hi once more: the staged u box has a halo of 2 * lo below and 2 * hi above along the tiled axes.  Both
// live in LDS as rings of s0 planes, in T.  Step p stages u plane p (zero outside the image); then the ring holds u planes
// p - (s0 - 1) .. p, exactly what r plane q = p - hi0 needs; r plane q goes to the r ring (exactly 0 outside the image, image read
// once), which then holds q - (s0 - 1) .. q, exactly what output plane z = q - hi0 = p - 2 * hi0 needs.  Two barriers a step: the
// u slot written at step p + 1 is the oldest, read last by the r sums of step p, which every thread has left at the second barrier
// of step p; the r slot written at step p + 1 is written after the first barrier of step p + 1, which no thread reaches before it
// has finished the output sums of step p.  Recomputation of r is in-plane only, plus s0 - 1 planes per chunk.  PSF values are read
// through uniform addresses (scalar loads).  Images are the same kernel with one plane and rings of one.
#include "nd_common.hpp"
#include "skimage_common.hpp"

namespace mi {

constexpr int kRlNT = 256;
constexpr int kRlLdsBytes = 64 * 1024;
constexpr int kRlSmallLdsBytes = 16 * 1024;     // mi_debug_set_richardson_lucy(2)

static Knob g_rl_route{0};                      // 0 the planner, 1 split everywhere, 2 fused on small tiles, 3 fused wherever it fits

template <typename T>
__device__ __forceinline__ T rl_ratio(T image, double c_sum, int use_eps, double eps)
{
    const T c = (T)c_sum;
    T r = image / c;
    if (use_eps && c < (T)eps) r = T(0);
    return r;
}

template <typename T>
__device__ __forceinline__ T rl_update(T u, double sum, int clip)
{
    T v = u * (T)sum;
    if (clip) {
        if (v > T(1)) v = T(1);
        if (v < T(-1)) v = T(-1);
    }
    return v;
}

// sum over the table's taps of src[tap] * value, samples outside the array 0
template <typename T, int ND>
__device__ __forceinline__ double rl_tap_sum(const T *__restrict__ src, const NdGeom &g, const TapTable &tt, int64_t i)
{
    const Voxel<ND> v = locate<ND>(g, i);
    double acc = 0.0;
    if (v.interior) {
        for (int t = 0; t < tt.ntaps; t++) acc += (double)src[i + tt.lin[t]] * tt.val[t];
    } else {
        for (int t = 0; t < tt.ntaps; t++) {
            const int64_t pos = tap_pos<ND>(g, v, tt.idx, t, MI_MODE_CONSTANT);
            const double x = pos < 0 ? 0.0 : (double)src[pos];
            acc += x * tt.val[t];
        }
    }
    return acc;
}

template <typename T, int ND>
__global__ void __launch_bounds__(kRlNT)
rl_ratio_kernel(const T *__restrict__ image, const T *__restrict__ u_in, T *__restrict__ r, NdGeom g, TapTable tt, int64_t total,
                int use_eps, double eps)
{
    for (int64_t i = (int64_t)blockIdx.x * kRlNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRlNT)
        r[i] = rl_ratio<T>(image[i], rl_tap_sum<T, ND>(u_in, g, tt, i), use_eps, eps);
}

template <typename T, int ND>
__global__ void __launch_bounds__(kRlNT)
rl_update_kernel(const T *__restrict__ u_in, const T *__restrict__ r, T *__restrict__ u_out, NdGeom g, TapTable tt, int64_t total, int clip)
{
    for (int64_t i = (int64_t)blockIdx.x * kRlNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRlNT)
        u_out[i] = rl_update<T>(u_in[i], rl_tap_sum<T, ND>(r, g, tt, i), clip);
}

struct RlParams {
    int n[3];           // planes, rows, columns (images: 1 plane)
    int s[3];           // the PSF
    int lo[3], hi[3];   // s / 2, (s - 1) / 2
    int ty, tx;         // outputs of a tile
    int nty, ntx;       // tiles per plane
    int zchunk, nzc;    // planes of a chunk, chunks
    int uy, ux, ry, rx; // rows and columns of the staged u box and of the r box
    int upitch, rpitch; // elements between two staged rows
    int use_eps, clip;
    double eps;
};

__device__ __forceinline__ int rl_slot(int plane, int depth)
{
    const int m = plane % depth;
    return m < 0 ? m + depth : m;
}

constexpr int kRlR = 4;                         // consecutive outputs of a thread along x
template <typename T>
struct alignas(16) RlVec {
    T v[kRlR];
};
static inline int rl_round4(int n) { return (n + 3) & ~3; }

// acc[r] += sum over the s0 x s1 x s2 window of ring sample (first_plane + t0, row + t1, c0 + r + t2) * psf value of the tap, for
// the kRlR outputs r of a thread, the taps in C order.  REVERSED: tap t takes psf[last - t] (the first sum), else psf[t].  The
// thread keeps a window of kRlR samples in registers and reads the next kRlR with one vector load per kRlR PSF columns; every
// PSF value is wave-uniform (a scalar load) and serves kRlR outputs.  c0 is a multiple of kRlR and so are the pitches, so the
// vector loads are aligned; they reach at most kRlR + 3 samples past the last one used, which the pitches leave room for.
template <typename T, bool REVERSED>
__device__ __forceinline__ void rl_window_sums(const T *__restrict__ ring, int plane_elems, int pitch, int depth, int first_plane,
                                               int row, int c0, const double *__restrict__ psf, int s0, int s1, int s2, double *acc)
{
    int t = REVERSED ? s0 * s1 * s2 - 1 : 0;
    constexpr int step = REVERSED ? -1 : 1;
    for (int t0 = 0; t0 < s0; t0++) {
        const T *pl = ring + rl_slot(first_plane + t0, depth) * plane_elems + c0;
        for (int t1 = 0; t1 < s1; t1++) {
            const T *line = pl + (row + t1) * pitch;
            double xw[kRlR], xn[kRlR];
            {
                const RlVec<T> cur = *reinterpret_cast<const RlVec<T> *>(line);
#pragma unroll
                for (int j = 0; j < kRlR; j++) xw[j] = (double)cur.v[j];
            }
            int t2 = 0;
            for (; t2 + kRlR <= s2; t2 += kRlR, t += kRlR * step) {
                const RlVec<T> nx = *reinterpret_cast<const RlVec<T> *>(line + t2 + kRlR);
                double w[kRlR];
#pragma unroll
                for (int j = 0; j < kRlR; j++) {
                    w[j] = psf[t + step * j];
                    xn[j] = (double)nx.v[j];
                }
#pragma unroll
                for (int j = 0; j < kRlR; j++) {
                    if (w[j] != 0.0) {
#pragma unroll
                        for (int r = 0; r < kRlR; r++) acc[r] += (j + r < kRlR ? xw[(j + r) % kRlR] : xn[(j + r) % kRlR]) * w[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < kRlR; j++) xw[j] = xn[j];
            }
            const int rem = s2 - t2;
            if (rem > 0) {
                const RlVec<T> nx = *reinterpret_cast<const RlVec<T> *>(line + t2 + kRlR);
#pragma unroll
                for (int j = 0; j < kRlR; j++) xn[j] = (double)nx.v[j];
#pragma unroll
                for (int j = 0; j < kRlR - 1; j++) {
                    if (j < rem) {
                        const double w = psf[t + step * j];
                        if (w != 0.0) {
#pragma unroll
                            for (int r = 0; r < kRlR; r++) acc[r] += (j + r < kRlR ? xw[(j + r) % kRlR] : xn[(j + r) % kRlR]) * w;
                        }
                    }
                }
                t += rem * step;
            }
        }
    }
}

template <typename T, int ND>
__global__ void __launch_bounds__(kRlNT)
rl_fused_kernel(const T *__restrict__ image, const T *__restrict__ u_in, T *__restrict__ u_out, const double *__restrict__ psf,
                const RlParams p, const int64_t ntiles)
{
    extern __shared__ __attribute__((aligned(16))) char rl_smem[];
    const int s0 = p.s[0], s1 = p.s[1], s2 = p.s[2];
    const int uplane = p.uy * p.upitch, rplane = p.ry * p.rpitch;
    T *ub = reinterpret_cast<T *>(rl_smem);
    T *rb = ub + s0 * uplane;
    const int64_t plane_elems = (int64_t)p.n[1] * p.n[2];
    const int rgroups = (p.rx + kRlR - 1) / kRlR, ogroups = (p.tx + kRlR - 1) / kRlR;
    // the staging walk of a thread: elements threadIdx.x, + 256, ... of a plane of uy rows of upitch columns, without a division a step
    const int drow = kRlNT / p.upitch, dcol = kRlNT % p.upitch;
    const int row_a = (int)threadIdx.x / p.upitch, col_a = (int)threadIdx.x % p.upitch;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int bx = (int)(tile % p.ntx);
        const int64_t rest = tile / p.ntx;
        const int by = (int)(rest % p.nty), bz = (int)(rest / p.nty);
        const int z0 = bz * p.zchunk, z1 = min(z0 + p.zchunk, p.n[0]);
        const int y0 = by * p.ty, x0 = bx * p.tx;
        for (int pz = z0 - 2 * p.lo[0]; pz <= z1 - 1 + 2 * p.hi[0]; pz++) {
            // (a) u plane pz -> its ring slot: box (row, col) is the sample at (pz, y0 - 2 lo1 + row, x0 - 2 lo2 + col); the columns
            // from ux to the pitch are zeros too
            {
                T *dst = ub + rl_slot(pz, s0) * uplane;
                const bool zin = pz >= 0 && pz < p.n[0];
                int row = row_a, col = col_a;
                while (row < p.uy) {
                    const int gy = y0 - 2 * p.lo[1] + row, gx = x0 - 2 * p.lo[2] + col;
                    T v = T(0);
                    if (zin && col < p.ux && gy >= 0 && gy < p.n[1] && gx >= 0 && gx < p.n[2])
                        v = u_in[(int64_t)pz * plane_elems + (int64_t)gy * p.n[2] + gx];
                    dst[row * p.upitch + col] = v;
                    row += drow;
                    col += dcol;
                    if (col >= p.upitch) {
                        col -= p.upitch;
                        row++;
                    }
                }
            }
            __syncthreads();
            // (b) r plane q: box (row, col) is the voxel (q, y0 - lo1 + row, x0 - lo2 + col); a thread takes kRlR columns
            const int q = pz - p.hi[0];
            if (q >= z0 - p.lo[0]) {
                T *dst = rb + rl_slot(q, s0) * rplane;
                const bool zin = q >= 0 && q < p.n[0];
                for (int e = threadIdx.x; e < p.ry * rgroups; e += kRlNT) {
                    const int row = e / rgroups, c0 = (e - row * rgroups) * kRlR;
                    const int gy = y0 - p.lo[1] + row, gx0 = x0 - p.lo[2] + c0;
                    RlVec<T> r;
#pragma unroll
                    for (int k = 0; k < kRlR; k++) r.v[k] = T(0);
                    if (zin && gy >= 0 && gy < p.n[1] && gx0 + kRlR > 0 && gx0 < p.n[2]) {
                        double acc[kRlR] = {0.0, 0.0, 0.0, 0.0};
                        rl_window_sums<T, true>(ub, uplane, p.upitch, s0, q - p.lo[0], row, c0, psf, s0, s1, s2, acc);
                        const T *img = image + (int64_t)q * plane_elems + (int64_t)gy * p.n[2];
#pragma unroll
                        for (int k = 0; k < kRlR; k++) {
                            const int gx = gx0 + k;
                            if (c0 + k < p.rx && gx >= 0 && gx < p.n[2]) r.v[k] = rl_ratio<T>(img[gx], acc[k], p.use_eps, p.eps);
                        }
                    }
                    *reinterpret_cast<RlVec<T> *>(dst + row * p.rpitch + c0) = r;
                }
            }
            __syncthreads();
            // (c) output plane z over the tile
            const int z = pz - 2 * p.hi[0];
            if (z >= z0 && z < z1) {
                for (int e = threadIdx.x; e < p.ty * ogroups; e += kRlNT) {
                    const int row = e / ogroups, c0 = (e - row * ogroups) * kRlR;
                    const int gy = y0 + row, gx0 = x0 + c0;
                    if (gy >= p.n[1] || gx0 >= p.n[2]) continue;
                    double acc[kRlR] = {0.0, 0.0, 0.0, 0.0};
                    rl_window_sums<T, false>(rb, rplane, p.rpitch, s0, z - p.lo[0], row, c0, psf, s0, s1, s2, acc);
                    const int64_t o = (int64_t)z * plane_elems + (int64_t)gy * p.n[2];
#pragma unroll
                    for (int k = 0; k < kRlR; k++) {
                        const int gx = gx0 + k;
                        if (c0 + k < p.tx && gx < p.n[2]) u_out[o + gx] = rl_update<T>(u_in[o + gx], acc[k], p.clip);
                    }
                }
            }
        }
        // no barrier between tiles: the last output sums read the r ring only, which the next tile writes after its first barrier
    }
}

// The tile, the rings and the chunks of the fused kernel.  false: the staged boxes do not fit the budget with one output row.
// Pitches: a multiple of kRlR that leaves the vector loads of rl_window_sums kRlR + 3 samples past the last window of a row.
static bool rl_plan(RlParams *p, int rank, size_t es, bool small, int64_t *lds_bytes)
{
    const int64_t budget = small ? kRlSmallLdsBytes : kRlLdsBytes;
    p->tx = small ? 5 : 64;
    p->ux = p->tx + 2 * (p->s[2] - 1);
    p->rx = p->tx + p->s[2] - 1;
    p->upitch = rl_round4(rl_round4(p->rx) + p->s[2] + 3);
    p->rpitch = rl_round4(rl_round4(p->tx) + p->s[2] + 3);
    auto bytes = [&](int ty) {
        const int64_t uy = ty + 2 * (p->s[1] - 1), ry = ty + p->s[1] - 1;
        return (int64_t)p->s[0] * (uy * p->upitch + ry * p->rpitch) * (int64_t)es;
    };
    int ty = small ? 3 : 32;
    while (ty > 1 && bytes(ty) > budget) ty = small ? ty - 1 : ty / 2;
    if (bytes(ty) > budget) return false;
    p->ty = ty;
    p->uy = ty + 2 * (p->s[1] - 1);
    p->ry = ty + p->s[1] - 1;
    p->nty = (p->n[1] + p->ty - 1) / p->ty;
    p->ntx = (p->n[2] + p->tx - 1) / p->tx;
    // planes are cut into chunks only as far as it takes to give every CU about four workgroups: a chunk recomputes s0 - 1 planes of r
    if (small) {
        p->zchunk = 3;
    } else {
        const int64_t inplane = (int64_t)p->nty * p->ntx, want = 4 * (int64_t)device_cus();
        int64_t nzc = std::max<int64_t>(1, std::min<int64_t>(p->n[0], (want + inplane - 1) / inplane));
        p->zchunk = (int)((p->n[0] + nzc - 1) / nzc);
    }
    p->nzc = (p->n[0] + p->zchunk - 1) / p->zchunk;
    *lds_bytes = bytes(ty);
    return true;
}

// Where the fused kernel was measured faster than the split route (profiles/richardson_lucy.txt): on all six cases
// measured, images and volumes, float32 and float64, 25 to 225 taps, by 2.0 to 3.7 times; no case is routed away.  A case that
// measures slower belongs here.
static bool rl_planner_takes_fused(int rank, size_t es, const RlParams &p)
{
    (void)rank; (void)es; (void)p;
    return true;
}

static PerDeviceOnce g_rl_attr[4];

template <typename T, int ND>
static int rl_launch_fused(const T *image, const T *u_in, T *u_out, const double *psf_host, RlParams &p, int64_t lds_bytes, int slot,
                           const char *tname, hipStream_t s)
{
    Scratch spsf;
    int rc;
    if ((rc = spsf.upload(psf_host, (size_t)p.s[0] * p.s[1] * p.s[2] * sizeof(double), s))) return rc;
    if (!g_rl_attr[slot]) {
        MI_HIP(hipFuncSetAttribute((const void *)rl_fused_kernel<T, ND>, hipFuncAttributeMaxDynamicSharedMemorySize, kRlLdsBytes));
        g_rl_attr[slot] = true;
    }
    const int64_t ntiles = (int64_t)p.nzc * p.nty * p.ntx;
    const int grid = box_grid(ntiles);
    hipLaunchKernelGGL((rl_fused_kernel<T, ND>), dim3(grid), dim3(kRlNT), (size_t)lds_bytes, s, image, u_in, u_out, (const double *)spsf.ptr, p, ntiles);
    MI_HIP(hipGetLastError());
    note_kernel("mi::rl_fused_kernel<%s,%d> grid=%d tile=%dx%d chunk=%d ring=%d lds=%lld (one launch: u and r in LDS rings, streamed along axis 0)",
                tname, ND, grid, p.ty, p.tx, p.zchunk, p.s[0], (long long)lds_bytes);
    return MI_OK;
}

template <typename T>
static int rl_launch_split(const mi_array *image, const T *u_in, T *u_out, const double *psf, const int64_t *psf_shape, int use_eps,
                           double eps, int clip, void *scratch, const char *tname, hipStream_t s)
{
    int rc;
    int origins[MI_MAX_NDIM] = {0};
    int64_t ntot = 1;
    for (int d = 0; d < image->ndim; d++) ntot *= psf_shape[d];
    TapBuilder fwd, bwd;
    if ((rc = fwd.init(image, psf_shape, origins, "psf")) || (rc = bwd.init(image, psf_shape, origins, "psf"))) return rc;
    fwd.fill([&](int64_t k) { return psf[ntot - 1 - k] != 0.0; }, [&](int64_t k) { return psf[ntot - 1 - k]; }, true);
    bwd.fill([&](int64_t k) { return psf[k] != 0.0; }, [&](int64_t k) { return psf[k]; }, true);
    TapTable tf, tb;
    if ((rc = fwd.upload(&tf, s)) || (rc = bwd.upload(&tb, s))) return rc;
    const int64_t total = numel(image);
    void *own = nullptr;
    if (!scratch) {
        if ((rc = pool_alloc(&own, (size_t)total * sizeof(T), s))) return rc;
        scratch = own;
    }
    T *r = (T *)scratch;
    const T *img = (const T *)image->data;
    const int grid = capped_grid(total, kRlNT, 1 << 16);
    if (fwd.g.ndim == 3) {
        hipLaunchKernelGGL((rl_ratio_kernel<T, 3>), dim3(grid), dim3(kRlNT), 0, s, img, u_in, r, fwd.g, tf, total, use_eps, eps);
        hipLaunchKernelGGL((rl_update_kernel<T, 3>), dim3(grid), dim3(kRlNT), 0, s, u_in, (const T *)r, u_out, bwd.g, tb, total, clip);
    } else {
        hipLaunchKernelGGL((rl_ratio_kernel<T, MI_MAX_NDIM>), dim3(grid), dim3(kRlNT), 0, s, img, u_in, r, fwd.g, tf, total, use_eps, eps);
        hipLaunchKernelGGL((rl_update_kernel<T, MI_MAX_NDIM>), dim3(grid), dim3(kRlNT), 0, s, u_in, (const T *)r, u_out, bwd.g, tb, total, clip);
    }
    const hipError_t e = hipGetLastError();
    if (own) pool_free(own);
    MI_HIP(e);
    note_kernel("mi::rl_ratio_kernel<%s,%d> + mi::rl_update_kernel<%s,%d> grid=%d taps=%d+%d (two launches: one thread per voxel, r in a scratch volume)",
                tname, fwd.g.ndim, tname, fwd.g.ndim, grid, tf.ntaps, tb.ntaps);
    return MI_OK;
}

// fills p and says whether this call goes to the fused kernel under the current route setting
static bool rl_route_fused(const mi_array *image, const int64_t *psf_shape, RlParams *p, int64_t *lds_bytes)
{
    const int rank = image->ndim, route = g_rl_route;
    if (route == 1 || (rank != 2 && rank != 3)) return false;
    memset(p, 0, sizeof(*p));
    p->n[0] = p->s[0] = 1;
    for (int d = 0; d < rank; d++) {
        const int a = d + 3 - rank;
        if (image->shape[d] >= ((int64_t)1 << 30) || psf_shape[d] > 32767) return false;
        p->n[a] = (int)image->shape[d];
        p->s[a] = (int)psf_shape[d];
    }
    for (int a = 0; a < 3; a++) {
        p->lo[a] = p->s[a] / 2;
        p->hi[a] = (p->s[a] - 1) / 2;
    }
    const size_t es = dtype_size(image->dtype);
    if (!rl_plan(p, rank, es, route == 2, lds_bytes)) return false;
    return route >= 2 || rl_planner_takes_fused(rank, es, *p);
}

template <typename T>
static int rl_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const double *psf, const int64_t *psf_shape,
                   double eps, int use_eps, int clip, void *scratch, const char *tname, hipStream_t s)
{
    RlParams p;
    int64_t lds_bytes = 0;
    const T *img = (const T *)image->data, *ui = (const T *)u_in->data;
    T *uo = (T *)u_out->data;
    if (rl_route_fused(image, psf_shape, &p, &lds_bytes)) {
        p.use_eps = use_eps;
        p.clip = clip;
        p.eps = eps;
        const int slot = (sizeof(T) == 8 ? 2 : 0) + (image->ndim == 3 ? 1 : 0);
        if (image->ndim == 3) return rl_launch_fused<T, 3>(img, ui, uo, psf, p, lds_bytes, slot, tname, s);
        return rl_launch_fused<T, 2>(img, ui, uo, psf, p, lds_bytes, slot, tname, s);
    }
    return rl_launch_split<T>(image, ui, uo, psf, psf_shape, use_eps, eps, clip, scratch, tname, s);
}

static int rl_check(const mi_array *image, const int64_t *psf_shape)
{
    int rc;
    if ((rc = check_array(image, "image"))) return rc;
    MI_REQUIRE(image->ndim >= 1, MI_ERR_INVALID_ARG, "richardson_lucy: arrays of rank 1 to MI_MAX_NDIM");
    MI_REQUIRE(psf_shape, MI_ERR_INVALID_ARG, "NULL argument");
    if (image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("richardson_lucy: float32 and float64 only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    for (int d = 0; d < image->ndim; d++)
        MI_REQUIRE(psf_shape[d] >= 1, MI_ERR_INVALID_ARG, "richardson_lucy: a PSF of at least one sample along every axis");
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_richardson_lucy(int route)
{
    g_rl_route = route >= 1 && route <= 3 ? route : 0;
    return MI_OK;
}

extern "C" int mi_richardson_lucy_needs_scratch(const mi_array *image, const int64_t *psf_shape, int *needs_scratch)
{
    int rc;
    if ((rc = rl_check(image, psf_shape))) return rc;
    MI_REQUIRE(needs_scratch, MI_ERR_INVALID_ARG, "NULL argument");
    RlParams p;
    int64_t lds_bytes;
    *needs_scratch = rl_route_fused(image, psf_shape, &p, &lds_bytes) ? 0 : 1;
    return MI_OK;
}

extern "C" int mi_richardson_lucy_step(const mi_array *image, const mi_array *u_in, const mi_array *u_out, const double *psf,
                                       const int64_t *psf_shape, double filter_epsilon, int use_epsilon, int clip, void *scratch_dev,
                                       mi_stream stream)
{
    int rc;
    if ((rc = rl_check(image, psf_shape)) || (rc = check_array(u_in, "u_in")) || (rc = check_array(u_out, "u_out"))) return rc;
    MI_REQUIRE(psf, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(same_shape(image, u_in) && same_shape(image, u_out), MI_ERR_INVALID_ARG, "richardson_lucy: u_in and u_out have the image's shape");
    MI_REQUIRE(u_in->dtype == image->dtype && u_out->dtype == image->dtype, MI_ERR_INVALID_ARG, "richardson_lucy: u_in and u_out have the image's dtype");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(u_in) && is_contiguous(u_out), MI_ERR_NOT_CONTIGUOUS, "richardson_lucy needs C-contiguous arrays");
    MI_REQUIRE(u_out->data != u_in->data && u_out->data != image->data, MI_ERR_INVALID_ARG, "richardson_lucy: u_out overlaps neither u_in nor the image");
    if (numel(image) == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    use_epsilon = use_epsilon != 0;
    clip = clip != 0;
    if (image->dtype == MI_F32)
        return rl_step<float>(image, u_in, u_out, psf, psf_shape, filter_epsilon, use_epsilon, clip, scratch_dev, "float32", s);
    return rl_step<double>(image, u_in, u_out, psf, psf_shape, filter_epsilon, use_epsilon, clip, scratch_dev, "float64", s);
}
