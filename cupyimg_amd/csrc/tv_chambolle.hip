// tv_chambolle.hip -- total-variation denoising by Chambolle's projection algorithm (skimage.restoration.denoise_tv_chambolle):
// one launch per iteration plus a one-workgroup energy / stop step, no host round trip inside the loop.
//
// Reference path replaced: cupyimg/skimage/restoration/_denoise.py:6-87, which runs one iteration as about 25 whole-array
// operations (roughly 40 volume passes, two full reductions and a host synchronisation for the stopping test).
//
// One iteration, per voxel q, p_a the component of the dual field along axis a, n_a that axis' length, T the image dtype,
// all arithmetic in T and this file compiled with -ffp-contract=off (every product and sum rounds on its own):
//
//     d(q)   = -((p_0(q) + p_1(q)) + p_2(q) ...)  then, for a = 0, 1, ...:  d += p_a(q - e_a) where q_a >= 1
//     out(q) = image(q) + d(q)
//     g_a(q) = out(q + e_a) - out(q) where q_a < n_a - 1, else 0
//     norm   = sqrt(((g_0 g_0 + g_1 g_1) + g_2 g_2) ...)
//     den    = norm * T(tau / weight) + 1
//     p_a'   = (p_a - T(tau) g_a) / den
//     E_i    = (sum_q d d + weight * sum_q norm) / size        products d d in T, both sums and E in double
//
// tv_fused_kernel (C-contiguous 3-D volumes, 2-D images as one plane without the dead axis): a workgroup owns a tile of
// ty x TX voxels in the plane and a chunk of planes, and streams along axis 0.  `out` is never stored: it lives in a window
// of two planes in LDS, on the tile plus one voxel towards larger y and x; for that, p_in is staged on the tile plus one
// voxel either way (two planes: the update of plane z needs out(z + 1), hence p_in(z + 1), before p_in(z) is used up).  Every
// position of the staged window belongs to ONE thread for the whole chunk, which updates it (plane z) and then stages it
// (plane z + 2) in the same phase, so the plane loop needs two barriers: stage -> out -> (update, stage) ...
// A workgroup writes its own voxels of p_out and two double partial sums; nothing crosses workgroups inside a launch.
//
// tv_generic_kernel: the same arithmetic with one thread per voxel straight from global memory, ranks 1 .. MI_MAX_NDIM.
// tv_energy_kernel: one workgroup adds the partials in a fixed order, forms E_i and applies the stopping rule in the state block.
// tv_output_kernel: out = image + d(p).
#include "skimage_common.hpp"

namespace mi {

constexpr int kTvNT = 256;

// the first MI_TV_STATE_BYTES of the caller's work block (include/mi355img.h)
struct TvState {
    int32_t stopped;        // 1: the stopping rule held in iteration `stop_iter`; later launches return at once
    int32_t stop_iter;
    int32_t done;           // iterations that ran (the one that stopped included)
    int32_t pad;
    double e_prev, e_init, e_last;
    double spare[3];
};
static_assert(sizeof(TvState) == MI_TV_STATE_BYTES, "state block layout");

struct TvParams {
    int nx, ny, nz;
    int ty;                 // rows of a tile (its columns: the template argument)
    int zc;                 // planes of a chunk
    int nxt, nyt, nzc;
};

// the two partial sums of a workgroup, reduced in a fixed order (a tree over the thread index): no floating-point atomics
__device__ __forceinline__ void tv_block_partials(double sdd, double snorm, double *__restrict__ part)
{
    __shared__ double red[2][kTvNT];
    const int tid = threadIdx.x;
    red[0][tid] = sdd;
    red[1][tid] = snorm;
    __syncthreads();
    for (int sft = kTvNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) {
            red[0][tid] += red[0][tid + sft];
            red[1][tid] += red[1][tid + sft];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = red[0][0];
        part[2 * (int64_t)blockIdx.x + 1] = red[1][0];
    }
}

// VOL: axis 0 is an axis of the array (p has 3 components); false: an image as one plane (2 components, no p_0)
template <typename T, bool VOL, int TX>
__global__ void __launch_bounds__(kTvNT)
tv_fused_kernel(const T *__restrict__ img, const T *__restrict__ pin, T *__restrict__ pout, const TvParams g, const T tau, const T tw,
                double *__restrict__ part, const TvState *__restrict__ state)
{
    if (state->stopped) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_lds[];
    constexpr int NC = VOL ? 3 : 2;
    constexpr int LX = TX + 2;
    constexpr int C1 = VOL ? 1 : 0, C2 = VOL ? 2 : 1;      // components of the y and x axes
    const int tid = threadIdx.x;
    const int LY = g.ty + 2;
    const int npos = LY * LX;
    // staged position l = ly * LX + lx  <->  voxel (y0 - 1 + ly, x0 - 1 + lx)
    T *P = reinterpret_cast<T *>(tv_lds);            // [2][NC][npos]  p_in of two planes
    T *O = P + 2 * NC * npos;                        // [2][npos]      out of two planes
    T *I = O + 2 * npos;                             // [npos]         image of the plane being staged

    int b = blockIdx.x;
    const int xt = b % g.nxt;
    b /= g.nxt;
    const int yt = b % g.nyt, zt = b / g.nyt;
    const int x0 = xt * TX, y0 = yt * g.ty, z0 = zt * g.zc;
    const int z1 = min(g.nz, z0 + g.zc);                     // own planes: z0 .. z1 - 1
    const int zend = min(z1, g.nz - 1);                      // last plane whose `out` is needed
    const int64_t plane = (int64_t)g.ny * g.nx;
    const int64_t total = plane * g.nz;

    double sdd = 0.0, snorm = 0.0;

    if (VOL && z0 >= 1) {
        // p_0 of the plane below the chunk: what out(z0) takes from it
        T *Pb = P + ((z0 - 1) & 1) * NC * npos;
        for (int l = tid; l < npos; l += kTvNT) {
            const int ly = l / LX, lx = l - ly * LX;
            const int y = y0 - 1 + ly, x = x0 - 1 + lx;
            if (ly >= 1 && lx >= 1 && y < g.ny && x < g.nx) Pb[l] = pin[(int64_t)(z0 - 1) * plane + (int64_t)y * g.nx + x];
        }
    }

    for (int k = z0; k <= zend + 2; k++) {
        // ---- phase 1: update plane k - 2 (needs out(k - 2) and out(k - 1)), then stage plane k over what it used
        const int zu = k - 2;
        const bool upd = zu >= z0 && zu < z1, stg = k <= zend;
        if (upd || stg) {
            const int bu = zu & 1;                            // == k & 1
            T *Pb = P + bu * NC * npos;
            const T *Ob = O + bu * npos, *On = O + (bu ^ 1) * npos;
            for (int l = tid; l < npos; l += kTvNT) {
                const int ly = l / LX, lx = l - ly * LX;
                const int y = y0 - 1 + ly, x = x0 - 1 + lx;
                const bool in_arr = y >= 0 && x >= 0 && y < g.ny && x < g.nx;
                if (!in_arr) continue;
                const int64_t gi = (int64_t)y * g.nx + x;
                T s0 = T(0), s1 = T(0), s2 = T(0), si = T(0);
                if (stg) {
                    // the loads of the next plane first: they fly while the update below computes
                    const int64_t q = (int64_t)k * plane + gi;
                    // (the row before the tile is read for p_y only, the column before it for p_x only)
                    if (VOL && ly >= 1 && lx >= 1) s0 = pin[q];
                    if (lx >= 1) s1 = pin[C1 * total + q];
                    if (ly >= 1) s2 = pin[C2 * total + q];
                    if (ly >= 1 && lx >= 1) si = img[q];
                }
                if (upd && ly >= 1 && ly <= g.ty && lx >= 1 && lx <= TX) {
                    const T o = Ob[l];
                    const T g0 = (VOL && zu < g.nz - 1) ? On[l] - o : T(0);
                    const T g1 = y < g.ny - 1 ? Ob[l + LX] - o : T(0);
                    const T g2 = x < g.nx - 1 ? Ob[l + 1] - o : T(0);
                    T n2;
                    if (VOL) n2 = (g0 * g0 + g1 * g1) + g2 * g2;
                    else n2 = g1 * g1 + g2 * g2;
                    const T nrm = sqrt_t<T>(n2);
                    snorm += (double)nrm;
                    const T den = nrm * tw + T(1);
                    const int64_t q = (int64_t)zu * plane + gi;
                    if (VOL) pout[q] = (Pb[l] - tau * g0) / den;
                    pout[C1 * total + q] = (Pb[C1 * npos + l] - tau * g1) / den;
                    pout[C2 * total + q] = (Pb[C2 * npos + l] - tau * g2) / den;
                }
                if (stg) {
                    if (VOL) Pb[l] = s0;
                    Pb[C1 * npos + l] = s1;
                    Pb[C2 * npos + l] = s2;
                    I[l] = si;
                }
            }
        }
        __syncthreads();
        // ---- phase 2: out(k) on the tile plus one voxel towards larger y and x
        if (stg) {
            const int bk = k & 1;
            const T *Pb = P + bk * NC * npos, *Pp = P + (bk ^ 1) * NC * npos;
            T *Ob = O + bk * npos;
            for (int l = tid; l < npos; l += kTvNT) {
                const int ly = l / LX, lx = l - ly * LX;
                const int y = y0 - 1 + ly, x = x0 - 1 + lx;
                if (ly < 1 || lx < 1 || y >= g.ny || x >= g.nx) continue;
                T d;
                if (VOL) d = -((Pb[l] + Pb[C1 * npos + l]) + Pb[C2 * npos + l]);
                else d = -(Pb[C1 * npos + l] + Pb[C2 * npos + l]);
                if (VOL && k >= 1) d += Pp[l];
                if (y >= 1) d += Pb[C1 * npos + l - LX];
                if (x >= 1) d += Pb[C2 * npos + l - 1];
                Ob[l] = I[l] + d;
                if (k < z1 && ly <= g.ty && lx <= TX) sdd += (double)(d * d);
            }
        }
        __syncthreads();
    }
    tv_block_partials(sdd, snorm, part);
}

// The per-voxel kernels are built for the ranks 1 .. 4 (ND = the rank: trip counts known to the compiler) and once for
// 5 .. MI_MAX_NDIM (ND = MI_MAX_NDIM, axes beyond g.nd skipped at run time).
#define TV_AXIS(a) (ND != MI_MAX_NDIM || (a) < g.nd)

// d(q) for the voxel at linear index i with coordinates c
template <typename T, int ND>
__device__ __forceinline__ T tv_d_at(const T *__restrict__ p, const VoxelGeom<MI_MAX_NDIM> &g, int64_t i, const int64_t *c)
{
    T s = p[i];
#pragma unroll
    for (int a = 1; a < ND; a++)
        if (TV_AXIS(a)) s = s + p[a * g.total + i];
    T d = -s;
#pragma unroll
    for (int a = 0; a < ND; a++)
        if (TV_AXIS(a) && c[a] >= 1) d += p[a * g.total + i - g.stride[a]];
    return d;
}

template <typename T, int ND>
__global__ void __launch_bounds__(kTvNT)
tv_generic_kernel(const T *__restrict__ img, const T *__restrict__ pin, T *__restrict__ pout, const VoxelGeom<MI_MAX_NDIM> g, const T tau, const T tw,
                  double *__restrict__ part, const TvState *__restrict__ state)
{
    if (state->stopped) return;
    double sdd = 0.0, snorm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kTvNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kTvNT) {
        int64_t c[ND];
        voxel_coords<ND, ND == MI_MAX_NDIM>(g, i, c);
        const T d = tv_d_at<T, ND>(pin, g, i, c);
        const T o = img[i] + d;
        sdd += (double)(d * d);
        T gr[ND];
        T n2 = T(0);
#pragma unroll
        for (int a = 0; a < ND; a++) {
            gr[a] = T(0);
            if (TV_AXIS(a)) {
                if (c[a] < g.shape[a] - 1) {
                    const int64_t j = i + g.stride[a];
                    c[a] += 1;
                    gr[a] = (img[j] + tv_d_at<T, ND>(pin, g, j, c)) - o;
                    c[a] -= 1;
                }
                n2 = a == 0 ? gr[a] * gr[a] : n2 + gr[a] * gr[a];
            }
        }
        const T nrm = sqrt_t<T>(n2);
        snorm += (double)nrm;
        const T den = nrm * tw + T(1);
#pragma unroll
        for (int a = 0; a < ND; a++)
            if (TV_AXIS(a)) pout[a * g.total + i] = (pin[a * g.total + i] - tau * gr[a]) / den;
    }
    tv_block_partials(sdd, snorm, part);
}

template <typename T, int ND>
__global__ void __launch_bounds__(kTvNT)
tv_output_kernel(const T *__restrict__ img, const T *__restrict__ p, T *__restrict__ out, const VoxelGeom<MI_MAX_NDIM> g)
{
    for (int64_t i = (int64_t)blockIdx.x * kTvNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kTvNT) {
        int64_t c[ND];
        voxel_coords<ND, ND == MI_MAX_NDIM>(g, i, c);
        out[i] = img[i] + tv_d_at<T, ND>(p, g, i, c);
    }
}

// One workgroup: thread t adds partials t, t + 256, ... in that order, a tree adds the threads; thread 0 forms E_i and
// applies the rule.  The order depends on nothing but the number of partials.
__global__ void __launch_bounds__(kTvNT)
tv_energy_kernel(const double *__restrict__ part, int npart, double weight, double eps, double size, int iteration, TvState *state)
{
    if (state->stopped) return;
    __shared__ double red[2][kTvNT];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = tid; i < npart; i += kTvNT) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    red[0][tid] = a;
    red[1][tid] = b;
    __syncthreads();
    for (int sft = kTvNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) {
            red[0][tid] += red[0][tid + sft];
            red[1][tid] += red[1][tid + sft];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double e = (red[0][0] + weight * red[1][0]) / size;
        state->e_last = e;
        state->done = iteration + 1;
        if (iteration == 0) {
            state->e_init = e;
            state->e_prev = e;
        } else if (fabs(state->e_prev - e) < eps * state->e_init) {
            state->stop_iter = iteration;
            state->stopped = 1;
        } else {
            state->e_prev = e;
        }
    }
}

// test / tuning hook: tile rows, planes per chunk (0 = the planner's), 8-column tiles, every call on the generic kernel
static Knob g_tv_ty{0}, g_tv_zc{0}, g_tv_narrow{0}, g_tv_generic{0};

constexpr int kTvGenericMaxGrid = 2048;

template <typename T, bool VOL, int TX>
static int launch_tv_fused(const mi_array *image, const mi_array *p_in, const mi_array *p_out, const TvParams &p, size_t lds, double tau,
                           double weight, double *part, TvState *state, hipStream_t s)
{
    static PerDeviceOnce attr;
    if (!attr) {
        MI_HIP(hipFuncSetAttribute((const void *)tv_fused_kernel<T, VOL, TX>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        attr = true;
    }
    const int grid = p.nxt * p.nyt * p.nzc;
    hipLaunchKernelGGL((tv_fused_kernel<T, VOL, TX>), dim3((unsigned)grid), dim3(kTvNT), lds, s, (const T *)image->data,
                       (const T *)p_in->data, (T *)p_out->data, p, (T)tau, (T)(tau / weight), part, (const TvState *)state);
    MI_HIP(hipGetLastError());
    note_kernel("mi::tv_fused_kernel<%s,%s> grid=%d tile=%dx%d chunk=%d (one Chambolle iteration: out in an LDS plane window, streamed along axis 0)",
                sizeof(T) == 4 ? "float32" : "float64", VOL ? "volume" : "image", grid, p.ty, TX, p.zc);
    return MI_OK;
}

// MI_ERR_UNSUPPORTED (nothing queued): not a shape of the fused kernel
static int tv_fused(const mi_array *image, const mi_array *p_in, const mi_array *p_out, double tau, double weight, double *part,
                    TvState *state, int *npart, hipStream_t s)
{
    const bool vol = image->ndim == 3;
    const int64_t nz = vol ? image->shape[0] : 1, ny = image->shape[vol ? 1 : 0], nx = image->shape[vol ? 2 : 1];
    if (nz >= ((int64_t)1 << 24) || ny >= ((int64_t)1 << 24) || nx >= ((int64_t)1 << 24)) return MI_ERR_UNSUPPORTED;
    const int es = (int)dtype_size(image->dtype);
    const bool narrow = g_tv_narrow != 0;
    const int tx = narrow ? 8 : 64;
    TvParams p;
    memset(&p, 0, sizeof(p));
    p.nx = (int)nx; p.ny = (int)ny; p.nz = (int)nz;
    // 16 rows of 64 voxels (8 rows for float64): 9 staged planes of (ty + 2) x 66 elements = 43 / 48 KiB, three workgroups a CU
    p.ty = es == 8 ? 8 : 16;
    if (g_tv_ty) p.ty = std::min((int)g_tv_ty, p.ty);
    p.ty = (int)std::min<int64_t>(p.ty, ny);
    p.nxt = (int)((nx + tx - 1) / tx);
    p.nyt = (int)((ny + p.ty - 1) / p.ty);
    const int64_t tiles = (int64_t)p.nxt * p.nyt;
    if (tiles > MI_TV_MAX_PARTIALS) return MI_ERR_UNSUPPORTED;
    // chunks of planes: a chunk pays one extra staged plane at its end (and p_0 of the plane below it), so at least 16
    // planes each (6 %); no more chunks than it takes to give every CU a few workgroups
    int64_t nzc;
    if (g_tv_zc) nzc = (nz + (int)g_tv_zc - 1) / (int)g_tv_zc;
    else nzc = std::max<int64_t>(1, std::min<int64_t>((1024 + tiles - 1) / tiles, nz / 16));
    nzc = std::min<int64_t>(nzc, MI_TV_MAX_PARTIALS / tiles);
    p.zc = (int)((nz + nzc - 1) / nzc);
    p.nzc = (int)((nz + p.zc - 1) / p.zc);
    const size_t lds = (size_t)((vol ? 3 : 2) * 2 + 3) * (p.ty + 2) * (tx + 2) * es;
    *npart = p.nxt * p.nyt * p.nzc;
#define TV_GO(T)                                                                                                             \
    (vol ? (narrow ? launch_tv_fused<T, true, 8>(image, p_in, p_out, p, lds, tau, weight, part, state, s)                     \
                   : launch_tv_fused<T, true, 64>(image, p_in, p_out, p, lds, tau, weight, part, state, s))                   \
         : (narrow ? launch_tv_fused<T, false, 8>(image, p_in, p_out, p, lds, tau, weight, part, state, s)                    \
                   : launch_tv_fused<T, false, 64>(image, p_in, p_out, p, lds, tau, weight, part, state, s)))
    return image->dtype == MI_F32 ? TV_GO(float) : TV_GO(double);
#undef TV_GO
}

static int tv_check(const mi_array *image, const mi_array *p, const char *name)
{
    int rc;
    if ((rc = check_array(p, name))) return rc;
    MI_REQUIRE(p->ndim == 2 && p->shape[0] == image->ndim && p->shape[1] == numel(image), MI_ERR_INVALID_ARG,
               "p must have shape (image.ndim, image.size)");
    MI_REQUIRE(p->dtype == image->dtype, MI_ERR_INVALID_ARG, "p must have the image's dtype");
    MI_REQUIRE(is_contiguous(p), MI_ERR_NOT_CONTIGUOUS, "tv_chambolle needs C-contiguous arrays");
    return MI_OK;
}

static int tv_check_image(const mi_array *image)
{
    int rc;
    if ((rc = check_array(image, "image"))) return rc;
    MI_REQUIRE(image->ndim >= 1, MI_ERR_INVALID_ARG, "image must have at least one dimension");
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "tv_chambolle needs C-contiguous arrays");
    if (image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("tv_chambolle: float32 and float64 arrays only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    return MI_OK;
}

// GO(T, ND) for the image's dtype and rank
#define TV_BY_RANK(GO)                                                  \
    do {                                                                \
        const bool f32__ = image->dtype == MI_F32;                      \
        switch (image->ndim) {                                          \
        case 1: if (f32__) GO(float, 1); else GO(double, 1); break;     \
        case 2: if (f32__) GO(float, 2); else GO(double, 2); break;     \
        case 3: if (f32__) GO(float, 3); else GO(double, 3); break;     \
        case 4: if (f32__) GO(float, 4); else GO(double, 4); break;     \
        default: if (f32__) GO(float, MI_MAX_NDIM); else GO(double, MI_MAX_NDIM); break; \
        }                                                               \
    } while (0)

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_tv_chambolle(int tile_rows, int chunk_planes, int narrow_tiles, int force_generic)
{
    g_tv_ty = tile_rows < 0 ? 0 : tile_rows;
    g_tv_zc = chunk_planes < 0 ? 0 : chunk_planes;
    g_tv_narrow = narrow_tiles != 0;
    g_tv_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_tv_chambolle_step(const mi_array *image, const mi_array *p_in, const mi_array *p_out, double weight, double eps,
                                    int iteration, void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = tv_check_image(image)) || (rc = tv_check(image, p_in, "p_in")) || (rc = tv_check(image, p_out, "p_out"))) return rc;
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(iteration >= 0, MI_ERR_INVALID_ARG, "iteration must not be negative");
    MI_REQUIRE(p_in->data != p_out->data, MI_ERR_INVALID_ARG, "p_out may not be p_in");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    TvState *state = (TvState *)work_dev;
    double *part = (double *)((char *)work_dev + MI_TV_STATE_BYTES);
    const double tau = 1.0 / (2.0 * image->ndim);
    int npart = 0;
    rc = MI_ERR_UNSUPPORTED;
    if (!g_tv_generic && (image->ndim == 2 || image->ndim == 3)) rc = tv_fused(image, p_in, p_out, tau, weight, part, state, &npart, s);
    if (rc == MI_ERR_UNSUPPORTED) {
        VoxelGeom<MI_MAX_NDIM> g;
        voxel_geom(image, &g);
        npart = capped_grid(total, kTvNT, kTvGenericMaxGrid);          // total >= 1 here
#define TV_GEN(T, ND)                                                                                                         \
    hipLaunchKernelGGL((tv_generic_kernel<T, ND>), dim3(npart), dim3(kTvNT), 0, s, (const T *)image->data, (const T *)p_in->data, \
                       (T *)p_out->data, g, (T)tau, (T)(tau / weight), part, (const TvState *)state)
        TV_BY_RANK(TV_GEN);
#undef TV_GEN
        MI_HIP(hipGetLastError());
        note_kernel("mi::tv_generic_kernel<%s> grid=%d (one Chambolle iteration, one thread per voxel, rank %d)",
                    image->dtype == MI_F32 ? "float32" : "float64", npart, image->ndim);
    } else if (rc) {
        return rc;
    }
    hipLaunchKernelGGL(tv_energy_kernel, dim3(1), dim3(kTvNT), 0, s, (const double *)part, npart, weight, eps, (double)total, iteration, state);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_tv_chambolle_output(const mi_array *image, const mi_array *p, const mi_array *out, mi_stream stream)
{
    int rc;
    if ((rc = tv_check_image(image)) || (rc = tv_check(image, p, "p")) || (rc = check_array(out, "out"))) return rc;
    MI_REQUIRE(same_shape(image, out) && out->dtype == image->dtype, MI_ERR_INVALID_ARG, "out must have the image's shape and dtype");
    MI_REQUIRE(is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "tv_chambolle needs C-contiguous arrays");
    MI_REQUIRE(out->data != image->data && out->data != p->data, MI_ERR_INVALID_ARG, "out may not overlap image or p in memory");
    const int64_t total = numel(image);
    if (total == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    VoxelGeom<MI_MAX_NDIM> g;
    voxel_geom(image, &g);
    const int grid = capped_grid(total, kTvNT, 65536);
#define TV_OUT(T, ND)                                                                                                         \
    hipLaunchKernelGGL((tv_output_kernel<T, ND>), dim3(grid), dim3(kTvNT), 0, s, (const T *)image->data, (const T *)p->data,      \
                       (T *)out->data, g)
    TV_BY_RANK(TV_OUT);
#undef TV_OUT
    MI_HIP(hipGetLastError());
    return MI_OK;
}
