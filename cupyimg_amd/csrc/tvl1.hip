// tvl1.hip -- the TV-L1 optical flow solver (skimage.registration.optical_flow_tvl1): two launches per fixed-point iteration.
//
// Reference path replaced: cupyimg/skimage/registration/_optical_flow.py:20-158, which runs one fixed-point iteration as about
// 140 whole-array operations (boolean-mask gathers and scatters among them).
//
// T is the image dtype (float32 / float64); all arithmetic in T, this file compiled with -ffp-contract=off (every product and
// sum rounds on its own), sums over the component axis left to right.  n_a: length of axis a, e_a its unit vector.
//
// tvl1_prepare_kernel (once per warp), w the warped moving image, r the reference image, u the flow:
//     grad_a(q) = (w(q + e_a) - w(q - e_a)) / 2 inside, w(1) - w(0) and w(n_a - 1) - w(n_a - 2) at the ends   (numpy.gradient)
//     NI(q)     = (grad_0 grad_0 + grad_1 grad_1) + ...,  1 where that is 0
//     rho_0(q)  = (w(q) - r(q)) - ((grad_0 u_0 + grad_1 u_1) + ...)
// tvl1_data_kernel (the data term, in place on the flow; what it leaves is the reference's flow_auxiliary):
//     rho = rho_0 + ((grad_0 u_0 + grad_1 u_1) + ...)
//     |rho| <= T(f0) NI :  u_a -= (rho grad_a) / NI          else:  u_a -= (T(f0) sign(rho)) grad_a
// the regularisation of flow component c, v = flow_auxiliary[c], p = proj[c] (ndim components), u^0 = v, twice (s = 1, 2):
//     g_a(q)   = u^(s-1)(q + e_a) - u^(s-1)(q) where q_a < n_a - 1, else 0
//     norm     = sqrt((g_0 g_0 + g_1 g_1) + ...) * T(f1) + 1
//     p^s_a    = (p^(s-1)_a - T(dt) g_a) / norm
//     d(q)     = -((p^s_0(q) + p^s_1(q)) + ...), then for a = 0, 1, ...: d += p^s_a(q - e_a) where q_a >= 1
//     u^s(q)   = v(q) + d(q)
// new flow[c] = u^2, new proj[c] = p^2.
//
// Dependencies of a tile [0, t) along one axis, backwards: u^2 and p^2 on [0, t) <- p^2 on [-1, t) <- u^1 on [-1, t] and p^1 on
// [-1, t) <- (u^1) p^1 on [-2, t] <- p^0 on [-2, t] and v on [-2, t + 1].  So v is staged on the tile plus 2 voxels either way
// and p^0 on the tile plus 2 voxels towards smaller and 1 towards larger indices.
//
// tvl1_reg_fused_kernel (C-contiguous 3-D volumes; 2-D images as one plane without the dead axis): a workgroup owns one flow
// component of a tile of ty x TX voxels in the plane and a chunk of planes and streams along axis 0.  Rings in LDS, every
// plane on the tile plus 2 voxels either way: v (4 planes), p (4 planes of ndim components, updated in place p^0 -> p^1 ->
// p^2) and u^1 (2 planes).  Step t: stage plane t (its loads were issued a step earlier and waited in registers); p^1(t - 1);
// u^1(t - 1); p^2(t - 2); u^2(t - 2) and the stores.  A workgroup writes its own voxels of the output flow and proj only, into
// buffers that no workgroup reads in this launch.
//
// tvl1_step_p_kernel / tvl1_step_u_kernel: the same arithmetic as four launches with one thread per voxel straight from global
// memory (u^1 and p^1 in a scratch array), ranks 2 .. 4; the forced comparison route for 2-D and 3-D.
// tvl1_diff_kernel / tvl1_diff_final_kernel: sum (a - b)^2, the difference and its square in T, the sum in double from
// per-workgroup partials in an order fixed by the size: no floating-point atomics.
#include "skimage_common.hpp"

namespace mi {

constexpr int kFlNT = 256;
constexpr int kFlMaxNd = 4;
constexpr int kFlMaxGrid = 4096;
constexpr int kFlDiffGrid = 1024;

template <typename T, int ND>
__global__ void __launch_bounds__(kFlNT)
tvl1_coords_kernel(const T *__restrict__ flow, T *__restrict__ out, const VoxelGeom<kFlMaxNd> g)
{
    for (int64_t i = (int64_t)blockIdx.x * kFlNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kFlNT) {
        int64_t c[ND];
        voxel_coords<ND, false>(g, i, c);
#pragma unroll
        for (int a = 0; a < ND; a++) out[a * g.total + i] = (T)c[a] + flow[a * g.total + i];
    }
}

template <typename T, int ND>
__global__ void __launch_bounds__(kFlNT)
tvl1_prepare_kernel(const T *__restrict__ w, const T *__restrict__ ref, const T *__restrict__ flow, T *__restrict__ grad,
                    T *__restrict__ ni, T *__restrict__ rho0, const VoxelGeom<kFlMaxNd> g)
{
    for (int64_t i = (int64_t)blockIdx.x * kFlNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kFlNT) {
        int64_t c[ND];
        voxel_coords<ND, false>(g, i, c);
        const T wi = w[i];
        T s = T(0), dot = T(0);
#pragma unroll
        for (int a = 0; a < ND; a++) {
            const int64_t st = g.stride[a];
            T gr;
            if (c[a] == 0) gr = w[i + st] - wi;
            else if (c[a] == g.shape[a] - 1) gr = wi - w[i - st];
            else gr = (w[i + st] - w[i - st]) / T(2);
            grad[a * g.total + i] = gr;
            const T f = flow[a * g.total + i];
            s = a == 0 ? gr * gr : s + gr * gr;
            dot = a == 0 ? gr * f : dot + gr * f;
        }
        ni[i] = s == T(0) ? T(1) : s;
        rho0[i] = (wi - ref[i]) - dot;
    }
}

template <typename T, int ND>
__global__ void __launch_bounds__(kFlNT)
tvl1_data_kernel(const T *__restrict__ grad, const T *__restrict__ ni, const T *__restrict__ rho0, T *__restrict__ flow, int64_t total,
                 const T f0)
{
    for (int64_t i = (int64_t)blockIdx.x * kFlNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kFlNT) {
        T gr[ND], u[ND];
        T dot = T(0);
#pragma unroll
        for (int a = 0; a < ND; a++) {
            gr[a] = grad[a * total + i];
            u[a] = flow[a * total + i];
            dot = a == 0 ? gr[a] * u[a] : dot + gr[a] * u[a];
        }
        const T rho = rho0[i] + dot;
        const T n = ni[i];
        if ((rho < T(0) ? -rho : rho) <= f0 * n) {
#pragma unroll
            for (int a = 0; a < ND; a++) flow[a * total + i] = u[a] - (rho * gr[a]) / n;
        } else {
            const T sg = rho > T(0) ? T(1) : (rho < T(0) ? T(-1) : rho);
            const T srho = f0 * sg;
#pragma unroll
            for (int a = 0; a < ND; a++) flow[a * total + i] = u[a] - srho * gr[a];
        }
    }
}

// p_out[c] = one dual step of p_in[c] against u[c]; index over (component, voxel)
template <typename T, int ND>
__global__ void __launch_bounds__(kFlNT)
tvl1_step_p_kernel(const T *__restrict__ u, const T *__restrict__ pin, T *__restrict__ pout, const VoxelGeom<kFlMaxNd> g, const T dt, const T f1)
{
    const int64_t all = g.total * ND;
    for (int64_t j = (int64_t)blockIdx.x * kFlNT + threadIdx.x; j < all; j += (int64_t)gridDim.x * kFlNT) {
        const int64_t cmp = j / g.total, i = j - cmp * g.total;
        int64_t c[ND];
        voxel_coords<ND, false>(g, i, c);
        const T *uc = u + cmp * g.total;
        const T u0 = uc[i];
        T gr[ND];
        T s = T(0);
#pragma unroll
        for (int a = 0; a < ND; a++) {
            gr[a] = c[a] < g.shape[a] - 1 ? uc[i + g.stride[a]] - u0 : T(0);
            s = a == 0 ? gr[a] * gr[a] : s + gr[a] * gr[a];
        }
        T norm = sqrt_t<T>(s);
        norm = norm * f1;
        norm = norm + T(1);
#pragma unroll
        for (int a = 0; a < ND; a++) {
            const int64_t k = (cmp * ND + a) * g.total + i;
            pout[k] = (pin[k] - dt * gr[a]) / norm;
        }
    }
}

// out[c] = v[c] - div p[c]
template <typename T, int ND>
__global__ void __launch_bounds__(kFlNT)
tvl1_step_u_kernel(const T *__restrict__ v, const T *__restrict__ p, T *__restrict__ out, const VoxelGeom<kFlMaxNd> g)
{
    const int64_t all = g.total * ND;
    for (int64_t j = (int64_t)blockIdx.x * kFlNT + threadIdx.x; j < all; j += (int64_t)gridDim.x * kFlNT) {
        const int64_t cmp = j / g.total, i = j - cmp * g.total;
        int64_t c[ND];
        voxel_coords<ND, false>(g, i, c);
        const T *pc = p + cmp * ND * g.total;
        T s = pc[i];
#pragma unroll
        for (int a = 1; a < ND; a++) s = s + pc[a * g.total + i];
        T d = -s;
#pragma unroll
        for (int a = 0; a < ND; a++)
            if (c[a] >= 1) d += pc[a * g.total + i - g.stride[a]];
        out[j] = v[j] + d;
    }
}

struct FlParams {
    int nx, ny, nz;
    int ty;                 // rows of a tile (its columns: the template argument)
    int zc;                 // planes of a chunk
    int nxt, nyt, nzc;
};

// VOL: axis 0 is an axis of the array (3 components); false: an image as one plane (2 components)
template <typename T, bool VOL, int TX>
__global__ void __launch_bounds__(kFlNT)
tvl1_reg_fused_kernel(const T *__restrict__ vin, const T *__restrict__ pin, T *__restrict__ uout, T *__restrict__ pout, const FlParams g,
                      const T dt, const T f1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fl_lds[];
    constexpr int NC = VOL ? 3 : 2;
    constexpr int LX = TX + 4;
    constexpr int CY = VOL ? 1 : 0, CX = VOL ? 2 : 1;      // components of the y and x axes
    const int tid = threadIdx.x;
    const int LY = g.ty + 4;
    const int npos = LY * LX;
    // staged position l = ly * LX + lx  <->  voxel (y0 - 2 + ly, x0 - 2 + lx)
    T *A = reinterpret_cast<T *>(fl_lds);            // [4][npos]       v
    T *P = A + 4 * npos;                             // [4][NC][npos]   p^0, then p^1, then p^2
    T *U = P + 4 * NC * npos;                        // [2][npos]       u^1

    int b = blockIdx.x;
    const int xt = b % g.nxt;
    b /= g.nxt;
    const int yt = b % g.nyt, zt = b / g.nyt;
    const int cmp = blockIdx.y;
    const int x0 = xt * TX, y0 = yt * g.ty, z0 = zt * g.zc;
    const int z1 = min(g.nz, z0 + g.zc);                     // own planes: z0 .. z1 - 1
    const int64_t plane = (int64_t)g.ny * g.nx;
    const int64_t total = plane * g.nz;
    const T *v = vin + (int64_t)cmp * total;
    const T *p0 = pin + (int64_t)cmp * NC * total;
    T *po = pout + (int64_t)cmp * NC * total;
    T *uo = uout + (int64_t)cmp * total;
    const int zlast = g.nz - 1;
    const int kp_lo = max(0, z0 - 2), kp_hi = min(zlast, z1);           // planes of p^0 / p^1
    const int ka_hi = min(zlast, z1 + 1);                               // planes of v: kp_lo .. ka_hi
    const int ku_lo = max(0, z0 - 1);                                   // planes of u^1: ku_lo .. kp_hi; of p^2: ku_lo .. z1 - 1

    // The loads of plane t + 1 are issued before the four compute phases of step t and land in registers; the stage phase of
    // step t + 1 only moves them to LDS.  Position j of a thread: l = tid + j * kFlNT.
    constexpr int NPT = (12 * LX + kFlNT - 1) / kFlNT;      // ty <= 8
    T rv[NPT], rp[NPT][NC];
    auto fetch = [&](int k) {
        if (k > ka_hi) return;
        const bool withp = k <= kp_hi;
#pragma unroll
        for (int j = 0; j < NPT; j++) {
            const int l = tid + j * kFlNT;
            const int ly = l / LX, lx = l - ly * LX;
            const int y = y0 - 2 + ly, x = x0 - 2 + lx;
            if (l >= npos || y < 0 || x < 0 || y >= g.ny || x >= g.nx) continue;
            const int64_t q = (int64_t)k * plane + (int64_t)y * g.nx + x;
            rv[j] = v[q];
            if (withp && ly < LY - 1 && lx < LX - 1) {
                if (VOL) rp[j][0] = p0[q];
                rp[j][CY] = p0[CY * total + q];
                rp[j][CX] = p0[CX * total + q];
            }
        }
    };
    fetch(kp_lo);

    for (int t = kp_lo; t <= z1 + 1; t++) {
        // ---- stage plane t (out of the registers), then start the loads of plane t + 1
        if (t <= ka_hi) {
            T *Ab = A + (t & 3) * npos;
            T *Pb = P + (t & 3) * NC * npos;
            const bool withp = t <= kp_hi;
#pragma unroll
            for (int j = 0; j < NPT; j++) {
                const int l = tid + j * kFlNT;
                const int ly = l / LX, lx = l - ly * LX;
                const int y = y0 - 2 + ly, x = x0 - 2 + lx;
                if (l >= npos || y < 0 || x < 0 || y >= g.ny || x >= g.nx) continue;
                Ab[l] = rv[j];
                if (withp && ly < LY - 1 && lx < LX - 1) {
                    if (VOL) Pb[l] = rp[j][0];
                    Pb[CY * npos + l] = rp[j][CY];
                    Pb[CX * npos + l] = rp[j][CX];
                }
            }
        }
        fetch(t + 1);
        __syncthreads();
        // ---- p^1 of plane t - 1, from v
        {
            const int k = t - 1;
            if (k >= kp_lo && k <= kp_hi) {
                const T *Ab = A + (k & 3) * npos, *An = A + ((k + 1) & 3) * npos;
                T *Pb = P + (k & 3) * NC * npos;
                for (int l = tid; l < npos; l += kFlNT) {
                    const int ly = l / LX, lx = l - ly * LX;
                    const int y = y0 - 2 + ly, x = x0 - 2 + lx;
                    if (ly >= LY - 1 || lx >= LX - 1 || y < 0 || x < 0 || y >= g.ny || x >= g.nx) continue;
                    const T o = Ab[l];
                    const T gz = (VOL && k < zlast) ? An[l] - o : T(0);
                    const T gy = y < g.ny - 1 ? Ab[l + LX] - o : T(0);
                    const T gx = x < g.nx - 1 ? Ab[l + 1] - o : T(0);
                    T n2;
                    if (VOL) n2 = (gz * gz + gy * gy) + gx * gx;
                    else n2 = gy * gy + gx * gx;
                    T norm = sqrt_t<T>(n2);
                    norm = norm * f1;
                    norm = norm + T(1);
                    if (VOL) Pb[l] = (Pb[l] - dt * gz) / norm;
                    Pb[CY * npos + l] = (Pb[CY * npos + l] - dt * gy) / norm;
                    Pb[CX * npos + l] = (Pb[CX * npos + l] - dt * gx) / norm;
                }
            }
        }
        __syncthreads();
        // ---- u^1 of plane t - 1
        {
            const int k = t - 1;
            if (k >= ku_lo && k <= kp_hi) {
                const T *Ab = A + (k & 3) * npos;
                const T *Pb = P + (k & 3) * NC * npos, *Pp = P + ((k - 1) & 3) * NC * npos;
                T *Ub = U + (k & 1) * npos;
                for (int l = tid; l < npos; l += kFlNT) {
                    const int ly = l / LX, lx = l - ly * LX;
                    const int y = y0 - 2 + ly, x = x0 - 2 + lx;
                    if (ly < 1 || lx < 1 || ly >= LY - 1 || lx >= LX - 1 || y < 0 || x < 0 || y >= g.ny || x >= g.nx) continue;
                    T d;
                    if (VOL) d = -((Pb[l] + Pb[CY * npos + l]) + Pb[CX * npos + l]);
                    else d = -(Pb[CY * npos + l] + Pb[CX * npos + l]);
                    if (VOL && k >= 1) d += Pp[l];
                    if (y >= 1) d += Pb[CY * npos + l - LX];
                    if (x >= 1) d += Pb[CX * npos + l - 1];
                    Ub[l] = Ab[l] + d;
                }
            }
        }
        __syncthreads();
        // ---- p^2 of plane t - 2, from u^1
        {
            const int k = t - 2;
            if (k >= ku_lo && k < z1) {
                const T *Ub = U + (k & 1) * npos, *Un = U + ((k + 1) & 1) * npos;
                T *Pb = P + (k & 3) * NC * npos;
                for (int l = tid; l < npos; l += kFlNT) {
                    const int ly = l / LX, lx = l - ly * LX;
                    const int y = y0 - 2 + ly, x = x0 - 2 + lx;
                    if (ly < 1 || lx < 1 || ly >= LY - 2 || lx >= LX - 2 || y < 0 || x < 0 || y >= g.ny || x >= g.nx) continue;
                    const T o = Ub[l];
                    const T gz = (VOL && k < zlast) ? Un[l] - o : T(0);
                    const T gy = y < g.ny - 1 ? Ub[l + LX] - o : T(0);
                    const T gx = x < g.nx - 1 ? Ub[l + 1] - o : T(0);
                    T n2;
                    if (VOL) n2 = (gz * gz + gy * gy) + gx * gx;
                    else n2 = gy * gy + gx * gx;
                    T norm = sqrt_t<T>(n2);
                    norm = norm * f1;
                    norm = norm + T(1);
                    if (VOL) Pb[l] = (Pb[l] - dt * gz) / norm;
                    Pb[CY * npos + l] = (Pb[CY * npos + l] - dt * gy) / norm;
                    Pb[CX * npos + l] = (Pb[CX * npos + l] - dt * gx) / norm;
                }
            }
        }
        __syncthreads();
        // ---- u^2 of plane t - 2 and the stores of the tile's own voxels
        {
            const int k = t - 2;
            if (k >= z0 && k < z1) {
                const T *Ab = A + (k & 3) * npos;
                const T *Pb = P + (k & 3) * NC * npos, *Pp = P + ((k - 1) & 3) * NC * npos;
                for (int l = tid; l < npos; l += kFlNT) {
                    const int ly = l / LX, lx = l - ly * LX;
                    const int y = y0 - 2 + ly, x = x0 - 2 + lx;
                    if (ly < 2 || lx < 2 || ly >= LY - 2 || lx >= LX - 2 || y >= g.ny || x >= g.nx) continue;
                    T d;
                    if (VOL) d = -((Pb[l] + Pb[CY * npos + l]) + Pb[CX * npos + l]);
                    else d = -(Pb[CY * npos + l] + Pb[CX * npos + l]);
                    if (VOL && k >= 1) d += Pp[l];
                    if (y >= 1) d += Pb[CY * npos + l - LX];
                    if (x >= 1) d += Pb[CX * npos + l - 1];
                    const int64_t q = (int64_t)k * plane + (int64_t)y * g.nx + x;
                    uo[q] = Ab[l] + d;
                    if (VOL) po[q] = Pb[l];
                    po[CY * total + q] = Pb[CY * npos + l];
                    po[CX * total + q] = Pb[CX * npos + l];
                }
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(kFlNT)
tvl1_diff_kernel(const T *__restrict__ a, const T *__restrict__ b, int64_t n, double *__restrict__ part)
{
    __shared__ double red[kFlNT];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kFlNT + tid; i < n; i += (int64_t)gridDim.x * kFlNT) {
        const T d = a[i] - b[i];
        s += (double)(d * d);
    }
    red[tid] = s;
    __syncthreads();
    for (int sft = kFlNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) red[tid] += red[tid + sft];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// one workgroup: thread t adds partials t, t + 256, ... in that order, a tree adds the threads
__global__ void __launch_bounds__(kFlNT)
tvl1_diff_final_kernel(const double *__restrict__ part, int npart, double *__restrict__ result)
{
    __shared__ double red[kFlNT];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < npart; i += kFlNT) s += part[i];
    red[tid] = s;
    __syncthreads();
    for (int sft = kFlNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) red[tid] += red[tid + sft];
        __syncthreads();
    }
    if (tid == 0) result[0] = red[0];
}

// test / tuning hook: tiles of 3 x 8 voxels in chunks of 3 planes, every call on the per-voxel kernels
static Knob g_fl_small{0}, g_fl_generic{0};

static int fl_grid(int64_t n)
{
    return capped_grid(n, kFlNT, kFlMaxGrid);
}

// image: (n_0, ...), rank 2 .. 4, float32 / float64, C-contiguous, every axis at least 2 long
static int fl_check_image(const mi_array *image, const char *name)
{
    int rc;
    if ((rc = check_array(image, name))) return rc;
    MI_REQUIRE(image->ndim >= 2 && image->ndim <= kFlMaxNd, MI_ERR_INVALID_ARG, "tvl1: images of rank 2 to 4 only");
    MI_REQUIRE(is_contiguous(image), MI_ERR_NOT_CONTIGUOUS, "tvl1 needs C-contiguous arrays");
    if (image->dtype != MI_F32 && image->dtype != MI_F64) {
        set_error("tvl1: float32 and float64 arrays only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    for (int d = 0; d < image->ndim; d++)
        MI_REQUIRE(image->shape[d] >= 2, MI_ERR_INVALID_ARG, "tvl1: every axis must have at least 2 samples (numpy.gradient's rule)");
    return MI_OK;
}

// arr: (lead..., *shape) with `nlead` leading axes of length rank, the dtype of the image described by `shape`
static int fl_check_field(const mi_array *arr, int nlead, int nd, const int64_t *shape, int dtype, const char *name)
{
    int rc;
    if ((rc = check_array(arr, name))) return rc;
    MI_REQUIRE(arr->ndim == nd + nlead && arr->dtype == dtype, MI_ERR_INVALID_ARG, "tvl1: an array has the wrong rank or dtype");
    for (int d = 0; d < nlead; d++) MI_REQUIRE(arr->shape[d] == nd, MI_ERR_INVALID_ARG, "tvl1: a component axis has the wrong length");
    for (int d = 0; d < nd; d++) MI_REQUIRE(arr->shape[nlead + d] == shape[d], MI_ERR_INVALID_ARG, "tvl1: arrays must agree in shape");
    MI_REQUIRE(is_contiguous(arr), MI_ERR_NOT_CONTIGUOUS, "tvl1 needs C-contiguous arrays");
    return MI_OK;
}

// the image a flow field (ndim, *shape) belongs to
static int fl_image_of(const mi_array *flow, mi_array *image)
{
    int rc;
    if ((rc = check_array(flow, "flow"))) return rc;
    MI_REQUIRE(flow->ndim >= 3 && flow->ndim <= kFlMaxNd + 1 && flow->shape[0] == flow->ndim - 1, MI_ERR_INVALID_ARG,
               "tvl1: flow must have shape (ndim, *image.shape), ndim 2 to 4");
    MI_REQUIRE(is_contiguous(flow), MI_ERR_NOT_CONTIGUOUS, "tvl1 needs C-contiguous arrays");
    memset(image, 0, sizeof(*image));
    image->data = flow->data;
    image->dtype = flow->dtype;
    image->ndim = flow->ndim - 1;
    int64_t st = (int64_t)dtype_size(flow->dtype);
    for (int d = image->ndim - 1; d >= 0; d--) {
        image->shape[d] = flow->shape[d + 1];
        image->strides[d] = st;
        st *= image->shape[d];
    }
    return fl_check_image(image, "flow");
}

// GO(T, ND) for the dtype and rank
#define FL_BY_RANK(dtype_, nd_, GO)                                     \
    do {                                                                \
        const bool f32__ = (dtype_) == MI_F32;                          \
        switch (nd_) {                                                  \
        case 2: if (f32__) GO(float, 2); else GO(double, 2); break;     \
        case 3: if (f32__) GO(float, 3); else GO(double, 3); break;     \
        default: if (f32__) GO(float, 4); else GO(double, 4); break;    \
        }                                                               \
    } while (0)

template <typename T, bool VOL, int TX>
static int launch_fl_fused(const mi_array *v, const mi_array *pin, const mi_array *uout, const mi_array *pout, const FlParams &p, double dt,
                           double f1, hipStream_t s)
{
    static PerDeviceOnce attr;
    if (!attr) {
        MI_HIP(hipFuncSetAttribute((const void *)tvl1_reg_fused_kernel<T, VOL, TX>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        attr = true;
    }
    constexpr int NC = VOL ? 3 : 2;
    const size_t lds = (size_t)(4 + 4 * NC + 2) * (p.ty + 4) * (TX + 4) * sizeof(T);
    const int grid = p.nxt * p.nyt * p.nzc;
    hipLaunchKernelGGL((tvl1_reg_fused_kernel<T, VOL, TX>), dim3((unsigned)grid, NC), dim3(kFlNT), lds, s, (const T *)v->data,
                       (const T *)pin->data, (T *)uout->data, (T *)pout->data, p, (T)dt, (T)f1);
    MI_HIP(hipGetLastError());
    note_kernel("mi::tvl1_reg_fused_kernel<%s,%s> grid=%dx%d tile=%dx%d chunk=%d (both regularisation steps in one tile residency, "
                "streamed along axis 0)",
                sizeof(T) == 4 ? "float32" : "float64", VOL ? "volume" : "image", grid, NC, p.ty, TX, p.zc);
    return MI_OK;
}

// MI_ERR_UNSUPPORTED (nothing queued): not a shape of the fused kernel
static int fl_fused(const mi_array *image, const mi_array *v, const mi_array *pin, const mi_array *uout, const mi_array *pout, double dt,
                    double f1, hipStream_t s)
{
    const bool vol = image->ndim == 3;
    const int64_t nz = vol ? image->shape[0] : 1, ny = image->shape[vol ? 1 : 0], nx = image->shape[vol ? 2 : 1];
    if (nz >= ((int64_t)1 << 24) || ny >= ((int64_t)1 << 24) || nx >= ((int64_t)1 << 24)) return MI_ERR_UNSUPPORTED;
    const bool f32 = image->dtype == MI_F32;
    const bool small = g_fl_small != 0;
    // 8 rows of 64 voxels (32 for float64): 18 staged planes of 12 x 68 (12 x 36) elements = 57 (61) KiB, two workgroups a CU
    const int tx = small ? 8 : (f32 ? 64 : 32);
    FlParams p;
    memset(&p, 0, sizeof(p));
    p.nx = (int)nx; p.ny = (int)ny; p.nz = (int)nz;
    p.ty = (int)std::min<int64_t>(small ? 3 : 8, ny);      // at most 8: the kernel's registers hold a plane of 12 rows
    p.nxt = (int)((nx + tx - 1) / tx);
    p.nyt = (int)((ny + p.ty - 1) / p.ty);
    const int64_t tiles = (int64_t)p.nxt * p.nyt;
    if (tiles > 65535 * 16) return MI_ERR_UNSUPPORTED;
    // chunks of planes: a chunk stages four planes beyond its own, and the workgroups run in rounds of two per CU; take the
    // number of chunks (of at least 8 planes) for which rounds x staged planes per workgroup is least, the fewest on a tie
    int64_t nzc = 1;
    if (small) {
        nzc = (nz + 2) / 3;
    } else {
        const int64_t slots = 2 * (int64_t)std::max(1, device_cus()), per_chunk = tiles * (vol ? 3 : 2);
        int64_t best = -1;
        for (int64_t c = 1; c <= std::max<int64_t>(1, nz / 8); c++) {
            const int64_t zc = (nz + c - 1) / c, real = (nz + zc - 1) / zc;
            const int64_t cost = ((per_chunk * real + slots - 1) / slots) * (zc + 4);
            if (best < 0 || cost < best) {
                best = cost;
                nzc = c;
            }
        }
    }
    p.zc = (int)((nz + nzc - 1) / nzc);
    p.nzc = (int)((nz + p.zc - 1) / p.zc);
    if (tiles * p.nzc >= ((int64_t)1 << 31)) return MI_ERR_UNSUPPORTED;
#define FL_GO(T, TXF)                                                                                      \
    (vol ? (small ? launch_fl_fused<T, true, 8>(v, pin, uout, pout, p, dt, f1, s)                          \
                  : launch_fl_fused<T, true, TXF>(v, pin, uout, pout, p, dt, f1, s))                       \
         : (small ? launch_fl_fused<T, false, 8>(v, pin, uout, pout, p, dt, f1, s)                         \
                  : launch_fl_fused<T, false, TXF>(v, pin, uout, pout, p, dt, f1, s)))
    return f32 ? FL_GO(float, 64) : FL_GO(double, 32);
#undef FL_GO
}

static bool fl_takes_fused(const mi_array *image)
{
    return !g_fl_generic && (image->ndim == 2 || image->ndim == 3);
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_tvl1(int small_tiles, int force_generic)
{
    g_fl_small = small_tiles != 0;
    g_fl_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_tvl1_coords(const mi_array *flow, const mi_array *coords, mi_stream stream)
{
    int rc;
    mi_array image;
    if ((rc = fl_image_of(flow, &image)) || (rc = fl_check_field(coords, 1, image.ndim, image.shape, image.dtype, "coords"))) return rc;
    MI_REQUIRE(coords->data != flow->data, MI_ERR_INVALID_ARG, "coords may not be the flow");
    VoxelGeom<kFlMaxNd> g;
    voxel_geom(&image, &g);
    hipStream_t s = resolve_stream(stream);
    const int grid = fl_grid(g.total);
#define FL_COORDS(T, ND) hipLaunchKernelGGL((tvl1_coords_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)flow->data, (T *)coords->data, g)
    FL_BY_RANK(image.dtype, image.ndim, FL_COORDS);
#undef FL_COORDS
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_tvl1_prepare(const mi_array *warped, const mi_array *reference, const mi_array *flow, const mi_array *grad,
                               const mi_array *ni, const mi_array *rho0, mi_stream stream)
{
    int rc;
    if ((rc = fl_check_image(warped, "warped"))) return rc;
    const int nd = warped->ndim, dt = warped->dtype;
    if ((rc = fl_check_field(reference, 0, nd, warped->shape, dt, "reference")) || (rc = fl_check_field(flow, 1, nd, warped->shape, dt, "flow")) ||
        (rc = fl_check_field(grad, 1, nd, warped->shape, dt, "grad")) || (rc = fl_check_field(ni, 0, nd, warped->shape, dt, "NI")) ||
        (rc = fl_check_field(rho0, 0, nd, warped->shape, dt, "rho_0")))
        return rc;
    MI_REQUIRE(grad->data != warped->data && grad->data != flow->data && ni->data != warped->data && rho0->data != warped->data &&
               rho0->data != reference->data, MI_ERR_INVALID_ARG, "tvl1_prepare: outputs may not be inputs");
    VoxelGeom<kFlMaxNd> g;
    voxel_geom(warped, &g);
    hipStream_t s = resolve_stream(stream);
    const int grid = fl_grid(g.total);
#define FL_PREP(T, ND)                                                                                                        \
    hipLaunchKernelGGL((tvl1_prepare_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)warped->data, (const T *)reference->data, \
                       (const T *)flow->data, (T *)grad->data, (T *)ni->data, (T *)rho0->data, g)
    FL_BY_RANK(dt, nd, FL_PREP);
#undef FL_PREP
    MI_HIP(hipGetLastError());
    note_kernel("mi::tvl1_prepare_kernel<%s> grid=%d (gradient, NI and rho_0 of one warp, rank %d)", dt == MI_F32 ? "float32" : "float64", grid, nd);
    return MI_OK;
}

extern "C" int mi_tvl1_data(const mi_array *grad, const mi_array *ni, const mi_array *rho0, const mi_array *flow, double f0, mi_stream stream)
{
    int rc;
    if ((rc = fl_check_image(ni, "NI"))) return rc;
    const int nd = ni->ndim, dt = ni->dtype;
    if ((rc = fl_check_field(rho0, 0, nd, ni->shape, dt, "rho_0")) || (rc = fl_check_field(flow, 1, nd, ni->shape, dt, "flow")) ||
        (rc = fl_check_field(grad, 1, nd, ni->shape, dt, "grad")))
        return rc;
    MI_REQUIRE(flow->data != grad->data, MI_ERR_INVALID_ARG, "tvl1_data: the flow may not be grad");
    const int64_t total = numel(ni);
    hipStream_t s = resolve_stream(stream);
    const int grid = fl_grid(total);
#define FL_DATA(T, ND)                                                                                                        \
    hipLaunchKernelGGL((tvl1_data_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)grad->data, (const T *)ni->data,      \
                       (const T *)rho0->data, (T *)flow->data, total, (T)f0)
    FL_BY_RANK(dt, nd, FL_DATA);
#undef FL_DATA
    MI_HIP(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_tvl1_scratch_size(const mi_array *flow, int64_t *elements)
{
    int rc;
    mi_array image;
    MI_REQUIRE(elements, MI_ERR_INVALID_ARG, "NULL argument");
    if ((rc = fl_image_of(flow, &image))) return rc;
    *elements = fl_takes_fused(&image) ? 0 : (int64_t)(image.ndim + 1) * image.ndim * numel(&image);
    return MI_OK;
}

extern "C" int mi_tvl1_reg(const mi_array *flow_aux, const mi_array *proj_in, const mi_array *flow_out, const mi_array *proj_out,
                           void *scratch_dev, double dt, double f1, int *launches, mi_stream stream)
{
    int rc;
    mi_array image;
    if ((rc = fl_image_of(flow_aux, &image))) return rc;
    const int nd = image.ndim;
    if ((rc = fl_check_field(flow_out, 1, nd, image.shape, image.dtype, "flow_out")) ||
        (rc = fl_check_field(proj_in, 2, nd, image.shape, image.dtype, "proj_in")) ||
        (rc = fl_check_field(proj_out, 2, nd, image.shape, image.dtype, "proj_out")))
        return rc;
    MI_REQUIRE(flow_out->data != flow_aux->data && proj_out->data != proj_in->data, MI_ERR_INVALID_ARG,
               "tvl1_reg: the output buffers may not be the input buffers");
    if (launches) *launches = 0;
    hipStream_t s = resolve_stream(stream);
    rc = MI_ERR_UNSUPPORTED;
    if (fl_takes_fused(&image)) rc = fl_fused(&image, flow_aux, proj_in, flow_out, proj_out, dt, f1, s);
    if (rc == MI_OK) {
        if (launches) *launches = 1;
        return MI_OK;
    }
    if (rc != MI_ERR_UNSUPPORTED) return rc;
    MI_REQUIRE(scratch_dev, MI_ERR_INVALID_ARG, "tvl1_reg: the per-voxel route needs the scratch block (mi_tvl1_scratch_size)");
    VoxelGeom<kFlMaxNd> g;
    voxel_geom(&image, &g);
    const int grid = fl_grid(g.total * nd);
#define FL_GEN(T, ND)                                                                                                         \
    do {                                                                                                                      \
        T *p1 = (T *)scratch_dev, *u1 = p1 + (int64_t)ND * ND * g.total;                                                      \
        hipLaunchKernelGGL((tvl1_step_p_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)flow_aux->data,               \
                           (const T *)proj_in->data, p1, g, (T)dt, (T)f1);                                                    \
        hipLaunchKernelGGL((tvl1_step_u_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)flow_aux->data, (const T *)p1, u1, g); \
        hipLaunchKernelGGL((tvl1_step_p_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)u1, (const T *)p1,            \
                           (T *)proj_out->data, g, (T)dt, (T)f1);                                                             \
        hipLaunchKernelGGL((tvl1_step_u_kernel<T, ND>), dim3(grid), dim3(kFlNT), 0, s, (const T *)flow_aux->data,               \
                           (const T *)proj_out->data, (T *)flow_out->data, g);                                                \
    } while (0)
    FL_BY_RANK(image.dtype, nd, FL_GEN);
#undef FL_GEN
    MI_HIP(hipGetLastError());
    if (launches) *launches = 4;
    note_kernel("mi::tvl1_step_kernels<%s> grid=%d (both regularisation steps as four launches, one thread per voxel, rank %d)",
                image.dtype == MI_F32 ? "float32" : "float64", grid, nd);
    return MI_OK;
}

extern "C" int mi_tvl1_diff_sum(const mi_array *a, const mi_array *b, void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = check_array(a, "a")) || (rc = check_array(b, "b"))) return rc;
    MI_REQUIRE(work_dev, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(same_shape(a, b) && a->dtype == b->dtype && (a->dtype == MI_F32 || a->dtype == MI_F64), MI_ERR_INVALID_ARG,
               "tvl1_diff_sum: two float32 / float64 arrays of one shape");
    MI_REQUIRE(is_contiguous(a) && is_contiguous(b), MI_ERR_NOT_CONTIGUOUS, "tvl1 needs C-contiguous arrays");
    const int64_t n = numel(a);
    hipStream_t s = resolve_stream(stream);
    double *result = (double *)work_dev, *part = result + 8;
    const int grid = capped_grid(n, kFlNT, kFlDiffGrid);
    if (a->dtype == MI_F32)
        hipLaunchKernelGGL((tvl1_diff_kernel<float>), dim3(grid), dim3(kFlNT), 0, s, (const float *)a->data, (const float *)b->data, n, part);
    else
        hipLaunchKernelGGL((tvl1_diff_kernel<double>), dim3(grid), dim3(kFlNT), 0, s, (const double *)a->data, (const double *)b->data, n, part);
    hipLaunchKernelGGL(tvl1_diff_final_kernel, dim3(1), dim3(kFlNT), 0, s, (const double *)part, grid, result);
    MI_HIP(hipGetLastError());
    return MI_OK;
}
