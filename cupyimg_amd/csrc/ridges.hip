// ridges.hip -- the Hessian family (skimage.feature.hessian_matrix / hessian_matrix_eigvals, skimage.filters.frangi / sato /
// meijering / hessian): everything that follows the Gaussian of one scale in one launch.
//
// Reference path replaced: cupyimg/skimage/feature/corner.py:141-211, 260-309 and cupyimg/skimage/filters/ridges.py:112-635,
// which per scale take gradient of gradient (3 + 6 volume passes, 6 Hessian volumes in 3-D), scatter them into an
// (..., 3, 3) array for a batched eigvalsh, sort by fancy indexing and then run 15 to 20 element-wise operations into an
// (n_sigmas, ...) float64 stack; meijering copies the eigenvalues to the host and back.
//
// Arithmetic, all in the dtype T of the smoothed array G, this file compiled with -ffp-contract=off:
//
//   D_a f (q)  = f(q + e_a) - f(q)            q_a == 0              numpy.gradient, unit spacing, edge_order 1
//              = f(q) - f(q - e_a)            q_a == n_a - 1
//              = (f(q + e_a) - f(q - e_a)) / 2  otherwise
//   H(a0, a1)  = D_a1 (D_a0 G)                the end rules compose over the outermost two samples of an axis
//   elements   = H(a0, a1) for (a0, a1) in combinations_with_replacement(axes, 2), axes = ndim-1 .. 0 for order "rc" and
//                0 .. ndim-1 for "xy" (corner.py:201-209), so "rc" differentiates along the LAST axis first
//   matrix     = M[row][col] = M[col][row] = elements[idx], (row, col) the idx-th of combinations_with_replacement(0 .. ndim-1, 2)
//                (corner.py:328-335)
//   eigenvalues: 1 x 1 the element; 2 x 2 the closed form of corner.py:260-281 operation by operation; larger: cyclic Jacobi
//                (Rutishauser's form: the diagonal is rebuilt each sweep from its value at the start of the sweep plus the
//                accumulated corrections), at most 6 (float32) / 8 (float64) sweeps (two more above 4 x 4), stopping when
//                every off-diagonal element is exactly 0; then sorted decreasing
//   ordering   : none = decreasing; val = increasing; abs = stable sort of the decreasing list by |.| (ridges.py:53-81)
//   responses  : ridges.py:251-288 (meijering), 368-380 (sato), 497-530 (frangi), operation by operation
//
// ridge_tile_kernel (2-D and 3-D): a workgroup stages a tile of G with a two-sample halo in LDS and forms every element
// from it; as mi_hessian_matrix it writes them, as the fused step of mi_ridge_scale it goes on in registers to the response
// and updates `out` in place, so G is read once and the Hessian, the eigenvalues and a per-scale stack never exist in memory.
// hessian_generic_kernel + eig_generic_kernel: the same arithmetic with one thread per voxel and the elements in memory,
// any rank; the route of mi_debug_set_ridges(.., .., 1).
#include "skimage_common.hpp"
#include <limits>

namespace mi {

constexpr int kRgNT = 256;

template <typename T>
__device__ __forceinline__ T rg_exp(T v)
{
    if constexpr (std::is_same<T, float>::value) return ::expf(v);
    else return ::exp(v);
}
template <typename T>
__device__ __forceinline__ T rg_abs(T v)
{
    if constexpr (std::is_same<T, float>::value) return __builtin_fabsf(v);
    else return __builtin_fabs(v);
}

// ------------------------------------------------------------------ gradient of gradient
// f(j): the sample at position j of the axis, asked only for 0 <= j < n and |j - i| <= 1
template <typename T, typename I, typename F>
__device__ __forceinline__ T rg_grad1(F f, I i, I n)
{
    if (i == 0) return f((I)1) - f((I)0);
    if (i == n - 1) return f(n - 1) - f(n - 2);
    return (f(i + 1) - f(i - 1)) / T(2);
}

// H(a0, a1) at coordinates c: g(q) is G at coordinates q; touches G within two samples of c along a0 == a1, within one
// sample along each of a0 != a1, never outside the array
template <typename T, int ND, typename I, typename G>
__device__ __forceinline__ T rg_hess(G g, const I *c, const I *n, int a0, int a1)
{
    return rg_grad1<T, I>([&](I j) {
        I p[ND];
#pragma unroll
        for (int d = 0; d < ND; d++) p[d] = c[d];
        p[a1] = j;
        return rg_grad1<T, I>([&](I k) {
            I q[ND];
#pragma unroll
            for (int d = 0; d < ND; d++) q[d] = p[d];
            q[a0] = k;
            return g(q);
        }, p[a0], n[a0]);
    }, c[a1], n[a1]);
}

// ------------------------------------------------------------------ eigenvalues
// e: the upper triangle row by row; lam: decreasing
template <typename T, int N>
__device__ __forceinline__ void rg_eigvals(const T *e, T *lam)
{
    if constexpr (N == 1) {
        lam[0] = e[0];
    } else if constexpr (N == 2) {
        const T m00 = e[0], m01 = e[1], m11 = e[2];
        T tmp1 = m01 * m01;
        tmp1 = tmp1 * T(4);
        T tmp2 = m00 - m11;
        tmp2 = tmp2 * tmp2;
        tmp2 = tmp2 + tmp1;
        tmp2 = sqrt_t<T>(tmp2);
        tmp2 = tmp2 / T(2);
        tmp1 = m00 + m11;
        tmp1 = tmp1 / T(2);
        lam[0] = tmp1 + tmp2;
        lam[1] = tmp1 - tmp2;
    } else {
        T a[N][N];                                     // the upper triangle is kept
        {
            int idx = 0;
#pragma unroll
            for (int r = 0; r < N; r++)
#pragma unroll
                for (int c = r; c < N; c++) a[r][c] = e[idx++];
        }
        T d[N], b[N], z[N];
#pragma unroll
        for (int i = 0; i < N; i++) d[i] = b[i] = a[i][i];
        const int sweeps = (sizeof(T) == 4 ? 6 : 8) + (N > 4 ? 2 : 0);
#pragma unroll 1
        for (int sw = 0; sw < sweeps; sw++) {
            T off = T(0);
#pragma unroll
            for (int p = 0; p < N - 1; p++)
#pragma unroll
                for (int q = p + 1; q < N; q++) off += rg_abs<T>(a[p][q]);
            if (off == T(0)) break;
#pragma unroll
            for (int i = 0; i < N; i++) z[i] = T(0);
#pragma unroll
            for (int p = 0; p < N - 1; p++) {
#pragma unroll
                for (int q = p + 1; q < N; q++) {
                    const T apq = a[p][q];
                    if (apq != T(0)) {
                        const T h = d[q] - d[p];
                        const T theta = (T(0.5) * h) / apq;
                        const T th2 = theta * theta;
                        T t;
                        if (th2 <= std::numeric_limits<T>::max()) {
                            t = T(1) / (rg_abs<T>(theta) + sqrt_t<T>(th2 + T(1)));
                            if (theta < T(0)) t = -t;
                        } else {
                            t = apq / h;                  // theta squared overflows (or is NaN): the small-angle limit
                        }
                        const T c = T(1) / sqrt_t<T>(t * t + T(1));
                        const T s = t * c;
                        const T tau = s / (T(1) + c);
                        const T hh = t * apq;
                        z[p] -= hh; z[q] += hh;
                        d[p] -= hh; d[q] += hh;
                        a[p][q] = T(0);
#pragma unroll
                        for (int r = 0; r < N; r++) {
                            if (r == p || r == q) continue;
                            T &arp = r < p ? a[r][p] : a[p][r];
                            T &arq = r < q ? a[r][q] : a[q][r];
                            const T g = arp, k = arq;
                            arp = g - s * (k + g * tau);
                            arq = k + s * (g - k * tau);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < N; i++) {
                b[i] += z[i];
                d[i] = b[i];
            }
        }
        // decreasing
#pragma unroll
        for (int pass = 0; pass < N - 1; pass++)
#pragma unroll
            for (int j = 0; j < N - 1 - pass; j++)
                if (d[j] < d[j + 1]) { const T t = d[j]; d[j] = d[j + 1]; d[j + 1] = t; }
#pragma unroll
        for (int i = 0; i < N; i++) lam[i] = d[i];
    }
}

// lam: decreasing on entry
template <typename T, int N>
__device__ __forceinline__ void rg_order(T *lam, int sorting)
{
    if (sorting == MI_RIDGE_SORT_VAL) {
#pragma unroll
        for (int i = 0; i < N / 2; i++) { const T t = lam[i]; lam[i] = lam[N - 1 - i]; lam[N - 1 - i] = t; }
    } else if (sorting == MI_RIDGE_SORT_ABS) {
        // adjacent swaps on a strict comparison: a stable sort, ties keep the order of the decreasing list
#pragma unroll
        for (int pass = 0; pass < N - 1; pass++)
#pragma unroll
            for (int j = 0; j < N - 1 - pass; j++)
                if (rg_abs<T>(lam[j]) > rg_abs<T>(lam[j + 1])) { const T t = lam[j]; lam[j] = lam[j + 1]; lam[j + 1] = t; }
    }
}

template <typename T>
__device__ __forceinline__ T rg_nonzero(T v) { return v == T(0) ? T(1e-10) : v; }      // ridges.py:21-50

// frangi: lam ordered by |.|; a2, b2, g2 = 2 alpha^2, 2 beta^2, 2 gamma^2
template <typename T, int N>
__device__ __forceinline__ T rg_frangi(const T *lam, T a2, T b2, T g2)
{
    static_assert(N == 2 || N == 3, "frangi is defined for 2-D and 3-D");
    if constexpr (N == 2) {
        const T l1 = lam[0], l2 = lam[1];
        const T raw = rg_abs<T>(l2);
        const T q = l1 / rg_nonzero<T>(raw);
        const T rb = q * q;
        const T rg = l1 * l1 + l2 * l2;
        // r_a = inf: 1 - exp(-inf) = 1
        const T v = (T(1) * rg_exp<T>(-rb / b2)) * (T(1) - rg_exp<T>(-rg / g2));
        return l2 > T(0) ? T(0) : v;
    } else {
        const T l1 = lam[0], l2 = lam[1], l3 = lam[2];
        const T qa = l2 / rg_nonzero<T>(l3);
        const T ra = qa * qa;
        const T raw = sqrt_t<T>(rg_abs<T>(l2 * l3));
        const T qb = l1 / rg_nonzero<T>(raw);
        const T rb = qb * qb;
        const T rg = (l1 * l1 + l2 * l2) + l3 * l3;
        const T v = ((T(1) - rg_exp<T>(-ra / a2)) * rg_exp<T>(-rb / b2)) * (T(1) - rg_exp<T>(-rg / g2));
        return (l2 > l3 ? l2 : l3) > T(0) ? T(0) : v;
    }
}

// sato: lam increasing
template <typename T, int N>
__device__ __forceinline__ T rg_sato(const T *lam)
{
    static_assert(N == 2 || N == 3, "sato is defined for 2-D and 3-D");
    if constexpr (N == 2) return lam[1] > T(0) ? rg_abs<T>(lam[1]) : T(0);
    else return lam[2] > T(0) ? sqrt_t<T>(rg_abs<T>(lam[1] * lam[2])) : T(0);
}

// meijering: lam ordered by |.|.  ridges.py:262-278 as written: element i of `auxiliary` is the sum over j of
// eigenvalues[i] * roll(coefficients, j)[i], coefficients = [1, alpha, alpha, ...], and the last element is kept, so
// aux = ((l alpha + l alpha) + ...) + l * 1 with l the eigenvalue of largest magnitude.
template <typename T, int N>
__device__ __forceinline__ T rg_meijering_aux(const T *lam, T alpha)
{
    const T l = lam[N - 1];
    if constexpr (N == 1) return l;
    T s = l * alpha;
#pragma unroll
    for (int j = 1; j < N - 1; j++) s = s + l * alpha;
    return s + l;
}

// order-preserving key of a double: the smaller the value, the smaller the key
__device__ __forceinline__ unsigned long long rg_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double rg_unkey(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// minimum of a workgroup's keys into *slot (one atomic a workgroup)
__device__ __forceinline__ void rg_block_min(unsigned long long key, unsigned long long *slot)
{
    __shared__ unsigned long long red[kRgNT];
    const int tid = threadIdx.x;
    red[tid] = key;
    __syncthreads();
    for (int sft = kRgNT / 2; sft > 0; sft >>= 1) {
        if (tid < sft) red[tid] = red[tid] < red[tid + sft] ? red[tid] : red[tid + sft];
        __syncthreads();
    }
    if (tid == 0) atomicMin(slot, red[0]);
}

struct RgOut {
    void *out;                       // eigenvalues: T (N, total); aux (meijering): T (total); else double (total)
    unsigned long long *slot;        // meijering: the key of the minimum of aux
    int kind, sorting;
    double scale, p0, p1, p2;
};

// from the scaled elements of one voxel to what the launch writes for it; returns the key to reduce (meijering)
template <typename T, int N>
__device__ __forceinline__ unsigned long long rg_finish(const T *e, const RgOut &o, int64_t q, int64_t total)
{
    T lam[N];
    rg_eigvals<T, N>(e, lam);
    unsigned long long key = ~0ull;
    if (o.kind == MI_RIDGE_EIGENVALUES) {
        rg_order<T, N>(lam, o.sorting);
#pragma unroll
        for (int i = 0; i < N; i++) ((T *)o.out)[i * total + q] = lam[i];
    } else if (o.kind == MI_RIDGE_MEIJERING) {
        rg_order<T, N>(lam, MI_RIDGE_SORT_ABS);
        const T aux = rg_meijering_aux<T, N>(lam, (T)o.p0);
        ((T *)o.out)[q] = aux;
        key = rg_key((double)aux);
    } else if constexpr (N == 2 || N == 3) {
        T v;
        if (o.kind == MI_RIDGE_FRANGI) {
            rg_order<T, N>(lam, MI_RIDGE_SORT_ABS);
            v = rg_frangi<T, N>(lam, (T)o.p0, (T)o.p1, (T)o.p2);
        } else {
            rg_order<T, N>(lam, MI_RIDGE_SORT_VAL);
            v = rg_sato<T, N>(lam);
        }
        double *out = (double *)o.out;
        const double r = (double)v, was = out[q];
        out[q] = r > was ? r : was;
    }
    return key;
}

// ------------------------------------------------------------------ tile kernels (2-D and 3-D)
// g: the tiles (BoxDims, nz = 1 for images), their columns g.t[2] a power of two, at most 64
// WHAT: 0 = write the elements (XY: order "xy", else "rc"), 1 = go on to eigenvalues and response
template <typename T, int ND, int WHAT, bool XY>
__global__ void __launch_bounds__(kRgNT)
ridge_tile_kernel(const T *__restrict__ G, T *__restrict__ elems, const BoxDims g, const RgOut o)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
    T *S = reinterpret_cast<T *>(rg_lds);
    constexpr int NE = ND * (ND + 1) / 2;
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int xt = b % g.nt[2];
    b /= g.nt[2];
    const int yt = b % g.nt[1], zt = b / g.nt[1];
    const int x0 = xt * g.t[2], y0 = yt * g.t[1], z0 = zt * g.t[0];
    const int LX = g.t[2] + 4, LY = g.t[1] + 4, LZ = ND == 3 ? g.t[0] + 4 : 1;
    const int zb = ND == 3 ? z0 - 2 : 0, yb = y0 - 2, xb = x0 - 2;
    const int64_t plane = (int64_t)g.n[1] * g.n[2];
    const int64_t total = plane * g.n[0];

    // stage the tile and its halo: staged position (lz, ly, lx) <-> voxel (zb + lz, yb + ly, xb + lx), inside the array only
    for (int row = tid >> 6; row < LZ * LY; row += kRgNT / 64) {
        const int lz = row / LY, ly = row - lz * LY;
        const int z = zb + lz, y = yb + ly;
        if (z < 0 || z >= g.n[0] || y < 0 || y >= g.n[1]) continue;
        const T *src = G + (int64_t)z * plane + (int64_t)y * g.n[2];
        for (int lx = tid & 63; lx < LX; lx += 64) {
            const int x = xb + lx;
            if (x >= 0 && x < g.n[2]) S[row * LX + lx] = src[x];
        }
    }
    __syncthreads();

    unsigned long long key = ~0ull;
    const int txs = g.t[2];                                  // threads along x
    const int lx = tid & (txs - 1);
    const int rows_per_pass = kRgNT / txs;
    const int x = x0 + lx;
    for (int row = tid / txs; row < g.t[0] * g.t[1]; row += rows_per_pass) {
        const int tz = row / g.t[1], ty = row - tz * g.t[1];
        const int z = z0 + tz, y = y0 + ty;
        if (x >= g.n[2] || y >= g.n[1] || z >= g.n[0]) continue;
        int c[ND], n[ND];
        if constexpr (ND == 3) {
            c[0] = z; c[1] = y; c[2] = x;
            n[0] = g.n[0]; n[1] = g.n[1]; n[2] = g.n[2];
        } else {
            c[0] = y; c[1] = x;
            n[0] = g.n[1]; n[1] = g.n[2];
        }
        auto at = [&](const int *q) -> T {
            if constexpr (ND == 3) return S[((q[0] - zb) * LY + (q[1] - yb)) * LX + (q[2] - xb)];
            else return S[(q[0] - yb) * LX + (q[1] - xb)];
        };
        T e[NE];
        {
            int idx = 0;
#pragma unroll
            for (int i = 0; i < ND; i++)
#pragma unroll
                for (int j = i; j < ND; j++) {
                    const int a0 = XY ? i : ND - 1 - i, a1 = XY ? j : ND - 1 - j;
                    e[idx++] = rg_hess<T, ND, int>(at, c, n, a0, a1);
                }
        }
        const int64_t q = (int64_t)z * plane + (int64_t)y * g.n[2] + x;
        if constexpr (WHAT == 0) {
#pragma unroll
            for (int i = 0; i < NE; i++) elems[i * total + q] = e[i];
        } else {
            const T s2 = (T)o.scale;
#pragma unroll
            for (int i = 0; i < NE; i++) e[i] = s2 * e[i];
            const unsigned long long k = rg_finish<T, ND>(e, o, q, total);
            key = k < key ? k : key;
        }
    }
    if constexpr (WHAT == 1) {
        if (o.kind == MI_RIDGE_MEIJERING) rg_block_min(key, o.slot);
    }
}

// ------------------------------------------------------------------ per-voxel kernels (any rank)
template <typename T>
__global__ void __launch_bounds__(kRgNT)
hessian_generic_kernel(const T *__restrict__ G, T *__restrict__ elems, const VoxelGeom<MI_MAX_NDIM> g, int xy)
{
    for (int64_t i = (int64_t)blockIdx.x * kRgNT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * kRgNT) {
        int64_t c[MI_MAX_NDIM], n[MI_MAX_NDIM];
        int64_t r = i;
        for (int a = MI_MAX_NDIM - 1; a >= 0; a--) {         // voxel_coords and the lengths in one rolled loop
            c[a] = 0; n[a] = 1;
            if (a < g.nd) {
                const int64_t qq = r / g.shape[a];
                c[a] = r - qq * g.shape[a];
                n[a] = g.shape[a];
                r = qq;
            }
        }
        auto at = [&](const int64_t *q) -> T {
            int64_t off = 0;
            for (int a = 0; a < g.nd; a++) off += q[a] * g.stride[a];
            return G[off];
        };
        int idx = 0;
        for (int a = 0; a < g.nd; a++)
            for (int bb = a; bb < g.nd; bb++) {
                const int a0 = xy ? a : g.nd - 1 - a, a1 = xy ? bb : g.nd - 1 - bb;
                elems[idx * g.total + i] = rg_hess<T, MI_MAX_NDIM, int64_t>(at, c, n, a0, a1);
                idx++;
            }
    }
}

template <typename T, int N>
__global__ void __launch_bounds__(kRgNT)
eig_generic_kernel(const T *__restrict__ elems, int64_t total, const RgOut o)
{
    constexpr int NE = N * (N + 1) / 2;
    unsigned long long key = ~0ull;
    const T s2 = (T)o.scale;
    for (int64_t i = (int64_t)blockIdx.x * kRgNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRgNT) {
        T e[NE];
#pragma unroll
        for (int k = 0; k < NE; k++) e[k] = s2 * elems[k * total + i];
        const unsigned long long k = rg_finish<T, N>(e, o, i, total);
        key = k < key ? k : key;
    }
    if (o.kind == MI_RIDGE_MEIJERING) rg_block_min(key, o.slot);
}

// meijering, second launch: out = max(out, aux < 0 ? aux / min(aux) : 0), a zero minimum replaced by 1e-10
template <typename T>
__global__ void __launch_bounds__(kRgNT)
meijering_norm_kernel(const T *__restrict__ aux, double *__restrict__ out, int64_t total, const unsigned long long *__restrict__ slot)
{
    const T m = rg_nonzero<T>((T)rg_unkey(*slot));
    for (int64_t i = (int64_t)blockIdx.x * kRgNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRgNT) {
        const T a = aux[i];
        const double r = a < T(0) ? (double)(a / m) : 0.0, was = out[i];
        out[i] = r > was ? r : was;
    }
}

// hessian filter, last step: every value <= 0 becomes `value` (ridges.py:634)
__global__ void __launch_bounds__(kRgNT)
fill_nonpositive_kernel(double *__restrict__ a, int64_t total, double value)
{
    for (int64_t i = (int64_t)blockIdx.x * kRgNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRgNT)
        if (a[i] <= 0.0) a[i] = value;
}

// test / tuning hook: tile rows, tile planes (0 = the planner's), every call on the per-voxel kernels
static Knob g_rg_ty{0}, g_rg_tz{0}, g_rg_generic{0};

static int rg_grid(int64_t total)
{
    return capped_grid(total, kRgNT, 8192);
}

// the tile plan of a 2-D / 3-D array; false: not a shape of the tile kernels
static bool rg_plan(const mi_array *a, BoxDims *p, size_t *lds)
{
    if (a->ndim != 2 && a->ndim != 3) return false;
    const bool vol = a->ndim == 3;
    const int64_t nz = vol ? a->shape[0] : 1, ny = a->shape[vol ? 1 : 0], nx = a->shape[vol ? 2 : 1];
    if (nz >= ((int64_t)1 << 24) || ny >= ((int64_t)1 << 24) || nx >= ((int64_t)1 << 24)) return false;
    const int es = (int)dtype_size(a->dtype);
    const bool forced = g_rg_ty != 0 || g_rg_tz != 0;
    // 8 planes x 8 rows x 64 columns (float64: 4 planes): 12 x 12 x 68 staged samples = 38 KiB (51 KiB), four (three)
    // workgroups a CU, 2.4 (2.9) staged samples a voxel, most of them from L2; images: 16 rows x 64 columns.
    // Forced tiles are 16 columns wide, so that small test arrays have seams along every axis.
    p->t[2] = forced ? 16 : 64;
    p->t[1] = vol ? 8 : 16;
    p->t[0] = vol ? (es == 8 ? 4 : 8) : 1;
    if (g_rg_ty) p->t[1] = std::min((int)g_rg_ty, p->t[1]);
    if (g_rg_tz && vol) p->t[0] = std::min((int)g_rg_tz, p->t[0]);
    p->n[0] = (int)nz; p->n[1] = (int)ny; p->n[2] = (int)nx;
    int64_t blocks = 1;
    for (int d = 0; d < 3; d++) {
        p->nt[d] = (p->n[d] + p->t[d] - 1) / p->t[d];
        blocks *= p->nt[d];
    }
    if (blocks > 0x7fffffff) return false;
    *lds = (size_t)(vol ? p->t[0] + 4 : 1) * (p->t[1] + 4) * (p->t[2] + 4) * es;
    return true;
}

template <typename T, int ND, int WHAT, bool XY>
static int launch_rg_tile(const mi_array *G, void *elems, const BoxDims &p, size_t lds, const RgOut &o, hipStream_t s)
{
    const int grid = p.nt[0] * p.nt[1] * p.nt[2];
    hipLaunchKernelGGL((ridge_tile_kernel<T, ND, WHAT, XY>), dim3((unsigned)grid), dim3(kRgNT), lds, s, (const T *)G->data, (T *)elems, p, o);
    MI_HIP(hipGetLastError());
    note_kernel("mi::ridge_tile_kernel<%s,%d,%s> grid=%d tile=%dx%dx%d (%s)", sizeof(T) == 4 ? "float32" : "float64", ND,
                WHAT == 0 ? (XY ? "hessian-xy" : "hessian-rc") : "fused", grid, p.t[0], p.t[1], p.t[2],
                WHAT == 0 ? "all Hessian elements from one staged tile of the smoothed array"
                          : "Hessian, eigenvalues and response in registers from one staged tile");
    return MI_OK;
}

static int rg_check_g(const mi_array *G, const char *who)
{
    int rc;
    if ((rc = check_array(G, "g"))) return rc;
    MI_REQUIRE(G->ndim >= 1, MI_ERR_INVALID_ARG, "the smoothed array must have at least one dimension");
    MI_REQUIRE(is_contiguous(G), MI_ERR_NOT_CONTIGUOUS, "the ridge kernels need C-contiguous arrays");
    if (G->dtype != MI_F32 && G->dtype != MI_F64) {
        set_error("%s: float32 and float64 arrays only (the caller converts)", who);
        return MI_ERR_UNSUPPORTED;
    }
    for (int d = 0; d < G->ndim; d++)
        MI_REQUIRE(G->shape[d] >= 2, MI_ERR_INVALID_ARG, "the gradient needs at least 2 samples along every axis");
    return MI_OK;
}

// a C-contiguous (rows, total) array of dtype dt
static int rg_check_2d(const mi_array *a, int64_t rows, int64_t total, int dt, const char *msg)
{
    int rc;
    if ((rc = check_array(a, "out"))) return rc;
    MI_REQUIRE(a->ndim == 2 && a->shape[0] == rows && a->shape[1] == total && a->dtype == dt, MI_ERR_INVALID_ARG, msg);
    MI_REQUIRE(is_contiguous(a), MI_ERR_NOT_CONTIGUOUS, "the ridge kernels need C-contiguous arrays");
    return MI_OK;
}

static int hessian_elements(const mi_array *G, void *elems, int xy, bool allow_tile, hipStream_t s)
{
    BoxDims p;
    size_t lds = 0;
    const bool f32 = G->dtype == MI_F32;
    if (allow_tile && rg_plan(G, &p, &lds)) {
#define RG_H(T)                                                                                                      \
    (G->ndim == 3 ? (xy ? launch_rg_tile<T, 3, 0, true>(G, elems, p, lds, RgOut{}, s)                                 \
                        : launch_rg_tile<T, 3, 0, false>(G, elems, p, lds, RgOut{}, s))                                \
                  : (xy ? launch_rg_tile<T, 2, 0, true>(G, elems, p, lds, RgOut{}, s)                                 \
                        : launch_rg_tile<T, 2, 0, false>(G, elems, p, lds, RgOut{}, s)))
        return f32 ? RG_H(float) : RG_H(double);
#undef RG_H
    }
    VoxelGeom<MI_MAX_NDIM> g;
    voxel_geom(G, &g);
    const int grid = rg_grid(g.total);
    if (f32) hipLaunchKernelGGL(hessian_generic_kernel<float>, dim3(grid), dim3(kRgNT), 0, s, (const float *)G->data, (float *)elems, g, xy);
    else hipLaunchKernelGGL(hessian_generic_kernel<double>, dim3(grid), dim3(kRgNT), 0, s, (const double *)G->data, (double *)elems, g, xy);
    MI_HIP(hipGetLastError());
    note_kernel("mi::hessian_generic_kernel<%s> grid=%d (gradient of gradient, one thread per voxel, rank %d)",
                f32 ? "float32" : "float64", grid, G->ndim);
    return MI_OK;
}

static int eig_generic(const void *elems, int dtype, int n, int64_t total, const RgOut &o, hipStream_t s)
{
    const int grid = rg_grid(total);
#define RG_E(T, N) hipLaunchKernelGGL((eig_generic_kernel<T, N>), dim3(grid), dim3(kRgNT), 0, s, (const T *)elems, total, o)
#define RG_EN(N) do { if (dtype == MI_F32) RG_E(float, N); else RG_E(double, N); } while (0)
    switch (n) {
    case 1: RG_EN(1); break;
    case 2: RG_EN(2); break;
    case 3: RG_EN(3); break;
    case 4: RG_EN(4); break;
    case 5: RG_EN(5); break;
    case 6: RG_EN(6); break;
    case 7: RG_EN(7); break;
    default: RG_EN(8); break;
    }
#undef RG_EN
#undef RG_E
    MI_HIP(hipGetLastError());
    note_kernel("mi::eig_generic_kernel<%s,%d> grid=%d (eigenvalues and response of stored elements, one thread per voxel)",
                dtype == MI_F32 ? "float32" : "float64", n, grid);
    return MI_OK;
}

}  // namespace mi

using namespace mi;
static_assert(MI_MAX_NDIM == 8, "eig_generic dispatches the ranks 1 .. 8");

extern "C" int mi_debug_set_ridges(int tile_rows, int tile_planes, int force_generic)
{
    g_rg_ty = tile_rows < 0 ? 0 : tile_rows;
    g_rg_tz = tile_planes < 0 ? 0 : tile_planes;
    g_rg_generic = force_generic != 0;
    return MI_OK;
}

extern "C" int mi_hessian_matrix(const mi_array *g, const mi_array *out, int order_xy, mi_stream stream)
{
    int rc;
    if ((rc = rg_check_g(g, "hessian_matrix"))) return rc;
    const int64_t total = numel(g);
    const int ne = g->ndim * (g->ndim + 1) / 2;
    if ((rc = rg_check_2d(out, ne, total, g->dtype, "out must be (ndim (ndim + 1) / 2, g.size) of g's dtype"))) return rc;
    MI_REQUIRE(out->data != g->data, MI_ERR_INVALID_ARG, "out may not be g");
    return hessian_elements(g, out->data, order_xy != 0, !g_rg_generic, resolve_stream(stream));
}

extern "C" int mi_symmetric_eigvals(const mi_array *elems, const mi_array *out, int ndim, mi_stream stream)
{
    int rc;
    if ((rc = check_array(elems, "elems"))) return rc;
    MI_REQUIRE(ndim >= 1 && ndim <= MI_MAX_NDIM, MI_ERR_INVALID_ARG, "matrices of 1 x 1 to MI_MAX_NDIM x MI_MAX_NDIM");
    MI_REQUIRE(elems->ndim == 2 && elems->shape[0] == ndim * (ndim + 1) / 2, MI_ERR_INVALID_ARG,
               "elems must be (ndim (ndim + 1) / 2, size)");
    MI_REQUIRE(is_contiguous(elems), MI_ERR_NOT_CONTIGUOUS, "the ridge kernels need C-contiguous arrays");
    if (elems->dtype != MI_F32 && elems->dtype != MI_F64) {
        set_error("symmetric_eigvals: float32 and float64 arrays only (the caller converts)");
        return MI_ERR_UNSUPPORTED;
    }
    const int64_t total = elems->shape[1];
    if ((rc = rg_check_2d(out, ndim, total, elems->dtype, "out must be (ndim, size) of the elements' dtype"))) return rc;
    MI_REQUIRE(out->data != elems->data, MI_ERR_INVALID_ARG, "out may not be elems");
    if (total == 0) return MI_OK;
    RgOut o;
    memset(&o, 0, sizeof(o));
    o.out = out->data;
    o.kind = MI_RIDGE_EIGENVALUES;
    o.sorting = MI_RIDGE_SORT_NONE;
    o.scale = 1.0;
    return eig_generic(elems->data, elems->dtype, ndim, total, o, resolve_stream(stream));
}

extern "C" int mi_ridge_scale(const mi_array *g, const mi_array *out, int kind, int sorting, double sigma, double p0, double p1,
                              double p2, const mi_array *scratch, void *work_dev, mi_stream stream)
{
    int rc;
    if ((rc = rg_check_g(g, "ridge_scale"))) return rc;
    MI_REQUIRE(kind >= MI_RIDGE_EIGENVALUES && kind <= MI_RIDGE_MEIJERING, MI_ERR_INVALID_ARG, "unknown kind");
    MI_REQUIRE(sorting >= MI_RIDGE_SORT_NONE && sorting <= MI_RIDGE_SORT_ABS, MI_ERR_INVALID_ARG, "unknown sorting");
    const int nd = g->ndim;
    const int64_t total = numel(g);
    if ((kind == MI_RIDGE_FRANGI || kind == MI_RIDGE_SATO) && nd != 2 && nd != 3) {
        set_error("ridge_scale: frangi and sato are defined for 2-D and 3-D arrays");
        return MI_ERR_INVALID_ARG;
    }
    if (kind == MI_RIDGE_EIGENVALUES) {
        if ((rc = rg_check_2d(out, nd, total, g->dtype, "out must be (ndim, g.size) of g's dtype"))) return rc;
    } else {
        if ((rc = check_array(out, "out"))) return rc;
        MI_REQUIRE(same_shape(g, out) && out->dtype == MI_F64, MI_ERR_INVALID_ARG, "out must be float64 of g's shape");
        MI_REQUIRE(is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "the ridge kernels need C-contiguous arrays");
    }
    MI_REQUIRE(out->data != g->data, MI_ERR_INVALID_ARG, "out may not be g");
    RgOut o;
    memset(&o, 0, sizeof(o));
    o.out = out->data;
    o.kind = kind;
    o.sorting = sorting;
    o.scale = sigma * sigma;
    o.p0 = p0; o.p1 = p1; o.p2 = p2;
    if (kind == MI_RIDGE_MEIJERING) {
        MI_REQUIRE(scratch && work_dev, MI_ERR_INVALID_ARG, "meijering needs the scratch volume and the work block");
        if ((rc = check_array(scratch, "scratch"))) return rc;
        MI_REQUIRE(same_shape(g, scratch) && scratch->dtype == g->dtype && is_contiguous(scratch), MI_ERR_INVALID_ARG,
                   "scratch must be a C-contiguous array of g's shape and dtype");
        MI_REQUIRE(scratch->data != g->data && scratch->data != out->data, MI_ERR_INVALID_ARG, "scratch may not be g or out");
        o.out = scratch->data;
        o.slot = (unsigned long long *)work_dev;
    }
    hipStream_t s = resolve_stream(stream);
    BoxDims p;
    size_t lds = 0;
    const bool f32 = g->dtype == MI_F32;
    if (!g_rg_generic && rg_plan(g, &p, &lds)) {
#define RG_F(T) (nd == 3 ? launch_rg_tile<T, 3, 1, false>(g, nullptr, p, lds, o, s) : launch_rg_tile<T, 2, 1, false>(g, nullptr, p, lds, o, s))
        rc = f32 ? RG_F(float) : RG_F(double);
#undef RG_F
        if (rc) return rc;
    } else {
        // the unfused route: the elements in memory (the pool's, returned in stream order), then one thread per voxel
        void *elems = nullptr;
        const size_t bytes = (size_t)(nd * (nd + 1) / 2) * (size_t)total * dtype_size(g->dtype);
        if ((rc = pool_alloc(&elems, bytes, s))) return rc;
        rc = hessian_elements(g, elems, 0, false, s);
        if (!rc) rc = eig_generic(elems, g->dtype, nd, total, o, s);
        pool_free(elems);
        if (rc) return rc;
    }
    if (kind == MI_RIDGE_MEIJERING) {
        const int grid = rg_grid(total);
        if (f32) hipLaunchKernelGGL(meijering_norm_kernel<float>, dim3(grid), dim3(kRgNT), 0, s, (const float *)scratch->data, (double *)out->data, total, (const unsigned long long *)work_dev);
        else hipLaunchKernelGGL(meijering_norm_kernel<double>, dim3(grid), dim3(kRgNT), 0, s, (const double *)scratch->data, (double *)out->data, total, (const unsigned long long *)work_dev);
        MI_HIP(hipGetLastError());
    }
    return MI_OK;
}

extern "C" int mi_ridge_fill_nonpositive(const mi_array *a, double value, mi_stream stream)
{
    int rc;
    if ((rc = check_array(a, "a"))) return rc;
    MI_REQUIRE(a->dtype == MI_F64 && is_contiguous(a), MI_ERR_INVALID_ARG, "a must be a C-contiguous float64 array");
    const int64_t total = numel(a);
    if (total == 0) return MI_OK;
    hipLaunchKernelGGL(fill_nonpositive_kernel, dim3(rg_grid(total)), dim3(kRgNT), 0, resolve_stream(stream), (double *)a->data, total, value);
    MI_HIP(hipGetLastError());
    return MI_OK;
}
