// reconstruct.hip -- grey-level morphological reconstruction (skimage.morphology.reconstruction), one launch per call of
// mi_grey_reconstruction_step; the caller ping-pongs two buffers until the "changed" flag stays 0.
//
// Reference path replaced: cupyimg/skimage/morphology/greyreconstruct.py:18-238, which sorts on the device and then runs
// skimage's sequential reconstruction_loop ON THE HOST (:227-231).  What it computes: with S = the offsets d of the
// element's true cells relative to its centre (centre removed), reconstruction by dilation is the least image R >= seed
// that is stable under
//
//     R[q] <- min(mask[q], max(R[q], max over d in S of R[q - d]))
//
// (neighbours outside the image contribute nothing); by erosion: min and max swapped, the greatest image <= seed.  The
// operator is monotone and values are only compared and copied, so the fixed point is unique, independent of the order
// of the updates, and bit-identical to any correct host computation.
//
// greyrec3_kernel (2-D / 3-D, the 3^n box or the connectivity-1 cross, centred): the grey analogue of bitfill3_kernel
// (bitmorph3d.hip).  A workgroup stages a block of BZ x BY x BX voxels of `in` and `mask` plus a one-voxel halo in LDS and
// relaxes it IN PLACE until nothing inside changes; the halo keeps what the neighbours held when the launch began.  A round is
//   (1) every row swept along +x and -x:  r[i] = min(m[i], max(r[i], r[i - 1])) carried through the whole row by ONE
//       thread, so a value crosses the block in one pass where an iteration of the global operator moves it one voxel;
//   (2) the same along y and (3) along z, one thread per line -- lines of one pass are disjoint: no two threads touch a cell;
//   (4) box element only: one Jacobi step of the 20 (2-D: 4) diagonal taps, new values held in registers across a barrier.
// Every update is an application of the rule above to the current state, so any order reaches the same fixed point.
// A workgroup reads only `in` / `mask` and writes only its own block of `out`: nothing crosses workgroups inside a launch.
//
// greyrec_generic_kernel: one Jacobi step of the rule per launch over a tap table -- any rank, dtype, element, offset.
#include "nd_common.hpp"
#include "sep_common.hpp"
#include <algorithm>
#include <limits>
#include <vector>

namespace mi {

constexpr int kRecNT = 256;
constexpr int kRecLds = 80 * 1024;        // per workgroup: two workgroups share a CU's 160 KiB

struct RecParams {
    int nx, ny, nz;
    int bx, by, bz;         // block (own voxels)
    int hz;                 // 1: the block has a halo plane either side (volumes); 0: images
    int gx, gy, gz;         // staged extents = block + halo
    int pitch;              // LDS elements per staged row
    int nxt, nyt, nzt;
    int box;                // 1: the diagonal taps too (3^n box), 0: connectivity-1 cross
};

template <typename T, bool DIL>
__device__ __forceinline__ T rec_neutral()
{
    if constexpr (std::is_floating_point<T>::value) return DIL ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::infinity();
    else return DIL ? std::numeric_limits<T>::lowest() : std::numeric_limits<T>::max();
}

// the rule for one neighbour value: dilation min(m, max(r, nb)), erosion max(m, min(r, nb))
template <typename T, bool DIL>
__device__ __forceinline__ T rec_op(T r, T nb, T m)
{
    if constexpr (DIL) {
        const T a = nb > r ? nb : r;
        return a < m ? a : m;
    } else {
        const T a = nb < r ? nb : r;
        return a > m ? a : m;
    }
}

// One line of n own cells (first at `base`, `stride` apart; the cells before the first and after the last are halo) swept
// forwards and backwards.  Eight cells are read before the first is used: one LDS round trip per eight steps of the chain.
template <typename T, bool DIL>
__device__ __forceinline__ bool rec_sweep(T *__restrict__ R, const T *__restrict__ M, int base, int stride, int n)
{
    bool ch = false;
    T carry = R[base - stride];
    for (int i0 = 0; i0 < n; i0 += 8) {
        T r[8], m[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int c = base + min(i0 + j, n - 1) * stride;
            r[j] = R[c];
            m[j] = M[c];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (i0 + j < n) {
                const T v = rec_op<T, DIL>(r[j], carry, m[j]);
                if (v != r[j]) { R[base + (i0 + j) * stride] = v; ch = true; }
                carry = v;
            }
        }
    }
    carry = R[base + n * stride];
    for (int i0 = n - 1; i0 >= 0; i0 -= 8) {
        T r[8], m[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int c = base + max(i0 - j, 0) * stride;
            r[j] = R[c];
            m[j] = M[c];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (i0 - j >= 0) {
                const T v = rec_op<T, DIL>(r[j], carry, m[j]);
                if (v != r[j]) { R[base + (i0 - j) * stride] = v; ch = true; }
                carry = v;
            }
        }
    }
    return ch;
}

template <typename T, bool DIL>
__global__ void __launch_bounds__(kRecNT)
greyrec3_kernel(const T *__restrict__ in, T *__restrict__ out, const T *__restrict__ msk, const RecParams p, int32_t *flags)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rec_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gx = p.gx, gy = p.gy, gz = p.gz, pitch = p.pitch, hz = p.hz;
    const int plane = gy * pitch;
    T *R = reinterpret_cast<T *>(rec_lds);
    T *M = R + gz * plane;

    int b = blockIdx.x;
    const int xt = b % p.nxt;
    b /= p.nxt;
    const int yt = b % p.nyt, zt = b / p.nyt;
    const int x0 = xt * p.bx, y0 = yt * p.by, z0 = zt * p.bz;
    const int bxe = min(p.bx, p.nx - x0), bye = min(p.by, p.ny - y0), bze = min(p.bz, p.nz - z0);   // own voxels inside the array
    const T neutral = rec_neutral<T, DIL>();

    // ---- stage the block and its halo; positions outside the array hold the value that contributes nothing
    bool bad = false;
    for (int r = wave; r < gz * gy; r += kRecNT / 64) {
        const int zi = r / gy, yi = r - zi * gy;
        const int z = z0 - hz + zi, y = y0 - 1 + yi;
        const bool row_in = (unsigned)z < (unsigned)p.nz && (unsigned)y < (unsigned)p.ny;
        const int64_t g0 = ((int64_t)z * p.ny + y) * p.nx;
        for (int xi = lane; xi < gx; xi += 64) {
            const int x = x0 - 1 + xi;
            T v = neutral, m = neutral;
            if (row_in && (unsigned)x < (unsigned)p.nx) {
                v = in[g0 + x];
                m = msk[g0 + x];
                bad |= DIL ? v > m : v < m;          // the caller's precondition seed <= mask (>= for erosion)
            }
            R[r * pitch + xi] = v;
            M[r * pitch + xi] = m;
        }
    }
    __syncthreads();

    // ---- relax until nothing inside the block changes
    bool any = false;
    for (;;) {
        bool mine = false;
        for (int l = tid; l < bze * bye; l += kRecNT) {                 // rows along x
            const int zi = l / bye, yi = l - zi * bye;
            mine |= rec_sweep<T, DIL>(R, M, ((hz + zi) * gy + 1 + yi) * pitch + 1, 1, bxe);
        }
        __syncthreads();
        for (int l = tid; l < bze * bxe; l += kRecNT) {                 // lines along y
            const int zi = l / bxe, xi = l - zi * bxe;
            mine |= rec_sweep<T, DIL>(R, M, ((hz + zi) * gy + 1) * pitch + 1 + xi, pitch, bye);
        }
        __syncthreads();
        if (hz) {
            for (int l = tid; l < bye * bxe; l += kRecNT) {             // lines along z
                const int yi = l / bxe, xi = l - yi * bxe;
                mine |= rec_sweep<T, DIL>(R, M, (gy + 1 + yi) * pitch + 1 + xi, plane, bze);
            }
            __syncthreads();
        }
        if (p.box) {
            // the diagonal taps: 4 rows per wave and barrier pair, new values in registers until every thread has read
            const int nrows = bze * bye;
            for (int r0 = 0; r0 < nrows; r0 += 4 * (kRecNT / 64)) {
                T nv[4][2];
                bool wr[4][2];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int row = r0 + wave * 4 + k;
                    const int zi = row / bye, yi = row - zi * bye;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int xi = lane + 64 * h;
                        wr[k][h] = false;
                        nv[k][h] = neutral;
                        if (row < nrows && xi < bxe) {
                            const int c = ((hz + zi) * gy + 1 + yi) * pitch + 1 + xi;
                            const T r = R[c];
                            T nb = r;
#pragma unroll
                            for (int dz = -1; dz <= 1; dz++) {
                                if (dz != 0 && !hz) continue;
#pragma unroll
                                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                                    for (int dx = -1; dx <= 1; dx++) {
                                        if ((dz != 0) + (dy != 0) + (dx != 0) < 2) continue;
                                        const T t = R[c + dz * plane + dy * pitch + dx];
                                        nb = DIL ? (t > nb ? t : nb) : (t < nb ? t : nb);
                                    }
                            }
                            const T v = rec_op<T, DIL>(r, nb, M[c]);
                            nv[k][h] = v;
                            wr[k][h] = v != r;
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int row = r0 + wave * 4 + k;
                    const int zi = row / bye, yi = row - zi * bye;
#pragma unroll
                    for (int h = 0; h < 2; h++)
                        if (wr[k][h]) {
                            R[((hz + zi) * gy + 1 + yi) * pitch + 1 + lane + 64 * h] = nv[k][h];
                            mine = true;
                        }
                }
                __syncthreads();
            }
        }
        if (!__syncthreads_or(mine)) break;
        any = true;
    }

    // ---- write the block back (every voxel of the array belongs to exactly one block)
    for (int r = wave; r < bze * bye; r += kRecNT / 64) {
        const int zi = r / bye, yi = r - zi * bye;
        const int64_t g0 = ((int64_t)(z0 + zi) * p.ny + (y0 + yi)) * p.nx + x0;
        const int c = ((hz + zi) * gy + 1 + yi) * pitch + 1;
        for (int xi = lane; xi < bxe; xi += 64) out[g0 + xi] = R[c + xi];
    }
    if (tid == 0 && any) atomicOr(flags, 1);
    if (__any(bad) && lane == 0) atomicOr(flags + 1, 1);
}

// One Jacobi step of the rule for every voxel: neighbours from a tap table (the element mirrored on the host, so that tap t
// reads q - d).  `dil` is a run-time argument: the kernel is bound by its loads.
template <typename T, int ND>
__global__ void __launch_bounds__(256)
greyrec_generic_kernel(const T *__restrict__ in, T *__restrict__ out, const T *__restrict__ msk, NdGeom g, TapTable tt,
                       int64_t total, int dil, int32_t *flags)
{
    bool ch = false, bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const T r = in[i], m = msk[i];
        bad |= dil ? r > m : r < m;
        T v = r;
        const Voxel<ND> vx = locate<ND>(g, i);
        if (vx.interior) {
            for (int t = 0; t < tt.ntaps; t++) {
                const T nb = in[i + tt.lin[t]];
                v = dil ? (nb > v ? nb : v) : (nb < v ? nb : v);
            }
        } else {
            for (int t = 0; t < tt.ntaps; t++) {
                const int64_t pos = tap_pos<ND>(g, vx, tt.idx, t, MI_MODE_CONSTANT);
                if (pos < 0) continue;                       // outside the array: contributes nothing
                const T nb = in[pos];
                v = dil ? (nb > v ? nb : v) : (nb < v ? nb : v);
            }
        }
        v = dil ? (v < m ? v : m) : (v > m ? v : m);
        ch |= v != r;
        out[i] = v;
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) atomicOr(flags, 1);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags + 1, 1);
}

// test / tuning hook: block planes / rows of the next launches (0 = the planner's), 1 = every call on the generic kernel
static Knob g_rec_bz{0}, g_rec_by{0}, g_rec_generic{0};

static const char *rec_type_name(int dt)
{
    switch (dt) {
    case MI_U8: return "uint8";
    case MI_I16: return "int16";
    case MI_U16: return "uint16";
    default: return "float32";
    }
}

template <typename T, bool DIL>
static int launch_greyrec3(const mi_array *in, const mi_array *out, const mi_array *mask, const RecParams &p, size_t lds,
                           int32_t *flags, hipStream_t s)
{
    static PerDeviceOnce attr;
    if (!attr) {
        MI_HIP(hipFuncSetAttribute((const void *)greyrec3_kernel<T, DIL>, hipFuncAttributeMaxDynamicSharedMemorySize, kRecLds));
        attr = true;
    }
    const int64_t grid = (int64_t)p.nxt * p.nyt * p.nzt;
    hipLaunchKernelGGL((greyrec3_kernel<T, DIL>), dim3((unsigned)grid), dim3(kRecNT), lds, s, (const T *)in->data, (T *)out->data,
                       (const T *)mask->data, p, flags);
    MI_HIP(hipGetLastError());
    note_kernel("mi::greyrec3_kernel<%s,%s> grid=%lld block=%dx%dx%d %s (blocks relaxed in LDS to their fixed point: line sweeps along x, y, z)",
                rec_type_name(in->dtype), DIL ? "dilation" : "erosion", (long long)grid, p.bz, p.by, p.bx, p.box ? "box" : "cross");
    return MI_OK;
}

// 0 = not one of the two elements of the fast kernel, 1 = connectivity-1 cross, 2 = the full 3^n box (centred, centre ignored)
static int rec_element_kind(int nd, const uint8_t *structure, const int64_t *sshape, const int *offsets)
{
    int64_t n = 1;
    for (int d = 0; d < nd; d++) {
        if (sshape[d] != 3 || offsets[d] != 1) return 0;
        n *= 3;
    }
    bool cross = true, box = true;
    for (int64_t k = 0; k < n; k++) {
        int64_t r = k;
        int nonzero = 0;
        for (int d = 0; d < nd; d++) { nonzero += (r % 3) != 1; r /= 3; }
        if (nonzero == 0) continue;
        const bool set = structure[k] != 0;
        box = box && set;
        cross = cross && (set == (nonzero == 1));
    }
    return box ? 2 : cross ? 1 : 0;
}

static int greyrec3(const mi_array *in, const mi_array *out, const mi_array *mask, int kind, int dil, int32_t *flags, hipStream_t s)
{
    const int dt = in->dtype;
    const int pad = 3 - in->ndim;
    const int64_t nz = pad ? 1 : in->shape[0], ny = in->shape[1 - pad], nx = in->shape[2 - pad];
    const int es = (int)dtype_size(dt);
    RecParams p;
    memset(&p, 0, sizeof(p));
    p.nx = (int)nx; p.ny = (int)ny; p.nz = (int)nz;
    p.hz = nz > 1;
    p.box = kind == 2;
    // block: rows of 64 voxels (128 of one byte), 16 rows, as many planes (at most 16) as state + mask leave room for
    p.bx = (int)std::min<int64_t>(nx, es == 1 ? 128 : 64);
    p.by = (int)std::min<int64_t>(ny, g_rec_by ? (int)g_rec_by : 16);
    p.bz = (int)std::min<int64_t>(nz, g_rec_bz ? (int)g_rec_bz : 16);
    auto plan = [&]() {
        p.gx = p.bx + 2; p.gy = p.by + 2; p.gz = p.bz + 2 * p.hz;
        int words = (p.gx * es + 3) / 4;
        if (!(words & 1)) words++;                          // odd pitch in dwords: the rows of an x pass fall on different banks
        p.pitch = words * 4 / es;
        return (size_t)2 * p.gz * p.gy * p.pitch * es;
    };
    while (plan() > (size_t)kRecLds) {
        if (p.bz > 1) p.bz--;
        else if (p.by > 1) p.by--;
        else p.bx = (p.bx + 1) / 2;
    }
    const size_t lds = plan();
    p.nxt = (int)((nx + p.bx - 1) / p.bx); p.nyt = (int)((ny + p.by - 1) / p.by); p.nzt = (int)((nz + p.bz - 1) / p.bz);
    if ((int64_t)p.nxt * p.nyt * p.nzt >= ((int64_t)1 << 31)) { set_error("greyrec3: too many blocks for one grid"); return MI_ERR_UNSUPPORTED; }
#define REC_GO(T) (dil ? launch_greyrec3<T, true>(in, out, mask, p, lds, flags, s) : launch_greyrec3<T, false>(in, out, mask, p, lds, flags, s))
    switch (dt) {
    case MI_U8: return REC_GO(uint8_t);
    case MI_I16: return REC_GO(int16_t);
    case MI_U16: return REC_GO(uint16_t);
    default: return REC_GO(float);
    }
#undef REC_GO
}

static int greyrec_generic(const mi_array *in, const mi_array *out, const mi_array *mask, const uint8_t *structure,
                           const int64_t *sshape, const int *offsets, int dil, int32_t *flags, hipStream_t s)
{
    const int nd = in->ndim;
    // tap t of the table reads q + (t - off'): the element mirrored, off' = w - 1 - off, reads q - d; the centre is no tap
    int64_t n = 1;
    for (int d = 0; d < nd; d++) n *= sshape[d];
    std::vector<uint8_t> mirrored((size_t)n, 0);
    int origins[MI_MAX_NDIM];
    for (int d = 0; d < nd; d++) origins[d] = (int)(sshape[d] - 1 - offsets[d]) - (int)(sshape[d] / 2);
    for (int64_t k = 0; k < n; k++) {
        int64_t r = k, km = 0, mul = 1;
        bool centre = true;
        for (int d = nd - 1; d >= 0; d--) {
            const int64_t t = r % sshape[d];
            r /= sshape[d];
            centre = centre && t == offsets[d];
            km += (sshape[d] - 1 - t) * mul;
            mul *= sshape[d];
        }
        mirrored[(size_t)km] = structure[k] && !centre;
    }
    TapBuilder tb;
    TapTable tt;
    int rc;
    if ((rc = tb.init(in, sshape, origins, "selem"))) return rc;
    tb.fill([&](int64_t k) { return mirrored[(size_t)k] != 0; }, [](int64_t) { return 0.0; }, false);
    if ((rc = tb.upload(&tt, s))) return rc;
    const int64_t total = numel(in);
    dim3 grid;
    grid_for(total, 256, &grid);
    const int dt = in->dtype == MI_BOOL ? MI_U8 : in->dtype;
    rc = dispatch_dtype(dt, [&]<typename T>() -> int {
        const T *ip = (const T *)in->data, *mp = (const T *)mask->data;
        T *op = (T *)out->data;
        if (tb.g.ndim == 3)
            hipLaunchKernelGGL((greyrec_generic_kernel<T, 3>), grid, dim3(256), 0, s, ip, op, mp, tb.g, tt, total, dil, flags);
        else
            hipLaunchKernelGGL((greyrec_generic_kernel<T, MI_MAX_NDIM>), grid, dim3(256), 0, s, ip, op, mp, tb.g, tt, total, dil, flags);
        MI_HIP(hipGetLastError());
        return MI_OK;
    });
    if (rc) return rc;
    note_kernel("mi::greyrec_generic_kernel<%s> grid=%u (one step of the reconstruction rule per launch, rank %d, %d taps)",
                dil ? "dilation" : "erosion", grid.x, nd, tt.ntaps);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_reconstruct(int block_z, int block_y, int force_generic)
{
    g_rec_bz = block_z < 0 ? 0 : block_z;
    g_rec_by = block_y < 0 ? 0 : block_y;
    g_rec_generic = force_generic != 0;
    return MI_OK;
}

// One launch of grey reconstruction's relaxation: `out` = `in` moved towards the fixed point under `mask`; flags_dev[0] is
// OR-ed with 1 when any voxel of `out` differs from `in`, flags_dev[1] when `in` violates the order against `mask`
// somewhere.  method: 0 dilation, 1 erosion.  structure: host uint8 prod(sshape), offsets: the element's centre.
extern "C" int mi_grey_reconstruction_step(const mi_array *in, const mi_array *out, const mi_array *mask,
                                           const uint8_t *structure, const int64_t *sshape, const int *offsets, int method,
                                           int32_t *flags_dev, mi_stream stream)
{
    int rc;
    if ((rc = check_array(in, "in")) || (rc = check_array(out, "out")) || (rc = check_array(mask, "mask"))) return rc;
    MI_REQUIRE(structure && sshape && offsets && flags_dev, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(method == 0 || method == 1, MI_ERR_INVALID_ARG, "method must be 0 (dilation) or 1 (erosion)");
    MI_REQUIRE(in->ndim >= 1, MI_ERR_INVALID_ARG, "input must have at least one dimension");
    MI_REQUIRE(same_shape(in, out) && same_shape(in, mask), MI_ERR_INVALID_ARG, "seed, mask and output must have equal shapes");
    MI_REQUIRE(in->dtype == out->dtype && in->dtype == mask->dtype, MI_ERR_INVALID_ARG, "seed, mask and output must have one dtype");
    MI_REQUIRE(is_contiguous(in) && is_contiguous(out) && is_contiguous(mask), MI_ERR_NOT_CONTIGUOUS,
               "reconstruction needs C-contiguous arrays");
    MI_REQUIRE(in->data != out->data && mask->data != out->data, MI_ERR_INVALID_ARG, "output may not overlap seed or mask in memory");
    for (int d = 0; d < in->ndim; d++) {
        MI_REQUIRE(sshape[d] >= 1 && sshape[d] <= 32767, MI_ERR_INVALID_ARG, "selem: unsupported extent");
        MI_REQUIRE(offsets[d] >= 0 && offsets[d] < sshape[d], MI_ERR_INVALID_ARG, "offset must be included inside selem");
    }
    if (in->dtype == MI_F16) {
        set_error("reconstruction: float16 arrays are storage only (the caller converts to float32, which is exact here)");
        return MI_ERR_UNSUPPORTED;
    }
    if (numel(in) == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    const int dt = in->dtype;
    if (!g_rec_generic && (in->ndim == 2 || in->ndim == 3) && (dt == MI_U8 || dt == MI_BOOL || dt == MI_I16 || dt == MI_U16 || dt == MI_F32)
        && numel(in) < ((int64_t)1 << 40)) {
        bool fits = true;
        for (int d = 0; d < in->ndim; d++) fits = fits && in->shape[d] < ((int64_t)1 << 24);
        const int kind = rec_element_kind(in->ndim, structure, sshape, offsets);
        if (fits && kind) {
            mi_array a = *in, b = *out, c = *mask;
            if (dt == MI_BOOL) a.dtype = b.dtype = c.dtype = MI_U8;
            rc = greyrec3(&a, &b, &c, kind, method == 0, flags_dev, s);
            if (rc != MI_ERR_UNSUPPORTED) return rc;
        }
    }
    return greyrec_generic(in, out, mask, structure, sshape, offsets, method == 0, flags_dev, s);
}
