// template.hip -- skimage.feature.match_template: the normalised cross-correlation of an image (2-D) or a volume (3-D) with a
// template, as one launch.
//
// Reference path replaced: cupyimg/skimage/feature/template.py:125-205 (numpy.pad by the template's shape, an FFT convolution,
// two integral images built by cumsum in the image dtype, about ten whole-array passes).  Here the sums over every window are
// formed directly in float64; the padded image, the integral images, the cross-correlation and the denominator never exist in
// memory.
//
// The contract (include/mi355img.h, tests/helpers/template_ref.py).  Per axis the window of output index o starts at image
// index o - t / 2 (pad_input) or o (otherwise), t the template's extent; a sample outside the image is the one numpy.pad puts
// there (the index map of the mode, as often as it takes: the template may be as long as the axis; 'constant': cval).
//     x  = sum I * T,   s1 = sum I,   s2 = sum I * I      over the window, every sample converted to double first, every
//          product and sum a double rounded on its own, the taps in raster order (planes, rows, columns of the template):
//          x = x + I * T;  s1 = s1 + I;  s2 = s2 + I * I   -- the same order on both routes, whatever the tile and the slabs
//     num = x - s1 * mean
//     d   = s2 - (s1 * s1) / V;   d = d * ssd;   d = d < 0 ? 0 : d  (a NaN stays);   den = sqrt(d)
//     r   = den > DBL_EPSILON ? num / den : 0.0
// mean, ssd: the template's mean and sum of squared deviations, formed by the caller on the host; V: its number of samples.
// This file is compiled with -ffp-contract=off.
//
// mt_fused_kernel<T>: a workgroup of 256 threads owns tiles of TZ x TY x 128 outputs (images: 8 x 128, volumes: 2 x 4 x 128).
// It stages the samples the tile's windows cover -- the tile plus template - 1 samples per axis -- in LDS as doubles, every
// index through the boundary map, so the taps neither convert nor test anything.  A thread owns 4 consecutive outputs along x:
// it keeps a window of 4 samples and their squares in registers and reads ONE new sample from LDS per template column, which
// then serves 4 outputs (12 double additions and 4 multiplications per LDS read, one more multiplication for the square).
// The template value of a tap is the same for every lane: it is read through a uniform address, a scalar load.  The columns
// of a template row are taken four at a time, and the four template values and four window samples of the next chunk are
// loaded before the current chunk's 68 float64 instructions, which hide their latency (two waves a SIMD hide little).
// LDS layout: a row of the staged box is stored with one double of padding after every 4, so the 32 lanes of a row read
// addresses 5 doubles = 10 banks apart: 32 different even banks of the 64 a ds_read_b64 sees, no conflict (4 apart without the
// padding: 8 banks, a 4-way conflict).
// When the staged box is larger than the LDS budget (64 KiB: two workgroups per CU) the template is walked in slabs, in raster
// order: slabs of whole template planes where one plane's box fits, else slabs of rows of one plane at a time; x, s1 and s2
// stay in registers across the slabs, so the template's size is not bounded by LDS.  The route refuses (and the per-output
// kernel runs) only when the box of a single template row does not fit: templates more than about 690 columns wide.
//
// mt_generic_kernel<T>: one thread per output reading global memory, the same arithmetic in the same order: the comparator
// (mi_debug_set_match_template(1)) and the route of what the fused kernel refuses.
#include <float.h>

#include "skimage_common.hpp"

namespace mi {

constexpr int kMtNT = 256;
constexpr int kMtR = 4;                         // consecutive outputs of a thread along x
constexpr int kMtLdsBytes = 64 * 1024;
constexpr int kMtSmallLdsBytes = 4 * 1024;      // mi_debug_set_match_template(2)

static Knob g_mt_route{0};                      // 0 the planner, 1 the per-output kernel, 2 the fused kernel on small tiles

struct MtParams {
    int n[3];           // image: planes, rows, columns (images: 1 plane)
    int t[3];           // template
    int o[3];           // output
    int off[3];         // the window of output index i starts at image index i - off
    int tile[3];        // outputs of a workgroup's tile; tile[2] = lx * kMtR
    int nt[3];          // tiles per axis
    int lx;             // threads along x
    int kzs, kys;       // template planes and rows of a slab: kys == t[1] (slabs of planes) or kzs == 1 (slabs of rows)
    int pitch;          // doubles between two staged rows
    int mode;           // mi_mode of the boundary map
    double cval, mean, vol, ssd;
};

// where column c of a staged row lies: one double of padding after every kMtR
__device__ __forceinline__ int mt_skew(int c) { return c + c / kMtR; }
static inline int mt_pitch(int columns) { return columns + columns / kMtR + 1; }

__device__ __forceinline__ double mt_finish(double x, double s1, double s2, double mean, double vol, double ssd)
{
    const double num = x - s1 * mean;
    double d = s1 * s1;
    d = d / vol;
    d = s2 - d;
    d = d * ssd;
    d = d < 0.0 ? 0.0 : d;              // numpy.maximum(d, 0): a NaN stays a NaN
    const double den = sqrt_t<double>(d);
    return den > DBL_EPSILON ? num / den : 0.0;
}

template <typename T>
__global__ void __launch_bounds__(kMtNT)
mt_fused_kernel(const T *__restrict__ in, const double *__restrict__ tmpl, double *__restrict__ out, const MtParams p, const int64_t ntiles)
{
    __shared__ double box[kMtLdsBytes / sizeof(double)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lx = threadIdx.x % p.lx, slot = threadIdx.x / p.lx;
    const int cy = slot % p.tile[1], cz = slot / p.tile[1];
    const bool active = cz < p.tile[0];
    const int ex = p.tile[2] + p.t[2] - 1;              // columns of the staged box
    const int base = lx * (kMtR + 1);                   // mt_skew of the thread's first column
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int bx = (int)(tile % p.nt[2]);
        const int64_t rest = tile / p.nt[2];
        const int z0 = (int)(rest / p.nt[1]) * p.tile[0], y0 = (int)(rest % p.nt[1]) * p.tile[1], x0 = bx * p.tile[2];
        double x[kMtR], s1[kMtR], s2[kMtR];
#pragma unroll
        for (int r = 0; r < kMtR; r++) x[r] = s1[r] = s2[r] = 0.0;
        for (int kz0 = 0; kz0 < p.t[0]; kz0 += p.kzs) {
            const int nkz = min(p.kzs, p.t[0] - kz0);
            for (int ky0 = 0; ky0 < p.t[1]; ky0 += p.kys) {
                const int nky = min(p.kys, p.t[1] - ky0);
                const int sz = p.tile[0] + nkz - 1, sy = p.tile[1] + nky - 1;        // planes and rows of this slab's box
                // stage: box (bz, by, c) = the sample at (z0 - off + kz0 + bz, y0 - off + ky0 + by, x0 - off + c); a wave takes rows
                for (int row = wave; row < sz * sy; row += kMtNT / 64) {
                    const int bz = row / sy, by = row - bz * sy;
                    const int gz = bmap_near<int>(z0 - p.off[0] + kz0 + bz, p.n[0], p.mode);
                    const int gy = bmap_near<int>(y0 - p.off[1] + ky0 + by, p.n[1], p.mode);
                    const int64_t line = ((int64_t)gz * p.n[1] + gy) * p.n[2];
                    for (int c = lane; c < ex; c += 64) {
                        const int gx = bmap_near<int>(x0 - p.off[2] + c, p.n[2], p.mode);
                        double v = p.cval;
                        if (gz >= 0 && gy >= 0 && gx >= 0) v = (double)in[line + gx];
                        box[row * p.pitch + mt_skew(c)] = v;
                    }
                }
                __syncthreads();
                if (active) {
                    for (int kz = 0; kz < nkz; kz++) {
                        for (int ky = 0; ky < nky; ky++) {
                            const double *row = box + ((cz + kz) * sy + (cy + ky)) * p.pitch + base;
                            const double *trow = tmpl + ((int64_t)(kz0 + kz) * p.t[1] + (ky0 + ky)) * p.t[2];
                            // w[r]: the sample under template column kx0 for output r, q[r] its square.  Whole chunks of R template
                            // columns first: the R template values and the R window samples of the NEXT chunk are loaded
                            // before the current one is computed, so their latency hides behind 68 float64 instructions.
                            const int tx = p.t[2];
                            double w[kMtR], q[kMtR], tvn[kMtR], wn[kMtR];
#pragma unroll
                            for (int r = 0; r < kMtR; r++) {
                                w[r] = row[r];
                                q[r] = w[r] * w[r];
                                tvn[r] = wn[r] = 0.0;
                            }
                            // thread column kx0 + R + j lies at mt_skew(kx0 + R + j) = kx0 + R + j + kx0 / R + 1; the last one of
                            // the template's last whole chunk is past the staged row when no column follows: it is never used
                            auto fetch = [&](int kx0) {
#pragma unroll
                                for (int j = 0; j < kMtR; j++) tvn[j] = trow[kx0 + j];
#pragma unroll
                                for (int j = 0; j < kMtR - 1; j++) wn[j] = row[kx0 + kMtR + j + kx0 / kMtR + 1];
                                wn[kMtR - 1] = kx0 + kMtR < tx ? row[kx0 + 2 * kMtR + kx0 / kMtR] : 0.0;
                            };
                            int kx0 = 0;
                            if (kMtR <= tx) fetch(0);
                            for (; kx0 + kMtR <= tx; kx0 += kMtR) {
                                double tv[kMtR], wc[kMtR], qc[kMtR];
#pragma unroll
                                for (int j = 0; j < kMtR; j++) {
                                    tv[j] = tvn[j];
                                    wc[j] = wn[j];
                                }
                                if (kx0 + 2 * kMtR <= tx) fetch(kx0 + kMtR);
#pragma unroll
                                for (int j = 0; j < kMtR; j++) {
                                    qc[j] = wc[j] * wc[j];
#pragma unroll
                                    for (int r = 0; r < kMtR; r++) {
                                        const double v = j + r < kMtR ? w[(j + r) % kMtR] : wc[(j + r) % kMtR];
                                        x[r] = x[r] + v * tv[j];
                                        s1[r] = s1[r] + v;
                                        s2[r] = s2[r] + (j + r < kMtR ? q[(j + r) % kMtR] : qc[(j + r) % kMtR]);
                                    }
                                }
#pragma unroll
                                for (int r = 0; r < kMtR; r++) {
                                    w[r] = wc[r];
                                    q[r] = qc[r];
                                }
                            }
                            // the remaining tx % R columns: w[(j + r) % R] is the sample under column kx0 + j for output r
#pragma unroll
                            for (int j = 0; j < kMtR - 1; j++) {
                                const int kx = kx0 + j;
                                if (kx < tx) {
                                    const double tv = trow[kx];
#pragma unroll
                                    for (int r = 0; r < kMtR; r++) {
                                        const double v = w[(j + r) % kMtR];
                                        x[r] = x[r] + v * tv;
                                        s1[r] = s1[r] + v;
                                        s2[r] = s2[r] + q[(j + r) % kMtR];
                                    }
                                    if (kx + 1 < tx) {
                                        w[j] = row[kx0 + kMtR + j + kx0 / kMtR + 1];
                                        q[j] = w[j] * w[j];
                                    }
                                }
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (active) {
            const int oz = z0 + cz, oy = y0 + cy, ox = x0 + lx * kMtR;
            if (oz < p.o[0] && oy < p.o[1]) {
                double *o = out + ((int64_t)oz * p.o[1] + oy) * p.o[2];
#pragma unroll
                for (int r = 0; r < kMtR; r++)
                    if (ox + r < p.o[2]) o[ox + r] = mt_finish(x[r], s1[r], s2[r], p.mean, p.vol, p.ssd);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kMtNT)
mt_generic_kernel(const T *__restrict__ in, const double *__restrict__ tmpl, double *__restrict__ out, const MtParams p, const int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * kMtNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kMtNT) {
        const int ox = (int)(i % p.o[2]);
        const int64_t rest = i / p.o[2];
        const int oy = (int)(rest % p.o[1]), oz = (int)(rest / p.o[1]);
        double x = 0.0, s1 = 0.0, s2 = 0.0;
        const double *tv = tmpl;
        for (int kz = 0; kz < p.t[0]; kz++) {
            const int gz = bmap_near<int>(oz - p.off[0] + kz, p.n[0], p.mode);
            for (int ky = 0; ky < p.t[1]; ky++) {
                const int gy = bmap_near<int>(oy - p.off[1] + ky, p.n[1], p.mode);
                const int64_t line = ((int64_t)gz * p.n[1] + gy) * p.n[2];
                for (int kx = 0; kx < p.t[2]; kx++, tv++) {
                    const int gx = bmap_near<int>(ox - p.off[2] + kx, p.n[2], p.mode);
                    double v = p.cval;
                    if (gz >= 0 && gy >= 0 && gx >= 0) v = (double)in[line + gx];
                    x = x + v * *tv;
                    s1 = s1 + v;
                    s2 = s2 + v * v;
                }
            }
        }
        out[i] = mt_finish(x, s1, s2, p.mean, p.vol, p.ssd);
    }
}

// The tile and the slabs of the fused kernel.  false: not even the box of one template row fits the budget.
static bool mt_plan(MtParams *p, int rank, bool small, char *slabs, size_t nslabs)
{
    const int64_t budget = (small ? kMtSmallLdsBytes : kMtLdsBytes) / (int64_t)sizeof(double);
    p->lx = small ? 2 : 32;
    p->tile[0] = rank == 3 ? 2 : 1;
    p->tile[1] = small ? 3 : (rank == 3 ? 4 : 8);
    p->tile[2] = p->lx * kMtR;
    for (int d = 0; d < 3; d++) p->nt[d] = (p->o[d] + p->tile[d] - 1) / p->tile[d];
    p->pitch = mt_pitch(p->tile[2] + p->t[2] - 1);
    const int64_t row = p->pitch;
    auto fits = [&](int nkz, int nky) { return (int64_t)(p->tile[0] + nkz - 1) * (p->tile[1] + nky - 1) * row <= budget; };
    if (!fits(1, 1)) return false;
    if (fits(p->t[0], p->t[1])) {
        p->kzs = p->t[0];
        p->kys = p->t[1];
        snprintf(slabs, nslabs, "none");
    } else if (fits(1, p->t[1])) {
        p->kys = p->t[1];
        p->kzs = 1;
        while (fits(p->kzs + 1, p->t[1])) p->kzs++;
        snprintf(slabs, nslabs, "planes:%d", p->kzs);
    } else {
        p->kzs = 1;
        p->kys = 1;
        while (fits(1, p->kys + 1)) p->kys++;
        snprintf(slabs, nslabs, "rows:%d", p->kys);
    }
    return true;
}

template <typename T>
static int mt_launch(const mi_array *image, const double *tmpl, double *out, MtParams &p, const char *tname, hipStream_t s)
{
    const int rank = image->ndim;
    const int route = g_mt_route;
    const T *in = (const T *)image->data;
    char slabs[32];
    if (route != 1 && mt_plan(&p, rank, route == 2, slabs, sizeof(slabs))) {
        const int64_t ntiles = (int64_t)p.nt[0] * p.nt[1] * p.nt[2];
        const int grid = box_grid(ntiles);
        hipLaunchKernelGGL((mt_fused_kernel<T>), dim3(grid), dim3(kMtNT), 0, s, in, tmpl, out, p, ntiles);
        MI_HIP(hipGetLastError());
        note_kernel("mi::mt_fused_kernel<%s,%d> grid=%d tile=%dx%dx%d slabs=%s (one launch: the tile's windows staged in LDS as doubles, "
                    "four outputs a thread)", tname, rank, grid, p.tile[0], p.tile[1], p.tile[2], slabs);
        return MI_OK;
    }
    const int64_t total = (int64_t)p.o[0] * p.o[1] * p.o[2];
    const int grid = capped_grid(total, kMtNT, 1 << 16);
    hipLaunchKernelGGL((mt_generic_kernel<T>), dim3(grid), dim3(kMtNT), 0, s, in, tmpl, out, p, total);
    MI_HIP(hipGetLastError());
    note_kernel("mi::mt_generic_kernel<%s,%d> grid=%d (one launch: one thread per output)", tname, rank, grid);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" int mi_debug_set_match_template(int route)
{
    g_mt_route = route == 1 || route == 2 ? route : 0;
    return MI_OK;
}

extern "C" int mi_match_template(const mi_array *image, const mi_array *tmpl, const mi_array *out, int pad_input, int mode, double cval,
                                 double mean, double ssd, mi_stream stream)
{
    int rc;
    if ((rc = check_array(image, "image")) || (rc = check_array(tmpl, "template")) || (rc = check_array(out, "out"))) return rc;
    const int rank = image->ndim;
    MI_REQUIRE(rank == 2 || rank == 3, MI_ERR_INVALID_ARG, "match_template: images (rank 2) and volumes (rank 3)");
    MI_REQUIRE(tmpl->ndim == rank && out->ndim == rank, MI_ERR_INVALID_ARG, "match_template: the template and the output have the image's rank");
    MI_REQUIRE(tmpl->dtype == MI_F64 && out->dtype == MI_F64, MI_ERR_INVALID_ARG, "match_template: a float64 template and a float64 output");
    MI_REQUIRE(is_contiguous(image) && is_contiguous(tmpl) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "match_template needs C-contiguous arrays");
    MI_REQUIRE(mode >= MI_MODE_REFLECT && mode <= MI_MODE_GRID_WRAP, MI_ERR_INVALID_ARG, "match_template: unknown mode");
    MtParams p;
    memset(&p, 0, sizeof(p));
    p.n[0] = p.t[0] = p.o[0] = 1;
    for (int d = 0; d < rank; d++) {
        const int64_t n = image->shape[d], t = tmpl->shape[d];
        MI_REQUIRE(t >= 1 && t <= n, MI_ERR_INVALID_ARG, "match_template: a template of 1 to image.shape samples along every axis");
        MI_REQUIRE(out->shape[d] == (pad_input ? n : n - t + 1), MI_ERR_INVALID_ARG,
                   "match_template: the output has the image's shape (pad_input) or image.shape - template.shape + 1");
        if (n >= ((int64_t)1 << 30)) {
            set_error("match_template: axes of 2^30 samples or more are not supported");
            return MI_ERR_UNSUPPORTED;
        }
        const int a = d + 3 - rank;
        p.n[a] = (int)n;
        p.t[a] = (int)t;
        p.o[a] = (int)out->shape[d];
        p.off[a] = pad_input ? (int)(t / 2) : 0;
    }
    p.mode = filter_mode(mode);
    p.cval = cval;
    p.mean = mean;
    p.vol = (double)((int64_t)p.t[0] * p.t[1] * p.t[2]);
    p.ssd = ssd;
    hipStream_t s = resolve_stream(stream);
    const double *tv = (const double *)tmpl->data;
    double *o = (double *)out->data;
    switch (image->dtype) {
    case MI_U8: return mt_launch<uint8_t>(image, tv, o, p, "uint8", s);
    case MI_U16: return mt_launch<uint16_t>(image, tv, o, p, "uint16", s);
    case MI_I16: return mt_launch<int16_t>(image, tv, o, p, "int16", s);
    case MI_F32: return mt_launch<float>(image, tv, o, p, "float32", s);
    case MI_F64: return mt_launch<double>(image, tv, o, p, "float64", s);
    default: break;
    }
    set_error("match_template: uint8, uint16, int16, float32 and float64 images only (the caller converts)");
    return MI_ERR_UNSUPPORTED;
}
