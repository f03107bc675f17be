// skimage_common.hpp -- scaffolding shared by the skimage kernels; the arithmetic of every operator stays in its own file.
//
//   edges.hip, corners.hip              BoxDims, plan_halo1_box, box_grid, box_origin, stage_halo1_box
//   ridges.hip                          BoxDims (its planner and its halo-2 loader are its own), VoxelGeom, voxel_geom,
//                                       voxel_coords
//   tv_chambolle.hip, tvl1.hip          VoxelGeom, voxel_geom, voxel_coords
//   all of them and morphsnakes.hip     capped_grid, sqrt_t
#pragma once
#include <algorithm>

#include "common.hpp"

namespace mi {

// sqrt in T: correctly rounded, like every other operation of these files (-ffp-contract=off)
template <typename T>
__device__ __forceinline__ T sqrt_t(T v)
{
    if constexpr (std::is_same<T, float>::value) return __builtin_sqrtf(v);
    else return __builtin_sqrt(v);
}

// Workgroups of a grid-stride kernel with one thread per element: ceil(total / block), at least 1, at most `cap`.  The cap
// belongs to the call site: where a kernel writes per-workgroup partial sums it fixes the summation order, so the result bits.
static inline int capped_grid(int64_t total, int block, int64_t cap)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + block - 1) / block, cap));
}

// ------------------------------------------------------------------ core boxes of a 2-D / 3-D array
struct BoxDims {
    int n[3];           // nz, ny, nx (images: nz = 1)
    int t[3];           // the core box: planes, rows, columns
    int nt[3];          // boxes per axis
};

constexpr int kBoxMaxGrid = 1 << 20;

// workgroups of a kernel whose workgroups take the boxes one after the other
static inline int box_grid(int64_t nboxes) { return (int)std::min<int64_t>(nboxes, kBoxMaxGrid); }

// The plan of the kernels that stage a core box plus ONE sample either way: 8 planes of 8 x 64 voxels (float64: 4 planes),
// images 32 x 64 pixels; `small`: 2 x 3 x 5, so that small test arrays have seams along every axis.  MI_ERR_UNSUPPORTED:
// an axis of 2^30 or more; MI_ERR_INTERNAL (no message set): the staged box is larger than the caller's `lds_bytes`.
static inline int plan_halo1_box(const mi_array *image, bool small, int64_t lds_bytes, BoxDims *b, int64_t *nboxes)
{
    const int rank = image->ndim;
    const int64_t es = (int64_t)dtype_size(image->dtype);
    for (int d = 0; d < 3; d++) {
        const int64_t n = d < 3 - rank ? 1 : image->shape[d - (3 - rank)];
        if (n >= ((int64_t)1 << 30)) return MI_ERR_UNSUPPORTED;
        b->n[d] = (int)n;
    }
    if (rank == 3) {
        b->t[0] = small ? 2 : (es == 4 ? 8 : 4);
        b->t[1] = small ? 3 : 8;
    } else {
        b->t[0] = 1;
        b->t[1] = small ? 3 : 32;
    }
    b->t[2] = small ? 5 : 64;
    *nboxes = 1;
    for (int d = 0; d < 3; d++) {
        b->t[d] = std::min(b->t[d], b->n[d]);
        b->nt[d] = (b->n[d] + b->t[d] - 1) / b->t[d];
        *nboxes *= b->nt[d];
    }
    const int64_t staged = (int64_t)(b->t[0] + (rank == 3 ? 2 : 0)) * (b->t[1] + 2) * (b->t[2] + 2);
    return staged * es > lds_bytes ? MI_ERR_INTERNAL : MI_OK;
}

// first voxel of core box number `box` (boxes in C order)
__device__ __forceinline__ void box_origin(const BoxDims &b, int64_t box, int &z0, int &y0, int &x0)
{
    const int bx = (int)(box % b.nt[2]);
    const int64_t rest = box / b.nt[2];
    const int by = (int)(rest % b.nt[1]), bz = (int)(rest / b.nt[1]);
    z0 = bz * b.t[0];
    y0 = by * b.t[1];
    x0 = bx * b.t[2];
}

// Stage the core box at (z0, y0, x0) and its one-sample halo (RANK 2: none along z) as tile[sz][sy][sx], sy < t[1] + 2,
// sx < t[2] + 2: the sample of voxel (z0 + sz - 1, y0 + sy - 1, x0 + sx - 1), every index through the boundary map, so a
// staged index is always inside the array (the map of 'constant' gives -1: a zero is staged and never used).  A workgroup
// of NT threads: a wave takes rows, its lanes along x.  The caller synchronises.
template <typename T, int RANK, int NT>
__device__ __forceinline__ void stage_halo1_box(T *tile, const T *__restrict__ in, const BoxDims &b, int mode, int z0, int y0, int x0)
{
    constexpr int HZ = RANK == 3 ? 1 : 0;
    const int ez = b.t[0] + 2 * HZ, ey = b.t[1] + 2, ex = b.t[2] + 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int row = wave; row < ez * ey; row += NT / 64) {
        const int sz = row / ey, sy = row - sz * ey;
        const int gz = HZ ? bmap_near<int>(z0 + sz - 1, b.n[0], mode) : 0;
        const int gy = bmap_near<int>(y0 + sy - 1, b.n[1], mode);
        for (int sx = lane; sx < ex; sx += 64) {
            const int gx = bmap_near<int>(x0 + sx - 1, b.n[2], mode);
            T v = T(0);
            if (gz >= 0 && gy >= 0 && gx >= 0) v = in[((int64_t)gz * b.n[1] + gy) * b.n[2] + gx];
            tile[row * ex + sx] = v;
        }
    }
}

// (The walk over the core box that follows stays in each kernel: as a function taking the voxel's arithmetic as a lambda
// it compiled to different code, 2 to 13 more registers in st_fused_kernel.)

// ------------------------------------------------------------------ one thread per voxel, any rank up to MAXND
template <int MAXND>
struct VoxelGeom {
    int nd;
    int64_t total;
    int64_t shape[MAXND];
    int64_t stride[MAXND];       // elements, C order
};

template <int MAXND>
static inline void voxel_geom(const mi_array *a, VoxelGeom<MAXND> *g)
{
    memset(g, 0, sizeof(*g));
    g->nd = a->ndim;
    int64_t st = 1;
    for (int d = a->ndim - 1; d >= 0; d--) {
        g->shape[d] = a->shape[d];
        g->stride[d] = st;
        st *= a->shape[d];
    }
    g->total = st;
}

// c[0 .. ND - 1]: the coordinates of linear index i.  ND is the rank the kernel was built for; RUNTIME_RANK: it serves every
// rank up to ND, the axes from g.nd on are skipped and get 0.
template <int ND, bool RUNTIME_RANK, int MAXND>
__device__ __forceinline__ void voxel_coords(const VoxelGeom<MAXND> &g, int64_t i, int64_t *c)
{
    int64_t r = i;
#pragma unroll
    for (int a = ND - 1; a >= 0; a--) {
        c[a] = 0;
        if (!RUNTIME_RANK || a < g.nd) {
            const int64_t q = r / g.shape[a];
            c[a] = r - q * g.shape[a];
            r = q;
        }
    }
}

}  // namespace mi
