// Connected-component labelling (scipy.ndimage.label; reference cupyimg/scipy/ndimage/measurements.py:29-199).
//
// Union-find over int32 parent indices held in the output array itself.  Every union links the LARGER root under the
// SMALLER one, so the root of a component is its smallest linear index, i.e. its first voxel in C order -- and SciPy
// numbers features in C order of their first voxel.  The label of a voxel is therefore 1 + the rank of its root among all
// roots, which the count / scan / finalize passes below compute without sorting anything:
//
//   1. parents   tiled (rank 2 / 3, binary mode): union-find of one tile in LDS, global parent = global index of the tile
//                root;  generic (any rank, structure, greyscale mode): parent[i] = i for foreground voxels, -1 elsewhere
//   2. merge     tiled: voxels on tile faces unite with their backward neighbours in OTHER tiles (global atomicCAS);
//                generic: every voxel unites with every backward neighbour of the structure
//   3. count     new launch: parent[i] <- root(i) (flattening); one wave ballot per 64-voxel segment says which voxels are
//                roots: its popcount and its mask are stored per segment
//   4. scan      exclusive scan of the segment counts (three small launches); the total is num_features
//   5. finalize  label[i] = offset[root / 64] + popcount(mask[root / 64] below root % 64) + 1, in place
//
// Visibility across workgroups (per-XCD L2s are not coherent; a CU's L1 is not refreshed by other CUs' stores): inside
// the merge launch a plain load of parent[j] may return a value another workgroup has since replaced.  The design is
// correct under such stale reads, and relies on no fence to publish plain stores:
//   * a parent only ever decreases, and every value it ever held is an ancestor of the voxel in the current forest (a
//     root is re-pointed to a smaller root by CAS; flattening writes the root itself).  A stale read therefore still
//     walks towards the true root: find() may stop early at a node that WAS a root, never at a node of another set;
//   * the only write that changes the forest's shape is atomicCAS(&parent[ra], ra, rb) on a presumed root ra (device
//     scope, performed coherently).  If ra is no longer a root the CAS fails and returns ra's current parent, and the
//     union retries from that value -- so a union never links a non-root, and never loses one;
//   * find() terminates: parents strictly decrease along a path whatever version of them is read;
//   * anything that needs fully settled parents (count, finalize) is a new launch: the kernel boundary makes every
//     store and atomic of the merge launch visible.
#include <vector>
#include "common.hpp"

namespace mi {

static Knob g_label_generic{0};

constexpr int kLabelTile = 4096;             // voxels per tile of the LDS kernel

template <typename T>
__device__ __forceinline__ bool is_fg(T v) { return v != T(0); }    // NaN != 0: foreground, as in SciPy

// root of `a` by plain loads (possibly stale: see the file comment)
__device__ __forceinline__ int find_root(const int *p, int a)
{
    int q = p[a];
    while (q != a) {
        a = q;
        q = p[a];
    }
    return a;
}

__device__ __forceinline__ void unite(int *p, int a, int b)
{
    while (true) {
        a = find_root(p, a);
        b = find_root(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(&p[a], a, b);      // the only authority on whether a is still a root
        if (old == a) return;
        a = old;                                     // a was re-pointed meanwhile: continue from its current parent
    }
}

// ------------------------------------------------------------------ generic path
struct LabelGeom {
    int ndim, nnb;
    int64_t shape[MI_MAX_NDIM];
    int64_t cstride[MI_MAX_NDIM];                // elements
};

template <typename T>
__global__ void __launch_bounds__(256) label_init_kernel(const T *__restrict__ x, int *__restrict__ p, int64_t n, T bg, int all_fg)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = all_fg || x[i] != bg ? (int)i : -1;
}

// one thread per voxel; nb = nnb rows of (ndim deltas in -1..1), backward neighbours of a centrosymmetric structure
template <typename T, bool GREY>
__global__ void __launch_bounds__(256) label_connect_kernel(const T *__restrict__ x, int *p, int64_t n, LabelGeom g,
                                                            const int8_t *__restrict__ nb, T bg, int all_fg)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T v = x[i];
        if (!all_fg && !(v != bg)) continue;
        int64_t c[MI_MAX_NDIM];
        int64_t rem = i;
        for (int d = g.ndim - 1; d >= 0; d--) {
            const int64_t q = rem / g.shape[d];
            c[d] = rem - q * g.shape[d];
            rem = q;
        }
        for (int k = 0; k < g.nnb; k++) {
            const int8_t *dv = nb + k * g.ndim;
            int64_t j = i;
            bool in = true;
            for (int d = 0; d < g.ndim; d++) {
                const int64_t cc = c[d] + dv[d];
                in = in && cc >= 0 && cc < g.shape[d];
                j += dv[d] * g.cstride[d];
            }
            if (!in) continue;
            const T w = x[j];
            if (!all_fg && !(w != bg)) continue;
            if (GREY && !(w == v)) continue;
            unite(p, (int)i, (int)j);
        }
    }
}

// ------------------------------------------------------------------ tiled path (rank 3, binary mode)
struct TileGeom {
    int nz, ny, nx;
    int tz, ty, tx;          // tile shape, tz * ty * tx <= kLabelTile
    int ntz, nty, ntx;       // tiles per axis
    uint32_t smask;          // bit (dz + 1) * 9 + (dy + 1) * 3 + dx + 1: structure element
};

__device__ __forceinline__ int lds_find(const int *lp, int a)
{
    int q = lp[a];
    while (q != a) {
        a = q;
        q = lp[a];
    }
    return a;
}

__device__ __forceinline__ void lds_unite(int *lp, int a, int b)
{
    while (true) {
        a = lds_find(lp, a);
        b = lds_find(lp, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(&lp[a], a, b);
        if (old == a) return;
        a = old;
    }
}

// a tile's union-find in LDS: reads the input once, writes every voxel's global parent (its tile root's global index).
// Local index (a, b, c) -> (a * ty + b) * tx + c is monotone in the global C order, so the local root (the smallest local
// index) is also the component's smallest global index inside the tile.
template <typename T>
__global__ void __launch_bounds__(256) label_tile_kernel(const T *__restrict__ x, int *__restrict__ p, TileGeom g)
{
    __shared__ int lp[kLabelTile];
    const int t = blockIdx.x;
    const int bx = t % g.ntx, by = (t / g.ntx) % g.nty, bz = t / (g.ntx * g.nty);
    const int z0 = bz * g.tz, y0 = by * g.ty, x0 = bx * g.tx;
    const int tyx = g.ty * g.tx, nt = g.tz * tyx;
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int a = l / tyx, b = (l / g.tx) % g.ty, c = l % g.tx;
        const int z = z0 + a, y = y0 + b, xx = x0 + c;
        bool fg = false;
        if (z < g.nz && y < g.ny && xx < g.nx) fg = is_fg(x[((int64_t)z * g.ny + y) * g.nx + xx]);
        lp[l] = fg ? l : -1;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        if (lp[l] < 0) continue;                     // background stays -1 (unions only rewrite foreground entries)
        const int a = l / tyx, b = (l / g.tx) % g.ty, c = l % g.tx;
        for (int o = 0; o < 13; o++) {               // the 13 backward offsets of a 3 x 3 x 3 neighbourhood
            if (!((g.smask >> o) & 1u)) continue;
            const int da = o / 9 - 1, db = (o / 3) % 3 - 1, dc = o % 3 - 1;
            const int na = a + da, nb = b + db, nc = c + dc;
            if (na < 0 || na >= g.tz || nb < 0 || nb >= g.ty || nc < 0 || nc >= g.tx) continue;
            const int m = (na * g.ty + nb) * g.tx + nc;
            if (lp[m] < 0) continue;
            lds_unite(lp, l, m);
        }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int a = l / tyx, b = (l / g.tx) % g.ty, c = l % g.tx;
        const int z = z0 + a, y = y0 + b, xx = x0 + c;
        if (z >= g.nz || y >= g.ny || xx >= g.nx) continue;
        int r = lp[l];
        if (r >= 0) {
            r = lds_find(lp, l);
            const int ra = r / tyx, rb = (r / g.tx) % g.ty, rc = r % g.tx;
            r = (int)(((int64_t)(z0 + ra) * g.ny + (y0 + rb)) * g.nx + (x0 + rc));
        }
        p[((int64_t)z * g.ny + y) * g.nx + xx] = r;
    }
}

// voxels on a tile's faces unite with their backward neighbours that lie in another tile: every cross-tile edge once
template <typename T>
__global__ void __launch_bounds__(256) label_faces_kernel(const T *__restrict__ x, int *p, TileGeom g)
{
    const int t = blockIdx.x;
    const int bx = t % g.ntx, by = (t / g.ntx) % g.nty, bz = t / (g.ntx * g.nty);
    const int z0 = bz * g.tz, y0 = by * g.ty, x0 = bx * g.tx;
    const int tyx = g.ty * g.tx, nt = g.tz * tyx;
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int a = l / tyx, b = (l / g.tx) % g.ty, c = l % g.tx;
        // an axis whose single tile row covers the whole extent has no neighbour in another tile (images: z)
        if ((g.ntz == 1 || (a > 0 && a < g.tz - 1)) && (g.nty == 1 || (b > 0 && b < g.ty - 1)) &&
            (g.ntx == 1 || (c > 0 && c < g.tx - 1)))
            continue;
        const int z = z0 + a, y = y0 + b, xx = x0 + c;
        if (z >= g.nz || y >= g.ny || xx >= g.nx) continue;
        const int64_t i = ((int64_t)z * g.ny + y) * g.nx + xx;
        if (!is_fg(x[i])) continue;
        for (int o = 0; o < 13; o++) {
            if (!((g.smask >> o) & 1u)) continue;
            const int da = o / 9 - 1, db = (o / 3) % 3 - 1, dc = o % 3 - 1;
            const int na = a + da, nb = b + db, nc = c + dc;
            if (na >= 0 && na < g.tz && nb >= 0 && nb < g.ty && nc >= 0 && nc < g.tx) continue;   // same tile: done
            const int zz = z + da, yy = y + db, xn = xx + dc;
            if (zz < 0 || zz >= g.nz || yy < 0 || yy >= g.ny || xn < 0 || xn >= g.nx) continue;
            const int64_t j = ((int64_t)zz * g.ny + yy) * g.nx + xn;
            if (!is_fg(x[j])) continue;
            unite(p, (int)i, (int)j);
        }
    }
}

// ------------------------------------------------------------------ count / scan / finalize (both paths)
// parent[i] <- root(i); segment s = voxels [64 s, 64 s + 64) = one wave (blocks of 256, grid stride a multiple of 256)
__global__ void __launch_bounds__(256) label_count_kernel(int *p, int64_t n, int *__restrict__ segcnt,
                                                          uint64_t *__restrict__ segmask)
{
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        bool root = false;
        if (i < n) {
            const int q = p[i];
            if (q >= 0) {
                root = q == (int)i;
                if (!root) p[i] = find_root(p, q);
            }
        }
        const uint64_t m = __ballot(root);
        const int64_t seg = i >> 6;
        if ((threadIdx.x & 63) == 0 && (seg << 6) < n) {
            segcnt[seg] = __popcll(m);
            segmask[seg] = m;
        }
    }
}

constexpr int kScanPer = 8;                  // segment counts per thread of the scan (a block covers 2048)

__device__ __forceinline__ int block_excl_scan(int v, int *sh, int *total)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const int incl = sh[tid];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(256) label_scan_reduce_kernel(const int *__restrict__ cnt, int64_t nseg, int *__restrict__ bsum)
{
    __shared__ int sh[256];
    const int64_t b0 = (int64_t)blockIdx.x * 256 * kScanPer;
    int s = 0;
    for (int k = 0; k < kScanPer; k++) {
        const int64_t j = b0 + (int64_t)threadIdx.x * kScanPer + k;
        if (j < nseg) s += cnt[j];
    }
    int tot;
    block_excl_scan(s, sh, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one block: exclusive scan of the block sums in place; total -> *total
__global__ void __launch_bounds__(256) label_scan_top_kernel(int *bsum, int nb, int *total)
{
    __shared__ int sh[256];
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int j = base + threadIdx.x;
        const int v = j < nb ? bsum[j] : 0;
        int tot;
        const int e = block_excl_scan(v, sh, &tot);
        if (j < nb) bsum[j] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(256) label_scan_down_kernel(int *cnt, int64_t nseg, const int *__restrict__ bsum)
{
    __shared__ int sh[256];
    const int64_t b0 = (int64_t)blockIdx.x * 256 * kScanPer;
    int v[kScanPer];
    int s = 0;
    for (int k = 0; k < kScanPer; k++) {
        const int64_t j = b0 + (int64_t)threadIdx.x * kScanPer + k;
        v[k] = j < nseg ? cnt[j] : 0;
        s += v[k];
    }
    int tot;
    int e = block_excl_scan(s, sh, &tot) + bsum[blockIdx.x];
    for (int k = 0; k < kScanPer; k++) {
        const int64_t j = b0 + (int64_t)threadIdx.x * kScanPer + k;
        if (j < nseg) cnt[j] = e;
        e += v[k];
    }
}

__global__ void __launch_bounds__(256) label_finalize_kernel(int *p, int64_t n, const int *__restrict__ segoff,
                                                             const uint64_t *__restrict__ segmask)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = p[i];
        if (r < 0) { p[i] = 0; continue; }
        const int s = r >> 6;
        const uint64_t below = segmask[s] & ((1ull << (r & 63)) - 1ull);
        p[i] = segoff[s] + __popcll(below) + 1;
    }
}

static int grid_for(int64_t n)
{
    return (int)std::min<int64_t>((n + 255) / 256, (int64_t)device_cus() * 32);
}

// count, scan and finalize on the int32 parent array `p` of n voxels; num_features -> *num (one synchronisation)
static int label_number(int *p, int64_t n, int64_t *num, hipStream_t s)
{
    const int64_t nseg = (n + 63) / 64;
    const int64_t per = 256 * kScanPer;
    const int nblk = (int)((nseg + per - 1) / per);
    void *ws = nullptr;
    const size_t bytes = (size_t)nseg * 8 + (size_t)nseg * 4 + (size_t)nblk * 4 + 16;
    int rc = pool_alloc(&ws, bytes, s);
    if (rc) return rc;
    uint64_t *segmask = (uint64_t *)ws;
    int *segcnt = (int *)(segmask + nseg);
    int *bsum = segcnt + nseg;
    int *total = bsum + nblk;
    const int grid = grid_for(n);
    hipLaunchKernelGGL(label_count_kernel, dim3(grid), dim3(256), 0, s, p, n, segcnt, segmask);
    hipLaunchKernelGGL(label_scan_reduce_kernel, dim3(nblk), dim3(256), 0, s, (const int *)segcnt, nseg, bsum);
    hipLaunchKernelGGL(label_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, nblk, total);
    hipLaunchKernelGGL(label_scan_down_kernel, dim3(nblk), dim3(256), 0, s, segcnt, nseg, (const int *)bsum);
    hipLaunchKernelGGL(label_finalize_kernel, dim3(grid), dim3(256), 0, s, p, n, (const int *)segcnt,
                       (const uint64_t *)segmask);
    hipError_t e = hipGetLastError();
    int host_total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&host_total, total, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    pool_free(ws);
    if (e != hipSuccess) { set_error("HIP error: %s", hipGetErrorString(e)); return MI_ERR_INTERNAL; }
    *num = host_total;
    return MI_OK;
}

// tile shape: volumes 8 x 16 x 32 (faces are 38 % of a tile), one-plane volumes 1 x 64 x 64
static void plan_tiles(TileGeom &g)
{
    if (g.nz == 1) { g.tz = 1; g.ty = 64; g.tx = 64; }
    else { g.tz = 8; g.ty = 16; g.tx = 32; }
    g.ntz = (g.nz + g.tz - 1) / g.tz;
    g.nty = (g.ny + g.ty - 1) / g.ty;
    g.ntx = (g.nx + g.tx - 1) / g.tx;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_debug_set_label_generic(int on) { g_label_generic = on; return MI_OK; }

int mi_label(const mi_array *in, const mi_array *out, const uint8_t *structure, int greyscale, int64_t background,
             int64_t *num_features, mi_stream stream)
{
    int rc;
    if ((rc = check_array(in, "input")) || (rc = check_array(out, "output"))) return rc;
    MI_REQUIRE(structure && num_features, MI_ERR_INVALID_ARG, "NULL argument");
    MI_REQUIRE(out->dtype == MI_I32 && same_shape(in, out), MI_ERR_INVALID_ARG, "output must be int32 of the input's shape");
    MI_REQUIRE(is_contiguous(in) && is_contiguous(out), MI_ERR_NOT_CONTIGUOUS, "mi_label needs C-contiguous arrays");
    MI_REQUIRE(in->ndim >= 1, MI_ERR_INVALID_ARG, "mi_label: rank 1 .. 8");
    const int64_t n = numel(in);
    MI_REQUIRE(n < ((int64_t)1 << 31), MI_ERR_INVALID_ARG, "label: arrays of 2**31 voxels or more are not supported (int32 parents)");
    *num_features = 0;
    if (n == 0) return MI_OK;
    hipStream_t s = resolve_stream(stream);
    int *p = (int *)out->data;
    const int nd = in->ndim;
    int nsz = 1;
    for (int d = 0; d < nd; d++) nsz *= 3;
    // backward neighbours: structure elements whose ravelled offset (base 3, centred) is negative
    std::vector<int8_t> nb;
    int nnb = 0;
    uint32_t smask = 0;
    for (int e = 0; e < nsz; e++) {
        if (!structure[e]) continue;
        int8_t dv[MI_MAX_NDIM];
        int rem = e, off = 0, w = 1;
        for (int d = nd - 1; d >= 0; d--) { dv[d] = (int8_t)(rem % 3 - 1); rem /= 3; off += dv[d] * w; w *= 3; }
        if (off >= 0) continue;
        nb.insert(nb.end(), dv, dv + nd);
        nnb++;
        if (nd == 2 || nd == 3) {                    // the tiled kernels' 3 x 3 x 3 bit mask (images: the middle plane)
            const int dz = nd == 3 ? dv[0] : 0, dy = dv[nd - 2], dx = dv[nd - 1];
            smask |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1);
        }
    }
    const bool tiled = !greyscale && background == 0 && (nd == 2 || nd == 3) && !g_label_generic;
    if (tiled) {
        TileGeom g{};
        g.nz = nd == 3 ? (int)in->shape[0] : 1;
        g.ny = (int)in->shape[nd - 2];
        g.nx = (int)in->shape[nd - 1];
        g.smask = smask;
        plan_tiles(g);
        const int64_t tiles = (int64_t)g.ntz * g.nty * g.ntx;
        rc = dispatch_dtype(in->dtype, [&]<typename T>() -> int {
            hipLaunchKernelGGL((label_tile_kernel<T>), dim3((unsigned)tiles), dim3(256), 0, s, (const T *)in->data, p, g);
            if (smask) hipLaunchKernelGGL((label_faces_kernel<T>), dim3((unsigned)tiles), dim3(256), 0, s, (const T *)in->data, p, g);
            MI_HIP(hipGetLastError());
            return MI_OK;
        });
        if (rc) return rc;
        note_kernel("mi::label_tile_kernel (%d x %d x %d tiles) + label_faces_kernel grid=%lld", g.tz, g.ty, g.tx, (long long)tiles);
    } else {
        LabelGeom g{};
        g.ndim = nd;
        g.nnb = nnb;
        int64_t st = 1;
        for (int d = nd - 1; d >= 0; d--) { g.shape[d] = in->shape[d]; g.cstride[d] = st; st *= in->shape[d]; }
        Scratch sc;
        if (nnb && (rc = sc.upload(nb.data(), nb.size(), s))) return rc;
        const int grid = grid_for(n);
        rc = dispatch_dtype(in->dtype, [&]<typename T>() -> int {
            // a background the dtype cannot hold (bool and -1, uint8 and 300) equals no voxel: everything is foreground
            bool fits;
            if constexpr (std::is_same<T, bool>::value) fits = background == 0 || background == 1;
            else if constexpr (std::is_floating_point<T>::value) fits = (double)(T)background == (double)background;
            else if constexpr (std::is_same<T, uint64_t>::value) fits = background >= 0;
            else fits = (int64_t)(T)background == background;
            const T bg = fits ? (T)background : T(0);
            const int all_fg = !fits;
            hipLaunchKernelGGL((label_init_kernel<T>), dim3(grid), dim3(256), 0, s, (const T *)in->data, p, n, bg, all_fg);
            if (nnb) {
                if (greyscale)
                    hipLaunchKernelGGL((label_connect_kernel<T, true>), dim3(grid), dim3(256), 0, s, (const T *)in->data, p, n, g,
                                       (const int8_t *)sc.ptr, bg, all_fg);
                else
                    hipLaunchKernelGGL((label_connect_kernel<T, false>), dim3(grid), dim3(256), 0, s, (const T *)in->data, p, n, g,
                                       (const int8_t *)sc.ptr, bg, all_fg);
            }
            MI_HIP(hipGetLastError());
            return MI_OK;
        });
        if (rc) return rc;
        note_kernel("mi::label_connect_kernel<%s> (generic, rank %d, %d neighbours) grid=%d", greyscale ? "grey" : "binary", nd, nnb, grid);
    }
    return label_number(p, n, num_features, s);
}

}  // extern "C"
