// components.hip -- the tail of the 2-D (fundus / polyp) evaluation on the device: 8-connected component labelling, removal of fragmentary segments
// (test_util2d.py:267-289), the row extents behind the vertical cup/disc ratio (utils/losses.py:76-127) and the n-hot -> pixel-value maps
// (datasets2d.py:144-171, 225-...); further down the connected-component post-processing of 3-D predictions (6- / 26-connected labelling of volumes, the keep rule,
// the BraTS rule).  Integer kernels with exact, order-independent results; no host round trip, no stream synchronisation.
//
// Labelling of uint8 planes [P][H][W] in three launches.  A label is 1 + the raster index (inside its plane) of another pixel of the same component that is
// NOT LATER in raster order -- a parent pointer -- and 0 on the background; a pixel whose label is 1 + its own index is a root.
//   (a) ccl_tile_kernel     one workgroup labels a CCL_TH x CCL_TW tile in LDS by label equivalence to a fixed point (Kalentev et al. 2011): every component of the
//                           tile ends on its first pixel; the pixels of each are counted with LDS integer adds; the tile writes global parent pointers and, at
//                           each tile-local root, the local count (0 everywhere else).
//   (b) ccl_seam_kernel     one thread per pixel on the right column / bottom row of a tile unites it with its set neighbours across the seam (right, below and
//                           both diagonals) by the union that needs only atomicMin (Komura 2015; Playne & Hawick 2018).
//   (c) ccl_flatten_kernel  every pixel is pointed at its root, and every tile-local root hands its count to the final root: ONE integer atomicAdd per
//                           tile-local component, not one per pixel (a 10^6-pixel disc adding into one word would run at the single-address atomic rate).
//
// Why (b) is right without locks, and ends.  Labels only ever DECREASE, and a cell only ever points to a member of its own set, because the only writes are
// atomicMin(&L[a], b + 1) with b < a and a, b being united.  So whatever a thread reads -- also a stale value out of a cache that another XCD's atomic has since
// lowered -- is 1 + an ancestor-or-former-ancestor: following such values walks down a strictly decreasing sequence of non-negative indices inside the plane and
// stops at a cell that WAS a root when it was read.  Two walks that meet prove the sets are already one.  Otherwise the larger root a takes atomicMin with the
// smaller one; the returned old value is the arbiter: if it is a + 1, a was still a root and is now linked -- done; else some other thread linked a to old - 1 < a
// in between (that link may just have been replaced by ours, so it must be re-established): continue uniting old - 1 with b.  Every iteration therefore either
// ends or strictly lowers one of the two positive integers (a, b): it terminates.  Cells that other workgroups may change in the same launch are read through
// SEGX_TEAM_LOAD (agent scope: not out of this CU's L1); nothing here waits for another workgroup.
#include "common.h"

namespace segx {

constexpr int CCL_TH = SEGX_CCL_TILE_H, CCL_TW = SEGX_CCL_TILE_W;      // 32 x 64: label rows of 256 bytes
constexpr int CCL_PW = CCL_TW + 2, CCL_PN = (CCL_TH + 2) * CCL_PW;      // the LDS tile carries a one-pixel unset rim: no neighbour test at its edges
constexpr int CCL_PER = CCL_TH * CCL_TW / 256;                          // pixels a thread owns: rows 4k + wave, column lane
static_assert(CCL_TW == 64 && CCL_TH % 4 == 0, "a wave owns a tile row");

__global__ __launch_bounds__(256) void ccl_tile_kernel(const uint8_t* __restrict__ fg, int bg, int* __restrict__ labels, int* __restrict__ sizes, int H, int W,
                                                       int tiles_x, int tiles_y) {
    __shared__ int lab[CCL_PN], cnt[CCL_PN];
    __shared__ int changed[2];
    const int tid = threadIdx.x, lx = tid & 63, lw = tid >> 6;
    const int64_t blk = blockIdx.x, per_plane = (int64_t)tiles_x * tiles_y;
    const int64_t plane = blk / per_plane;
    const int t = (int)(blk - plane * per_plane), x0 = (t % tiles_x) * CCL_TW, y0 = (t / tiles_x) * CCL_TH;
    const int64_t base = plane * H * W;
    const int gx = x0 + lx;
    for (int i = tid; i < CCL_PN; i += 256) { lab[i] = -1; cnt[i] = 0; }
    if (tid < 2) changed[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CCL_PER; ++k) {
        const int ly = 4 * k + lw, gy = y0 + ly, c = (ly + 1) * CCL_PW + lx + 1;
        if (gx < W && gy < H && fg[base + (int64_t)gy * W + gx] != bg) lab[c] = c;
    }
    __syncthreads();
    // label equivalence: (scan) a pixel whose neighbourhood holds a smaller label lowers the label cell of ITS root; (analysis) every pixel follows the cells down to
    // a root.  Labels never rise, an iteration without a change is the fixed point: all pixels of a component carry its smallest (= first, raster order) cell.
    for (int it = 0;; ++it) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < CCL_PER; ++k) {
            const int c = (4 * k + lw + 1) * CCL_PW + lx + 1, r = lab[c];
            if (r < 0) continue;
            int m = r;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int v = lab[c + dy * CCL_PW + dx];
                    if (v >= 0 && v < m) m = v;
                }
            if (m < r) { atomicMin(&lab[r], m); any = true; }
        }
        if (any) changed[it & 1] = 1;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CCL_PER; ++k) {
            const int c = (4 * k + lw + 1) * CCL_PW + lx + 1;
            int r = lab[c];
            if (r < 0) continue;
            for (int v = lab[r]; v < r; v = lab[r]) r = v;       // cells hold values <= their own index: strictly down to a root
            lab[c] = r;
        }
        if (tid == 0) changed[(it + 1) & 1] = 0;                  // the other flag: nobody reads or sets it before the next barrier
        const int again = changed[it & 1];
        __syncthreads();
        if (!again) break;
    }
#pragma unroll
    for (int k = 0; k < CCL_PER; ++k) {
        const int r = lab[(4 * k + lw + 1) * CCL_PW + lx + 1];
        if (r >= 0) atomicAdd(&cnt[r], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CCL_PER; ++k) {
        const int ly = 4 * k + lw, gy = y0 + ly, c = (ly + 1) * CCL_PW + lx + 1;
        if (gx >= W || gy >= H) continue;
        const int r = lab[c];
        const int64_t g = base + (int64_t)gy * W + gx;
        labels[g] = r < 0 ? 0 : 1 + (y0 + r / CCL_PW - 1) * W + x0 + r % CCL_PW - 1;
        sizes[g] = r == c ? cnt[c] : 0;
    }
}

// the root below cell x of the plane L (x is set).  Values are 1 + an index <= the cell's own; anything else ends the walk, so it stays inside the plane whatever it reads.
__device__ __forceinline__ int ccl_find(const int* L, int x) {
    for (;;) {
        const int v = SEGX_TEAM_LOAD(L + x) - 1;
        if ((unsigned)v >= (unsigned)x) return x;
        x = v;
    }
}

// unite the sets of the set cells a and b (the argument for correctness and termination: head of this file)
__device__ __forceinline__ void ccl_union(int* L, int a, int b) {
    for (;;) {
        a = ccl_find(L, a); b = ccl_find(L, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(L + a, b + 1);
        if (old == a + 1 || old <= 0 || old > a) return;          // linked a root; (the other two: not a label of this plane -- never written by these kernels)
        a = old - 1;
    }
}

__device__ __forceinline__ bool ccl_set(const int* L, int i) { return SEGX_TEAM_LOAD(L + i) != 0; }

// One thread per seam pixel: the last column of every tile column but the last (all rows), then the last row of every tile row but the last (all columns).  A pixel whose
// straight neighbour across the seam is set unites with it alone: the diagonal ones touch that neighbour inside their tile or across a seam another thread handles.
__global__ __launch_bounds__(256) void ccl_seam_kernel(int* __restrict__ labels, int64_t planes, int H, int W) {
    const int nvs = (W - 1) / CCL_TW, nhs = (H - 1) / CCL_TH;
    const int64_t nv = (int64_t)nvs * H, per = nv + (int64_t)nhs * W, total = planes * per, HW = (int64_t)H * W;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
        const int64_t plane = it / per;
        int64_t r = it - plane * per;
        int* L = labels + plane * HW;
        if (r < nv) {
            const int k = (int)(r / H), y = (int)(r - (int64_t)k * H), a = y * W + (k + 1) * CCL_TW - 1;
            if (!ccl_set(L, a)) continue;
            if (ccl_set(L, a + 1)) ccl_union(L, a, a + 1);
            else {
                if (y > 0 && ccl_set(L, a + 1 - W)) ccl_union(L, a, a + 1 - W);
                if (y + 1 < H && ccl_set(L, a + 1 + W)) ccl_union(L, a, a + 1 + W);
            }
        } else {
            r -= nv;
            const int k = (int)(r / W), x = (int)(r - (int64_t)k * W), a = ((k + 1) * CCL_TH - 1) * W + x;
            if (!ccl_set(L, a)) continue;
            if (ccl_set(L, a + W)) ccl_union(L, a, a + W);
            else {
                if (x > 0 && ccl_set(L, a + W - 1)) ccl_union(L, a, a + W - 1);
                if (x + 1 < W && ccl_set(L, a + W + 1)) ccl_union(L, a, a + W + 1);
            }
        }
    }
}

// The union is complete (launch boundary): roots no longer change.  A store here may race with another thread's walk through the same cell; it too writes 1 + a member
// of the set that is not later, so the walk still ends on the root.  A count moves from a tile-local root that is not the final one; final roots are only added to.
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int* __restrict__ labels, int* __restrict__ sizes, int64_t planes, int HW) {
    const int64_t total = planes * HW;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t plane = idx / HW;
        const int i = (int)(idx - plane * HW);
        int* L = labels + plane * HW;
        if (!ccl_set(L, i)) continue;
        const int root = ccl_find(L, i);
        if (root == i) continue;
        L[i] = root + 1;
        const int s = sizes[idx];
        if (s) { atomicAdd(sizes + plane * HW + root, s); sizes[idx] = 0; }
    }
}

// ---- 3-D components ---------------------------------------------------------------------------------------------------------------------------
// Stacks of volumes [V][X][Y][Z], Z contiguous; 6- or 26-connectivity.  The three launches of the planes carry over: (a) ccl3_tile_kernel labels a
// C3_TX x C3_TY x C3_TZ tile in LDS to its fixed point (the tile's raster order is the volume's, so a tile-local root is the tile's first voxel of the component),
// (b) ccl3_seam_kernel unites across tile boundaries, (c) ccl_flatten_kernel -- the planes' own, a volume being a plane of X * Y * Z cells to it.
//
// The seam pass.  One thread per (axis A, voxel p on the last layer of a tile along A that has a layer p.A + 1 in the volume): if the straight neighbour s = p + e_A is
// set, unite(p, s) and nothing else; otherwise (26-connectivity) unite p with every set voxel among the other eight of the 3 x 3 patch around s in the layer p.A + 1.
// Every pair of adjacent set voxels in different tiles ends up united, by induction on the number d of coordinates in which the pair differs.  d = 1: the pair is
// straight across a seam, some thread's (p, s).  d > 1: the pair (p, q) crosses a seam along some axis A, p on the lower side; p's thread for A either finds s unset
// and unites (p, q) itself, or unites (p, s) -- and (s, q) are adjacent set voxels that differ in d - 1 coordinates: united inside their tile by (a), or by the
// induction.  Under 6-connectivity only d = 1 pairs are adjacent.  Pairs that touch only across a tile EDGE (d = 2, two seams) or a tile CORNER (d = 3, three seams) fall
// under the same rule.
// Termination is the argument at the head of this file word for word: the only writes are atomicMin(&L[a], b + 1) with b < a inside one volume's label array, labels only
// decrease, ccl_find walks a strictly decreasing sequence of indices of that volume, every round of ccl_union ends or lowers one of two positive integers, and the
// number of unions a thread attempts (at most 8) is fixed before it starts.  No thread waits for a value another thread has yet to write: there is no spin loop of
// any kind and no workgroup ever waits for another.
constexpr int C3_TX = SEGX_CCL3_TILE_X, C3_TY = SEGX_CCL3_TILE_Y, C3_TZ = SEGX_CCL3_TILE_Z;       // 8 x 8 x 32: rows of 128 bytes of float input
constexpr int C3_PZ = C3_TZ + 2, C3_SX = (C3_TY + 2) * C3_PZ, C3_PN = (C3_TX + 2) * C3_SX;       // the LDS tile with its one-voxel unset rim
static_assert(C3_TY * C3_TZ == 256, "a thread owns the column (y, z) of a tile: C3_TX voxels");

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void ccl3_tile_kernel(const T* __restrict__ fg, int bg, int* __restrict__ labels, int* __restrict__ sizes, int X, int Y, int Z,
                                                        int tiles_y, int tiles_z, int per_volume) {
    __shared__ int lab[C3_PN], cnt[C3_PN];
    __shared__ int changed[2];
    const int tid = threadIdx.x, lz = tid % C3_TZ, ly = tid / C3_TZ;
    const int64_t blk = blockIdx.x, vol = blk / per_volume;
    const int t = (int)(blk - vol * per_volume);
    const int x0 = (t / (tiles_y * tiles_z)) * C3_TX, y0 = ((t / tiles_z) % tiles_y) * C3_TY, z0 = (t % tiles_z) * C3_TZ;
    const int64_t base = vol * X * Y * Z;
    const int gy = y0 + ly, gz = z0 + lz, c0 = (ly + 1) * C3_PZ + lz + 1;
    const bool inside = gy < Y && gz < Z;
    const T bgv = (T)bg;
    for (int i = tid; i < C3_PN; i += 256) { lab[i] = -1; cnt[i] = 0; }
    if (tid < 2) changed[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < C3_TX; ++k) {
        const int c = (k + 1) * C3_SX + c0;
        if (inside && x0 + k < X && fg[base + ((int64_t)(x0 + k) * Y + gy) * Z + gz] != bgv) lab[c] = c;
    }
    __syncthreads();
    // label equivalence as in ccl_tile_kernel, over the 26 neighbours (FULL) or the 6 face neighbours
    for (int it = 0;; ++it) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < C3_TX; ++k) {
            const int c = (k + 1) * C3_SX + c0, r = lab[c];
            if (r < 0) continue;
            int m = r;
            if (FULL) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dz = -1; dz <= 1; ++dz) {
                            const int v = lab[c + dx * C3_SX + dy * C3_PZ + dz];
                            if (v >= 0 && v < m) m = v;
                        }
            } else {
#pragma unroll
                for (int n = 0; n < 6; ++n) {
                    const int v = lab[c + (n == 0 ? -C3_SX : n == 1 ? C3_SX : n == 2 ? -C3_PZ : n == 3 ? C3_PZ : n == 4 ? -1 : 1)];
                    if (v >= 0 && v < m) m = v;
                }
            }
            if (m < r) { atomicMin(&lab[r], m); any = true; }
        }
        if (any) changed[it & 1] = 1;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < C3_TX; ++k) {
            const int c = (k + 1) * C3_SX + c0;
            int r = lab[c];
            if (r < 0) continue;
            for (int v = lab[r]; v < r; v = lab[r]) r = v;       // cells hold values <= their own index: strictly down to a root
            lab[c] = r;
        }
        if (tid == 0) changed[(it + 1) & 1] = 0;                  // the other flag: nobody reads or sets it before the next barrier
        const int again = changed[it & 1];
        __syncthreads();
        if (!again) break;
    }
#pragma unroll
    for (int k = 0; k < C3_TX; ++k) {
        const int r = lab[(k + 1) * C3_SX + c0];
        if (r >= 0) atomicAdd(&cnt[r], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < C3_TX; ++k) {
        const int c = (k + 1) * C3_SX + c0;
        if (!inside || x0 + k >= X) continue;
        const int r = lab[c];
        const int64_t g = base + ((int64_t)(x0 + k) * Y + gy) * Z + gz;
        int label = 0;
        if (r >= 0) {
            const int rx = r / C3_SX - 1, ry = (r % C3_SX) / C3_PZ - 1, rz = r % C3_PZ - 1;
            label = 1 + ((x0 + rx) * Y + y0 + ry) * Z + z0 + rz;
        }
        labels[g] = label;
        sizes[g] = r == c ? cnt[c] : 0;
    }
}

template <bool FULL>
__global__ __launch_bounds__(256) void ccl3_seam_kernel(int* __restrict__ labels, int64_t volumes, int X, int Y, int Z) {
    const int64_t nx = (int64_t)((X - 1) / C3_TX) * Y * Z, ny = (int64_t)((Y - 1) / C3_TY) * X * Z, nz = (int64_t)((Z - 1) / C3_TZ) * X * Y;
    const int64_t per = nx + ny + nz, total = volumes * per, S = (int64_t)X * Y * Z;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
        const int64_t vol = it / per;
        int64_t r = it - vol * per;
        int* L = labels + vol * S;
        // a: the voxel; sA the stride along the seam's axis; (cB, cC), (sB, sC), (nB, nC): its coordinates, the strides and the extents along the two other axes
        int a, sA, sB, sC, cB, cC, nB, nC;
        if (r < nx) {
            const int k = (int)(r / ((int64_t)Y * Z)), rem = (int)(r - (int64_t)k * Y * Z);
            cB = rem / Z; cC = rem - cB * Z; nB = Y; nC = Z; sA = Y * Z; sB = Z; sC = 1;
            a = (((k + 1) * C3_TX - 1) * Y + cB) * Z + cC;
        } else if (r < nx + ny) {
            r -= nx;
            const int k = (int)(r / ((int64_t)X * Z)), rem = (int)(r - (int64_t)k * X * Z);
            cB = rem / Z; cC = rem - cB * Z; nB = X; nC = Z; sA = Z; sB = Y * Z; sC = 1;
            a = (cB * Y + (k + 1) * C3_TY - 1) * Z + cC;
        } else {
            r -= nx + ny;
            const int k = (int)(r / ((int64_t)X * Y)), rem = (int)(r - (int64_t)k * X * Y);
            cB = rem / Y; cC = rem - cB * Y; nB = X; nC = Y; sA = 1; sB = Y * Z; sC = Z;
            a = (cB * Y + cC) * Z + (k + 1) * C3_TZ - 1;
        }
        if (!ccl_set(L, a)) continue;
        const int s = a + sA;                                                       // inside the volume: k counts only the seams with a layer behind them
        if (ccl_set(L, s)) { ccl_union(L, a, s); continue; }
        if (!FULL) continue;
        for (int db = -1; db <= 1; ++db) {
            if ((unsigned)(cB + db) >= (unsigned)nB) continue;
            for (int dc = -1; dc <= 1; ++dc) {
                if ((db | dc) == 0 || (unsigned)(cC + dc) >= (unsigned)nC) continue;
                const int n = s + db * sB + dc * sC;
                if (ccl_set(L, n)) ccl_union(L, a, n);
            }
        }
    }
}

// ---- which components stay (3-D) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc3_zero_kernel(int* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

constexpr int C3_KEEP_MAX_CHUNKS = 1024;  // workgroups per volume of the largest-component reduction
constexpr int C3_FIRST = 0x7fffffff;      // stats[v][1] holds C3_FIRST - (first index of the largest component): a maximum again, so both words start at 0
// phase 0: stats[v][0] = the largest size of volume v; phase 1 (the next launch): stats[v][1] = the maximum of C3_FIRST - index over the cells whose size reaches it.
// A thread folds its share, the workgroup folds in LDS, ONE global atomicMax per workgroup.
__global__ __launch_bounds__(256) void cc3_largest_kernel(const int* __restrict__ sizes, int* __restrict__ stats, int S, int chunks, int phase) {
    __shared__ int best;
    const int64_t vol = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int* s = sizes + vol * S;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    const int top = phase ? stats[2 * vol] : 0;
    int m = 0;
    for (int64_t i = (int64_t)chunk * 256 + threadIdx.x; i < S; i += (int64_t)chunks * 256) {
        const int v = s[i];
        if (!phase) m = max(m, v);
        else if (v > 0 && v == top) m = max(m, C3_FIRST - (int)i);
    }
    if (m > 0) atomicMax(&best, m);
    __syncthreads();
    if (threadIdx.x == 0 && best > 0) atomicMax(stats + 2 * vol + phase, best);
}

__global__ __launch_bounds__(256) void cc3_keep_kernel(const int* __restrict__ labels, const int* __restrict__ sizes, const int* __restrict__ stats,
                                                       uint8_t* __restrict__ keep, int64_t volumes, int S, int min_voxels, int largest_only) {
    const int64_t total = volumes * S;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t vol = idx / S;
        const int l = labels[idx];
        bool k = false;
        if (l > 0 && l <= S) {                                                      // anything else is no label of this volume: not kept, and no read through it
            const int root = l - 1;
            k = sizes[vol * S + root] >= min_voxels && (!largest_only || root == C3_FIRST - stats[2 * vol + 1]);
        }
        keep[idx] = k ? 1 : 0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mask_apply_kernel(const T* __restrict__ src, const uint8_t* __restrict__ keep, T* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = keep[i] ? src[i] : (T)0;
}

// ---- the BraTS post-processing rule ---------------------------------------------------------------------------------------------------------------------------
// hard [4][S] = (bg, ET, WT, TC) as 0 / 1 floats; keep [S] bytes or NULL (= every voxel).  flag[0] += the number of voxels of ET . WT . keep: one LDS add per wave,
// one global add per workgroup.  The trip count is uniform over the wave only up to the tail, so the shuffles come after the loop.
__global__ __launch_bounds__(256) void brats_pp_count_kernel(const float* __restrict__ hard, const uint8_t* __restrict__ keep, int* __restrict__ flag, int64_t S) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int n = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256)
        n += (hard[S + i] != 0.0f && hard[2 * S + i] != 0.0f && (!keep || keep[i])) ? 1 : 0;
    for (int m = 32; m > 0; m >>= 1) n += __shfl_xor(n, m);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(flag, total);
}

// flag[0] is final (launch boundary): every thread forms the same decision from it, and one of them leaves it in flag[1] for the relabel pass and the caller.
__global__ __launch_bounds__(256) void brats_pp_apply_kernel(const float* __restrict__ hard, const uint8_t* __restrict__ keep, float* __restrict__ out,
                                                             int* __restrict__ flag, int64_t S, int et_min_voxels) {
    const bool drop = flag[0] < et_min_voxels;
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[1] = drop ? 1 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256) {
        const float wt = (!keep || keep[i]) ? hard[2 * S + i] : 0.0f;
        const bool in = wt != 0.0f;
        const float et = in && !drop ? hard[S + i] : 0.0f, tc = in ? hard[3 * S + i] : 0.0f;
        out[i] = et + wt + tc == 0.0f ? 1.0f : 0.0f;
        out[S + i] = et; out[2 * S + i] = wt; out[3 * S + i] = tc;
    }
}

__global__ __launch_bounds__(256) void brats_pp_relabel_kernel(const uint8_t* labels, const float* __restrict__ wt, const int* __restrict__ flag, uint8_t* out,
                                                               int64_t S) {                  // out may be labels: a thread reads a cell before it writes it
    const bool drop = flag[1] != 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256) {
        const uint8_t l = labels[i];
        out[i] = wt[i] == 0.0f ? (uint8_t)0 : (l == 4 && drop ? (uint8_t)1 : l);
    }
}

// ---- lesion-wise evaluation -------------------------------------------------------------------------------------------------------------------
// Stacks of region volumes [V][S].  How a voxel of a mask operand is read: KIND 1 = uint8, 4 = float32 (set = not 0; a NaN is set, as segx_ccl3d reads it),
// MASK_BRATS = ONE volume [S] of raw int32 BraTS labels shared by the three regions v = 0, 1, 2 = ET, WT, TC, mapped in registers as segx_brats_case_tail maps it
// (a raw 4 counts as 3; ET = 3, WT = 1, 2, 3, TC = 1, 3; any other value sets no region).
constexpr int MASK_BRATS = -4;
template <int KIND>
__device__ __forceinline__ bool mask_set(const void* p, int64_t S, int64_t v, int64_t i) {
    if (KIND == 1) return ((const uint8_t*)p)[v * S + i] != 0;
    if (KIND == 4) return ((const float*)p)[v * S + i] != 0.0f;
    int l = ((const int*)p)[i];
    if (l == 4) l = 3;
    return v == 0 ? l == 3 : v == 1 ? (l >= 1 && l <= 3) : (l == 1 || l == 3);
}

// One application of the 3 x 3 x 3 structuring element that holds the centre and its neighbours at L1 distance <= maxd (1 / 2 / 3 = 6 / 18 / 26 neighbours); voxels
// outside the volume are unset.  maxd = 0 copies the mask as bytes.  One workgroup per C3_TX x C3_TY x C3_TZ tile (the labelling's): the tile and its one-voxel rim
// go to LDS as bytes, 0 beyond the volume, so no neighbour test remains; a thread owns the column (y, z) of the tile and walks x with a window of three layers.  Of a
// layer it keeps three bits: the cell itself (distance 0 inside the layer), the OR of its 4 face neighbours inside the layer (1) and of the 4 diagonal ones (2); in the
// layer before and behind, those distances are one more.
constexpr int DL_PZ = C3_TZ + 2, DL_SX = (C3_TY + 2) * DL_PZ, DL_PN = (C3_TX + 2) * DL_SX;        // 10 x 10 x 34 bytes
template <int KIND>
__global__ __launch_bounds__(256) void dilate3_kernel(const void* __restrict__ src, uint8_t* __restrict__ out, int X, int Y, int Z, int tiles_y, int tiles_z,
                                                      int per_volume, int maxd) {
    __shared__ uint8_t m[DL_PN];
    const int tid = threadIdx.x, lz = tid % C3_TZ, ly = tid / C3_TZ;
    const int64_t blk = blockIdx.x, vol = blk / per_volume, S = (int64_t)X * Y * Z;
    const int t = (int)(blk - vol * per_volume);
    const int x0 = (t / (tiles_y * tiles_z)) * C3_TX, y0 = ((t / tiles_z) % tiles_y) * C3_TY, z0 = (t % tiles_z) * C3_TZ;
    for (int i = tid; i < DL_PN; i += 256) {
        const int px = i / DL_SX, r = i - px * DL_SX, py = r / DL_PZ, pz = r - py * DL_PZ;
        const int gx = x0 + px - 1, gy = y0 + py - 1, gz = z0 + pz - 1;
        bool s = false;
        if ((unsigned)gx < (unsigned)X && (unsigned)gy < (unsigned)Y && (unsigned)gz < (unsigned)Z) s = mask_set<KIND>(src, S, vol, ((int64_t)gx * Y + gy) * Z + gz);
        m[i] = s ? 1 : 0;
    }
    __syncthreads();
    const int gy = y0 + ly, gz = z0 + lz;
    if (gy >= Y || gz >= Z) return;                                                // behind the only barrier
    const uint8_t* col = m + (ly + 1) * DL_PZ + lz + 1;
    auto layer = [col](int px) -> int {
        const uint8_t* p = col + px * DL_SX;
        const int f = p[-1] | p[1] | p[-DL_PZ] | p[DL_PZ], e = p[-DL_PZ - 1] | p[-DL_PZ + 1] | p[DL_PZ - 1] | p[DL_PZ + 1];
        return p[0] | (f << 1) | (e << 2);
    };
    const int same_mask = maxd == 0 ? 1 : maxd == 1 ? 3 : 7, next_mask = maxd == 0 ? 0 : maxd == 1 ? 1 : maxd == 2 ? 3 : 7;
    int lo = layer(0), mid = layer(1);
#pragma unroll
    for (int k = 0; k < C3_TX; ++k) {
        const int hi = layer(k + 2);
        if (x0 + k < X) out[vol * S + ((int64_t)(x0 + k) * Y + gy) * Z + gz] = ((mid & same_mask) | ((lo | hi) & next_mask)) ? 1 : 0;
        lo = mid; mid = hi;
    }
}

// The workspace of segx_lesion_match / segx_lesion_reduce: per region LS_INTS words, then per region the touch matrix of LS_MAX_GT x LS_MAX_PRED bytes.
constexpr int LS_MAX_GT = SEGX_LESION_MAX_GT, LS_MAX_PRED = SEGX_LESION_MAX_PRED, LS_HEADER = SEGX_LESION_HEADER;
constexpr int LS_CNT = 4;                                                   // {lesion roots seen, predicted roots seen, overflow, unused}
constexpr int LS_INTS = LS_CNT + 3 * LS_MAX_GT + 2 * LS_MAX_PRED;
static_assert(LS_MAX_PRED % 4 == 0 && LS_INTS % 4 == 0, "touch rows are cleared as words");
struct LesionWs { int *cnt, *groot, *gvol, *tp, *psize, *matched; uint8_t* touch; };
__device__ __forceinline__ LesionWs lesion_ws(void* ws, int64_t volumes, int64_t v) {
    int* w = (int*)ws + v * LS_INTS;
    LesionWs r;
    r.cnt = w; r.groot = w + LS_CNT; r.gvol = r.groot + LS_MAX_GT; r.tp = r.gvol + LS_MAX_GT; r.psize = r.tp + LS_MAX_GT; r.matched = r.psize + LS_MAX_PRED;
    r.touch = (uint8_t*)((int*)ws + volumes * LS_INTS) + v * (int64_t)LS_MAX_GT * LS_MAX_PRED;
    return r;
}

// Compact ids.  A root cell (sizes > 0) draws its id from the region's counter and leaves 1 + id in its own cell of sizes: the cell becomes the map root -> id that the
// match pass reads through the labels, with no array of S words beside it.  The size of a predicted component moves to psize[id]; the size of a DILATED lesion is
// not used by anything.  The order of the ids is arbitrary; rows carry the root label.  A root past a cap gets no id (cell 0) and raises the overflow word.
// Roots are few (one atomic per component, not per voxel).
__global__ __launch_bounds__(256) void lesion_ids_kernel(int* __restrict__ gsizes, int* __restrict__ psizes, void* ws, int64_t volumes, int S) {
    const int64_t total = volumes * S;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t v = idx / S;
        const int gs = gsizes[idx], ps = psizes[idx];
        if (gs <= 0 && ps <= 0) continue;
        const LesionWs W = lesion_ws(ws, volumes, v);
        if (gs > 0) {
            const int id = atomicAdd(W.cnt, 1);
            if (id < LS_MAX_GT) { W.groot[id] = (int)(idx - v * S) + 1; gsizes[idx] = id + 1; }
            else { gsizes[idx] = 0; W.cnt[2] = 1; }
        }
        if (ps > 0) {
            const int id = atomicAdd(W.cnt + 1, 1);
            if (id < LS_MAX_PRED) { W.psize[id] = ps; psizes[idx] = id + 1; }
            else { psizes[idx] = 0; W.cnt[2] = 1; }
        }
    }
}

// the ids are final (launch boundary): clear the part of the touch matrix that can be written, rows < lesions, columns < components.  One workgroup per row.
__global__ __launch_bounds__(256) void lesion_clear_touch_kernel(void* ws, int64_t volumes) {
    const int64_t v = blockIdx.x / LS_MAX_GT;
    const int gid = blockIdx.x % LS_MAX_GT;
    const LesionWs W = lesion_ws(ws, volumes, v);
    if (gid >= min(W.cnt[0], LS_MAX_GT)) return;
    int* row = (int*)(W.touch + (int64_t)gid * LS_MAX_PRED);
    const int n = (min(W.cnt[1], LS_MAX_PRED) + 3) / 4;
    for (int t = threadIdx.x; t < n; t += 256) row[t] = 0;
}

// One pass over the voxels.  A voxel with a lesion label g and a component label p marks touch[id(g)][id(p)] with a plain store of 1 (idempotent: every writer stores
// the same byte).  A ground-truth voxel adds 1 to gvol[id(g)] and, where the prediction is set (p > 0), 1 to tp[id(g)].  Neighbouring voxels mostly belong to ONE
// lesion, so a wave folds its 64 voxels first: the lowest lane that still holds a count names its lesion, the lanes of that lesion are summed by shuffles, that lane
// issues the two atomics, and the round repeats while any lane is left -- one round for most waves, none for a wave without ground truth.  A wave walks whole groups of
// 64 cells, so every lane takes part in every shuffle; cells past the end carry nothing.
template <int KIND>
__global__ __launch_bounds__(256) void lesion_match_kernel(const void* __restrict__ gt, const int* __restrict__ GL, const int* __restrict__ gid_of,
                                                           const int* __restrict__ PL, const int* __restrict__ pid_of, void* ws, int64_t volumes, int S) {
    const int lane = threadIdx.x & 63;
    const int64_t total = volumes * S;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < total; base += (int64_t)gridDim.x * 256) {
        const int64_t idx = base + lane;
        int slot = -1, both = 0;                                                   // slot = v * LS_MAX_GT + id of the lesion this lane counts for
        if (idx < total) {
            const int64_t v = idx / S, i = idx - v * S;
            const int g = GL[idx];
            if (g > 0 && g <= S) {                                                  // anything else is no label of this volume: no read through it
                const int gid = gid_of[v * S + g - 1] - 1;
                if ((unsigned)gid < (unsigned)LS_MAX_GT) {
                    const int p = PL[idx];
                    const bool hit = p > 0 && p <= S;
                    if (hit) {
                        const int pid = pid_of[v * S + p - 1] - 1;
                        if ((unsigned)pid < (unsigned)LS_MAX_PRED) lesion_ws(ws, volumes, v).touch[(int64_t)gid * LS_MAX_PRED + pid] = 1;
                    }
                    if (mask_set<KIND>(gt, S, v, i)) { slot = (int)v * LS_MAX_GT + gid; both = hit ? 1 : 0; }
                }
            }
        }
        for (;;) {
            int first = slot >= 0 ? lane : 64;
            for (int m = 32; m > 0; m >>= 1) first = min(first, __shfl_xor(first, m));
            if (first == 64) break;                                                 // wave-uniform
            const int lead = __shfl(slot, first);
            const bool mine = slot == lead;
            int n = mine ? 1 + (both << 16) : 0;                                    // both counts stay below 2^16 in one word
            for (int m = 32; m > 0; m >>= 1) n += __shfl_xor(n, m);
            if (lane == first) {
                const LesionWs W = lesion_ws(ws, volumes, lead / LS_MAX_GT);
                atomicAdd(W.gvol + lead % LS_MAX_GT, n & 0xffff);
                if (n >> 16) atomicAdd(W.tp + lead % LS_MAX_GT, n >> 16);
            }
            if (mine) slot = -1;
        }
    }
}

// One workgroup per (region, lesion id): pvol = the sizes of the components of its touch row; every such component is marked matched (plain stores of 1).  The row
// (root label, tp, gvol, pvol) goes to the table; the rows past the last lesion are written as zeros.
__global__ __launch_bounds__(256) void lesion_rows_kernel(void* ws, int* __restrict__ rows, int64_t volumes) {
    __shared__ int total;
    const int64_t v = blockIdx.x / LS_MAX_GT;
    const int gid = blockIdx.x % LS_MAX_GT, tid = threadIdx.x;
    const LesionWs W = lesion_ws(ws, volumes, v);
    int* row = rows + ((int64_t)v * LS_MAX_GT + gid) * 4;
    if (gid >= min(W.cnt[0], LS_MAX_GT)) {                                          // uniform over the workgroup
        if (tid < 4) row[tid] = 0;
        return;
    }
    if (tid == 0) total = 0;
    __syncthreads();
    const int np = min(W.cnt[1], LS_MAX_PRED);
    const uint8_t* t = W.touch + (int64_t)gid * LS_MAX_PRED;
    int s = 0;
    for (int p = tid; p < np; p += 256)
        if (t[p]) { s += W.psize[p]; W.matched[p] = 1; }
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if ((tid & 63) == 0 && s) atomicAdd(&total, s);
    __syncthreads();
    if (tid == 0) { row[0] = W.groot[gid]; row[1] = W.tp[gid]; row[2] = W.gvol[gid]; row[3] = total; }
}

// matched is final (launch boundary).  One workgroup per region counts the components no lesion touches and writes the header.
__global__ __launch_bounds__(256) void lesion_header_kernel(void* ws, int* __restrict__ header, int64_t volumes) {
    __shared__ int nfp, fpv;
    const int64_t v = blockIdx.x;
    const int tid = threadIdx.x;
    const LesionWs W = lesion_ws(ws, volumes, v);
    if (tid == 0) { nfp = 0; fpv = 0; }
    __syncthreads();
    const int np = min(W.cnt[1], LS_MAX_PRED);
    int n = 0, s = 0;
    for (int p = tid; p < np; p += 256)
        if (!W.matched[p]) { ++n; s += W.psize[p]; }
    for (int m = 32; m > 0; m >>= 1) { n += __shfl_xor(n, m); s += __shfl_xor(s, m); }
    if ((tid & 63) == 0 && n) { atomicAdd(&nfp, n); atomicAdd(&fpv, s); }
    __syncthreads();
    if (tid < LS_HEADER) {
        const int over = (W.cnt[2] != 0 || W.cnt[0] > LS_MAX_GT || W.cnt[1] > LS_MAX_PRED) ? 1 : 0;
        header[v * LS_HEADER + tid] = tid == 0 ? W.cnt[0] : tid == 1 ? W.cnt[1] : tid == 2 ? nfp : tid == 3 ? fpv : tid == 4 ? over : 0;
    }
}

// ---- which labels stay ---------------------------------------------------------------------------------------------------------------------------------------
struct Top2 { int c1, l1, c2, l2; };                         // the best and the second candidate (count, label); count -1 = none
__device__ __forceinline__ bool frag_better(int ca, int la, int cb, int lb) { return ca > cb || (ca == cb && la < lb); }     // ties: the lower label (background = 0) first
__device__ __forceinline__ void frag_insert(Top2& t, int c, int l) {
    if (frag_better(c, l, t.c1, t.l1)) { t.c2 = t.c1; t.l2 = t.l1; t.c1 = c; t.l1 = l; }
    else if (frag_better(c, l, t.c2, t.l2)) { t.c2 = c; t.l2 = l; }
}

constexpr int KEEP_THREADS = 1024;
// One workgroup per plane: a thread folds its strided share of sizes[plane] into (sum, top two), then a fixed-order tree over LDS.  (count, label) is a total order,
// so the result does not depend on the order anyway.
__global__ __launch_bounds__(KEEP_THREADS) void frag_keep2_kernel(const int* __restrict__ sizes, int* __restrict__ keep, int HW) {
    __shared__ int sc1[KEEP_THREADS], sl1[KEEP_THREADS], sc2[KEEP_THREADS], sl2[KEEP_THREADS], ssum[KEEP_THREADS];
    const int tid = threadIdx.x;
    const int* s = sizes + (int64_t)blockIdx.x * HW;
    Top2 t{-1, 0x7fffffff, -1, 0x7fffffff};
    int sum = 0;
    int i = tid;
    for (; i + 3 * KEEP_THREADS < HW; i += 4 * KEEP_THREADS) {                      // four loads in flight per thread
        const int v0 = s[i], v1 = s[i + KEEP_THREADS], v2 = s[i + 2 * KEEP_THREADS], v3 = s[i + 3 * KEEP_THREADS];
        if (v0 | v1 | v2 | v3) {
            if (v0) { sum += v0; frag_insert(t, v0, i + 1); }
            if (v1) { sum += v1; frag_insert(t, v1, i + KEEP_THREADS + 1); }
            if (v2) { sum += v2; frag_insert(t, v2, i + 2 * KEEP_THREADS + 1); }
            if (v3) { sum += v3; frag_insert(t, v3, i + 3 * KEEP_THREADS + 1); }
        }
    }
    for (; i < HW; i += KEEP_THREADS) {
        const int v = s[i];
        if (v) { sum += v; frag_insert(t, v, i + 1); }
    }
    sc1[tid] = t.c1; sl1[tid] = t.l1; sc2[tid] = t.c2; sl2[tid] = t.l2; ssum[tid] = sum;
    __syncthreads();
    for (int h = KEEP_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            frag_insert(t, sc1[tid + h], sl1[tid + h]); frag_insert(t, sc2[tid + h], sl2[tid + h]);
            sum += ssum[tid + h];
            sc1[tid] = t.c1; sl1[tid] = t.l1; sc2[tid] = t.c2; sl2[tid] = t.l2; ssum[tid] = sum;
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (HW - sum > 0) frag_insert(t, HW - sum, 0);
        keep[2 * (int64_t)blockIdx.x] = t.c1 < 0 ? -1 : t.l1;
        keep[2 * (int64_t)blockIdx.x + 1] = t.c2 < 0 ? -1 : t.l2;
    }
}

__global__ __launch_bounds__(256) void frag_apply_kernel(const uint8_t* __restrict__ seg, const int* __restrict__ labels, const int* __restrict__ keep,
                                                         uint8_t* __restrict__ out, int64_t planes, int HW, int bg) {
    const int64_t total = planes * HW;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t plane = idx / HW;
        const int l = labels[idx];
        out[idx] = (l == 0 || l == keep[2 * plane] || l == keep[2 * plane + 1]) ? seg[idx] : (uint8_t)bg;
    }
}

// ---- row extents ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr int EXT_ROWS = 32;                 // rows of one plane a workgroup covers: a wave takes every fourth
__global__ __launch_bounds__(256) void row_extent_init_kernel(int* __restrict__ ext, int64_t planes, int H) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < planes; p += (int64_t)gridDim.x * 256) { ext[2 * p] = H; ext[2 * p + 1] = -1; }
}

__global__ __launch_bounds__(256) void row_extent_kernel(const float* __restrict__ mask, int* __restrict__ ext, int64_t planes, int H, int W, float thres) {
    __shared__ int lo_s, hi_s;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t groups = (H + EXT_ROWS - 1) / EXT_ROWS, items = planes * groups;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t plane = item / groups;
        const int y0 = (int)(item - plane * groups) * EXT_ROWS, y1 = min(y0 + EXT_ROWS, H);
        if (threadIdx.x == 0) { lo_s = H; hi_s = -1; }
        __syncthreads();
        int lo = H, hi = -1;
        for (int y = y0 + wave; y < y1; y += 4) {                                  // wave-uniform bounds: every lane takes part in the shuffles
            const float* row = mask + (plane * H + y) * W;
            int any = 0;
            for (int x = lane; x < W; x += 64) any |= row[x] >= thres ? 1 : 0;
            for (int m = 32; m > 0; m >>= 1) any |= __shfl_xor(any, m);
            if (any) { lo = min(lo, y); hi = max(hi, y); }
        }
        if (lane == 0 && hi >= 0) { atomicMin(&lo_s, lo); atomicMax(&hi_s, hi); }
        __syncthreads();
        if (threadIdx.x == 0 && hi_s >= 0) { atomicMin(ext + 2 * plane, lo_s); atomicMax(ext + 2 * plane + 1, hi_s); }
        __syncthreads();
    }
}

// ---- n-hot -> pixel values -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nhot_to_values_kernel(const float* __restrict__ nhot, const int* __restrict__ values, uint8_t* __restrict__ out, int64_t B,
                                                             int C, int64_t S) {
    const int64_t total = B * S;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / S, s = idx - b * S;
        const float* src = nhot + b * C * S + s;
        int v = 0;
        for (int c = 0; c < C; ++c)
            if (src[c * S] == 1.0f) v = values[c];                                 // ascending: a later class wins, as the reference's assignment order
        out[idx] = (uint8_t)v;
    }
}

}  // namespace segx

using namespace segx;
#define SEGX_STREAM hipStream_t stream = (hipStream_t)stream_

static inline unsigned grid_for(int64_t work) { return (unsigned)i64max(1, i64min(1 << 20, (work + 255) / 256)); }

extern "C" int segx_ccl2d(const uint8_t* fg, int bg_value, int32_t* labels, int32_t* sizes, int64_t planes, int H, int W, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(fg && labels && sizes, "segx_ccl2d: null pointer");
    SEGX_REQUIRE(planes > 0 && H > 0 && W > 0, "segx_ccl2d: planes, H and W must be positive");
    SEGX_REQUIRE((int64_t)H * W < SEGX_CCL_MAX_PLANE, "segx_ccl2d: H * W = %lld is not below the limit of 2^30 pixels per plane", (long long)H * W);
    SEGX_REQUIRE(bg_value >= 0 && bg_value <= 255, "segx_ccl2d: bg_value %d is no uint8 value", bg_value);
    const int tiles_x = (W + CCL_TW - 1) / CCL_TW, tiles_y = (H + CCL_TH - 1) / CCL_TH;
    const int64_t tiles = planes * tiles_x * tiles_y;
    SEGX_REQUIRE(tiles < ((int64_t)1 << 24), "segx_ccl2d: %lld tiles exceed one grid (2^24 workgroups of 256 threads)", (long long)tiles);
    hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, fg, bg_value, labels, sizes, H, W, tiles_x, tiles_y);
    const int64_t seam = planes * ((int64_t)((W - 1) / CCL_TW) * H + (int64_t)((H - 1) / CCL_TH) * W);
    if (seam > 0) {
        hipLaunchKernelGGL(ccl_seam_kernel, dim3(grid_for(seam)), dim3(256), 0, stream, labels, planes, H, W);
        hipLaunchKernelGGL(ccl_flatten_kernel, dim3(grid_for(planes * H * W)), dim3(256), 0, stream, labels, sizes, planes, H * W);
    }
    return check_launch("segx_ccl2d");
}

template <typename T>
static void ccl3_launch_tile(bool full, unsigned tiles, hipStream_t stream, const void* fg, int bg, int32_t* labels, int32_t* sizes, int X, int Y, int Z, int ty,
                             int tz, int per) {
    if (full) hipLaunchKernelGGL((ccl3_tile_kernel<T, true>), dim3(tiles), dim3(256), 0, stream, (const T*)fg, bg, labels, sizes, X, Y, Z, ty, tz, per);
    else hipLaunchKernelGGL((ccl3_tile_kernel<T, false>), dim3(tiles), dim3(256), 0, stream, (const T*)fg, bg, labels, sizes, X, Y, Z, ty, tz, per);
}

extern "C" int segx_ccl3d(const void* fg, int fg_bytes, int bg_value, int32_t* labels, int32_t* sizes, int64_t volumes, int X, int Y, int Z, int connectivity,
                          void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(fg && labels && sizes, "segx_ccl3d: null pointer");
    SEGX_REQUIRE(volumes > 0 && X > 0 && Y > 0 && Z > 0, "segx_ccl3d: volumes, X, Y and Z must be positive");
    const int64_t S = (int64_t)X * Y * Z;
    SEGX_REQUIRE(S < SEGX_CCL_MAX_PLANE, "segx_ccl3d: X * Y * Z = %lld is not below the limit of 2^30 voxels per volume", (long long)S);
    SEGX_REQUIRE(fg_bytes == 1 || fg_bytes == 4, "segx_ccl3d: fg_bytes %d is neither 1 (uint8) nor 4 (float32)", fg_bytes);
    SEGX_REQUIRE(connectivity == 6 || connectivity == 26, "segx_ccl3d: connectivity %d is neither 6 nor 26", connectivity);
    SEGX_REQUIRE(bg_value >= 0 && bg_value <= 255, "segx_ccl3d: bg_value %d is no uint8 value", bg_value);
    const int tx = (X + C3_TX - 1) / C3_TX, ty = (Y + C3_TY - 1) / C3_TY, tz = (Z + C3_TZ - 1) / C3_TZ;
    const int64_t per = (int64_t)tx * ty * tz, tiles = volumes * per;
    SEGX_REQUIRE(tiles < ((int64_t)1 << 24), "segx_ccl3d: %lld tiles exceed one grid (2^24 workgroups of 256 threads)", (long long)tiles);
    const bool full = connectivity == 26;
    if (fg_bytes == 1) ccl3_launch_tile<uint8_t>(full, (unsigned)tiles, stream, fg, bg_value, labels, sizes, X, Y, Z, ty, tz, (int)per);
    else ccl3_launch_tile<float>(full, (unsigned)tiles, stream, fg, bg_value, labels, sizes, X, Y, Z, ty, tz, (int)per);
    const int64_t seam = volumes * ((int64_t)((X - 1) / C3_TX) * Y * Z + (int64_t)((Y - 1) / C3_TY) * X * Z + (int64_t)((Z - 1) / C3_TZ) * X * Y);
    if (seam > 0) {
        if (full) hipLaunchKernelGGL(ccl3_seam_kernel<true>, dim3(grid_for(seam)), dim3(256), 0, stream, labels, volumes, X, Y, Z);
        else hipLaunchKernelGGL(ccl3_seam_kernel<false>, dim3(grid_for(seam)), dim3(256), 0, stream, labels, volumes, X, Y, Z);
        hipLaunchKernelGGL(ccl_flatten_kernel, dim3(grid_for(volumes * S)), dim3(256), 0, stream, labels, sizes, volumes, (int)S);
    }
    return check_launch("segx_ccl3d");
}

extern "C" int segx_cc3d_keep(const int32_t* labels, const int32_t* sizes, int32_t* stats, uint8_t* keep, int64_t volumes, int64_t S, int min_voxels,
                              int largest_only, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(labels && sizes && stats && keep, "segx_cc3d_keep: null pointer");
    SEGX_REQUIRE(volumes > 0 && S > 0, "segx_cc3d_keep: volumes and S must be positive");
    SEGX_REQUIRE(S < SEGX_CCL_MAX_PLANE, "segx_cc3d_keep: S = %lld is not below the limit of 2^30 voxels per volume", (long long)S);
    SEGX_REQUIRE(min_voxels >= 0, "segx_cc3d_keep: min_voxels %d is negative", min_voxels);
    const int chunks = (int)i64max(1, i64min(C3_KEEP_MAX_CHUNKS, (S + 2047) / 2048));         // a thread folds about eight cells
    SEGX_REQUIRE(volumes * chunks < ((int64_t)1 << 24), "segx_cc3d_keep: %lld volumes exceed one grid", (long long)volumes);
    if (largest_only) {
        hipLaunchKernelGGL(cc3_zero_kernel, dim3(grid_for(volumes * 2)), dim3(256), 0, stream, stats, volumes * 2);
        hipLaunchKernelGGL(cc3_largest_kernel, dim3((unsigned)(volumes * chunks)), dim3(256), 0, stream, sizes, stats, (int)S, chunks, 0);
        hipLaunchKernelGGL(cc3_largest_kernel, dim3((unsigned)(volumes * chunks)), dim3(256), 0, stream, sizes, stats, (int)S, chunks, 1);
    }
    hipLaunchKernelGGL(cc3_keep_kernel, dim3(grid_for(volumes * S)), dim3(256), 0, stream, labels, sizes, stats, keep, volumes, (int)S, min_voxels,
                       largest_only ? 1 : 0);
    return check_launch("segx_cc3d_keep");
}

extern "C" int segx_mask_apply(const void* src, int elem_bytes, const uint8_t* keep, void* out, int64_t n, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(src && keep && out, "segx_mask_apply: null pointer");
    SEGX_REQUIRE(n > 0, "segx_mask_apply: n must be positive");
    SEGX_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "segx_mask_apply: elem_bytes %d is not 1, 2, 4 or 8", elem_bytes);
    const dim3 grid(grid_for(n));                       // the elements move as integers of their width: an all-zero pattern is 0 in every type this serves
    if (elem_bytes == 1) hipLaunchKernelGGL(mask_apply_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t*)src, keep, (uint8_t*)out, n);
    else if (elem_bytes == 2) hipLaunchKernelGGL(mask_apply_kernel<uint16_t>, grid, dim3(256), 0, stream, (const uint16_t*)src, keep, (uint16_t*)out, n);
    else if (elem_bytes == 4) hipLaunchKernelGGL(mask_apply_kernel<uint32_t>, grid, dim3(256), 0, stream, (const uint32_t*)src, keep, (uint32_t*)out, n);
    else hipLaunchKernelGGL(mask_apply_kernel<uint64_t>, grid, dim3(256), 0, stream, (const uint64_t*)src, keep, (uint64_t*)out, n);
    return check_launch("segx_mask_apply");
}

extern "C" int segx_brats_postprocess(const float* hard, const uint8_t* keep, float* out, int32_t* flag, int64_t S, int et_min_voxels, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(hard && out && flag, "segx_brats_postprocess: null pointer");
    SEGX_REQUIRE(hard != out, "segx_brats_postprocess: out must not be hard");
    SEGX_REQUIRE(S > 0 && S < ((int64_t)1 << 31), "segx_brats_postprocess: S = %lld is not in 1 .. 2^31 - 1", (long long)S);
    SEGX_REQUIRE(et_min_voxels >= 0, "segx_brats_postprocess: et_min_voxels %d is negative", et_min_voxels);
    hipLaunchKernelGGL(cc3_zero_kernel, dim3(1), dim3(256), 0, stream, flag, (int64_t)2);
    hipLaunchKernelGGL(brats_pp_count_kernel, dim3((unsigned)i64min(4096, (S + 255) / 256)), dim3(256), 0, stream, hard, keep, flag, S);
    hipLaunchKernelGGL(brats_pp_apply_kernel, dim3(grid_for(S)), dim3(256), 0, stream, hard, keep, out, flag, S, et_min_voxels);
    return check_launch("segx_brats_postprocess");
}

extern "C" int segx_brats_relabel(const uint8_t* labels, const float* wt, const int32_t* flag, uint8_t* out, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(labels && wt && flag && out, "segx_brats_relabel: null pointer");
    SEGX_REQUIRE(S > 0 && S < ((int64_t)1 << 31), "segx_brats_relabel: S = %lld is not in 1 .. 2^31 - 1", (long long)S);
    hipLaunchKernelGGL(brats_pp_relabel_kernel, dim3(grid_for(S)), dim3(256), 0, stream, labels, wt, flag, out, S);
    return check_launch("segx_brats_relabel");
}

// the KIND of a mask operand (mask_set) from the ABI's (bytes, map) pair; 0 = refused
static int lesion_mask_kind(int bytes, int map, int64_t volumes) {
    if (map == SEGX_LESION_MAP_NONE) return bytes == 1 || bytes == 4 ? bytes : 0;
    return map == SEGX_LESION_MAP_BRATS && bytes == 4 && volumes == 3 ? MASK_BRATS : 0;
}

extern "C" int64_t segx_lesion_ws_bytes(int64_t volumes) {
    return volumes < 1 ? 0 : volumes * ((int64_t)LS_INTS * 4 + (int64_t)LS_MAX_GT * LS_MAX_PRED);
}

extern "C" int segx_dilate3d(const void* src, int src_bytes, int src_map, uint8_t* out, uint8_t* tmp, int64_t volumes, int X, int Y, int Z, int connectivity,
                             int iters, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(src && out, "segx_dilate3d: null pointer");
    SEGX_REQUIRE(volumes > 0 && X > 0 && Y > 0 && Z > 0, "segx_dilate3d: volumes, X, Y and Z must be positive");
    const int64_t S = (int64_t)X * Y * Z;
    SEGX_REQUIRE(S < SEGX_CCL_MAX_PLANE, "segx_dilate3d: X * Y * Z = %lld is not below the limit of 2^30 voxels per volume", (long long)S);
    const int kind = lesion_mask_kind(src_bytes, src_map, volumes);
    SEGX_REQUIRE(kind != 0, "segx_dilate3d: src_bytes %d with src_map %d over %lld volumes is no mask operand (uint8 / float32, or the raw BraTS labels: int32, 3 regions)",
                 src_bytes, src_map, (long long)volumes);
    SEGX_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "segx_dilate3d: connectivity %d is not 6, 18 or 26", connectivity);
    SEGX_REQUIRE(iters >= 0, "segx_dilate3d: iters %d is negative", iters);
    SEGX_REQUIRE(iters < 2 || (tmp && tmp != out), "segx_dilate3d: two or more iterations need tmp, another buffer than out");
    SEGX_REQUIRE((const void*)out != src && (const void*)tmp != src, "segx_dilate3d: out and tmp must not be src");
    const int maxd = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    const int ty = (Y + C3_TY - 1) / C3_TY, tz = (Z + C3_TZ - 1) / C3_TZ;
    const int64_t per = (int64_t)((X + C3_TX - 1) / C3_TX) * ty * tz, tiles = volumes * per;
    SEGX_REQUIRE(tiles < ((int64_t)1 << 24), "segx_dilate3d: %lld tiles exceed one grid (2^24 workgroups of 256 threads)", (long long)tiles);
    const dim3 grid((unsigned)tiles);
    // pass k of n writes out when n - 1 - k is even, so the last one lands in out; pass 0 reads src in its own type, the others the bytes of the pass before
    const int n = iters > 0 ? iters : 1;
    uint8_t* first = (n - 1) % 2 == 0 ? out : tmp;
    const int d0 = iters > 0 ? maxd : 0;
    if (kind == 1) hipLaunchKernelGGL(dilate3_kernel<1>, grid, dim3(256), 0, stream, src, first, X, Y, Z, ty, tz, (int)per, d0);
    else if (kind == 4) hipLaunchKernelGGL(dilate3_kernel<4>, grid, dim3(256), 0, stream, src, first, X, Y, Z, ty, tz, (int)per, d0);
    else hipLaunchKernelGGL(dilate3_kernel<MASK_BRATS>, grid, dim3(256), 0, stream, src, first, X, Y, Z, ty, tz, (int)per, d0);
    for (int k = 1; k < n; ++k) {
        uint8_t* from = (n - k) % 2 == 0 ? out : tmp;
        uint8_t* to = from == out ? tmp : out;
        hipLaunchKernelGGL(dilate3_kernel<1>, grid, dim3(256), 0, stream, (const void*)from, to, X, Y, Z, ty, tz, (int)per, maxd);
    }
    return check_launch("segx_dilate3d");
}

extern "C" int segx_lesion_match(const void* gt, int gt_bytes, int gt_map, const int32_t* gl, int32_t* gsizes, const int32_t* pl, int32_t* psizes, void* ws,
                                 int64_t volumes, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(gt && gl && gsizes && pl && psizes && ws, "segx_lesion_match: null pointer");
    SEGX_REQUIRE(volumes > 0 && volumes <= 65535 && S > 0, "segx_lesion_match: 1 <= volumes <= 65535 and S > 0");
    SEGX_REQUIRE(S < SEGX_CCL_MAX_PLANE, "segx_lesion_match: S = %lld is not below the limit of 2^30 voxels per volume", (long long)S);
    SEGX_REQUIRE(((uintptr_t)ws & 15) == 0, "segx_lesion_match: ws must be 16-byte aligned");
    const int kind = lesion_mask_kind(gt_bytes, gt_map, volumes);
    SEGX_REQUIRE(kind != 0, "segx_lesion_match: gt_bytes %d with gt_map %d over %lld volumes is no mask operand (uint8 / float32, or the raw BraTS labels: int32, 3 regions)",
                 gt_bytes, gt_map, (long long)volumes);
    const dim3 grid(grid_for(volumes * S)), rows((unsigned)(volumes * LS_MAX_GT));
    hipLaunchKernelGGL(cc3_zero_kernel, dim3(grid_for(volumes * LS_INTS)), dim3(256), 0, stream, (int*)ws, volumes * LS_INTS);
    hipLaunchKernelGGL(lesion_ids_kernel, grid, dim3(256), 0, stream, gsizes, psizes, ws, volumes, (int)S);
    hipLaunchKernelGGL(lesion_clear_touch_kernel, rows, dim3(256), 0, stream, ws, volumes);
    if (kind == 1) hipLaunchKernelGGL(lesion_match_kernel<1>, grid, dim3(256), 0, stream, gt, gl, (const int*)gsizes, pl, (const int*)psizes, ws, volumes, (int)S);
    else if (kind == 4) hipLaunchKernelGGL(lesion_match_kernel<4>, grid, dim3(256), 0, stream, gt, gl, (const int*)gsizes, pl, (const int*)psizes, ws, volumes, (int)S);
    else hipLaunchKernelGGL(lesion_match_kernel<MASK_BRATS>, grid, dim3(256), 0, stream, gt, gl, (const int*)gsizes, pl, (const int*)psizes, ws, volumes, (int)S);
    return check_launch("segx_lesion_match");
}

extern "C" int segx_lesion_reduce(void* ws, int32_t* rows, int32_t* header, int64_t volumes, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(ws && rows && header, "segx_lesion_reduce: null pointer");
    SEGX_REQUIRE(volumes > 0 && volumes <= 65535, "segx_lesion_reduce: 1 <= volumes <= 65535");
    hipLaunchKernelGGL(lesion_rows_kernel, dim3((unsigned)(volumes * LS_MAX_GT)), dim3(256), 0, stream, ws, rows, volumes);
    hipLaunchKernelGGL(lesion_header_kernel, dim3((unsigned)volumes), dim3(256), 0, stream, ws, header, volumes);
    return check_launch("segx_lesion_reduce");
}

extern "C" int segx_frag_keep2(const int32_t* sizes, int32_t* keep, int64_t planes, int H, int W, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(sizes && keep, "segx_frag_keep2: null pointer");
    SEGX_REQUIRE(planes > 0 && H > 0 && W > 0, "segx_frag_keep2: planes, H and W must be positive");
    SEGX_REQUIRE(planes < ((int64_t)1 << 22), "segx_frag_keep2: %lld planes exceed one grid (2^22 workgroups of 1024 threads)", (long long)planes);
    SEGX_REQUIRE((int64_t)H * W < SEGX_CCL_MAX_PLANE, "segx_frag_keep2: H * W = %lld is not below the limit of 2^30 pixels per plane", (long long)H * W);
    hipLaunchKernelGGL(frag_keep2_kernel, dim3((unsigned)planes), dim3(KEEP_THREADS), 0, stream, sizes, keep, H * W);
    return check_launch("segx_frag_keep2");
}

extern "C" int segx_frag_apply(const uint8_t* seg, const int32_t* labels, const int32_t* keep, uint8_t* out, int64_t planes, int H, int W, int bg_value,
                               void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(seg && labels && keep && out, "segx_frag_apply: null pointer");
    SEGX_REQUIRE(planes > 0 && H > 0 && W > 0, "segx_frag_apply: planes, H and W must be positive");
    SEGX_REQUIRE((int64_t)H * W < SEGX_CCL_MAX_PLANE, "segx_frag_apply: H * W = %lld is not below the limit of 2^30 pixels per plane", (long long)H * W);
    SEGX_REQUIRE(bg_value >= 0 && bg_value <= 255, "segx_frag_apply: bg_value %d is no uint8 value", bg_value);
    hipLaunchKernelGGL(frag_apply_kernel, dim3(grid_for(planes * H * W)), dim3(256), 0, stream, seg, labels, keep, out, planes, H * W, bg_value);
    return check_launch("segx_frag_apply");
}

extern "C" int segx_row_extent(const float* mask, int32_t* ext, int64_t planes, int H, int W, float thres, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(mask && ext, "segx_row_extent: null pointer");
    SEGX_REQUIRE(planes > 0 && H > 0 && W > 0, "segx_row_extent: planes, H and W must be positive");
    SEGX_REQUIRE((int64_t)H * W < SEGX_CCL_MAX_PLANE, "segx_row_extent: H * W = %lld is not below the limit of 2^30 pixels per plane", (long long)H * W);
    hipLaunchKernelGGL(row_extent_init_kernel, dim3(grid_for(planes)), dim3(256), 0, stream, ext, planes, H);
    const int64_t items = planes * ((H + EXT_ROWS - 1) / EXT_ROWS);
    hipLaunchKernelGGL(row_extent_kernel, dim3((unsigned)i64min(1 << 20, items)), dim3(256), 0, stream, mask, ext, planes, H, W, thres);
    return check_launch("segx_row_extent");
}

extern "C" int segx_nhot_to_values(const float* nhot, const int32_t* values, uint8_t* out, int64_t B, int C, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(nhot && values && out, "segx_nhot_to_values: null pointer");
    SEGX_REQUIRE(B > 0 && C > 0 && S > 0, "segx_nhot_to_values: B, C and S must be positive");
    hipLaunchKernelGGL(nhot_to_values_kernel, dim3(grid_for(B * S)), dim3(256), 0, stream, nhot, values, out, B, C, S);
    return check_launch("segx_nhot_to_values");
}
